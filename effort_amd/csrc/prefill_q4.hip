// Prompt prefill straight from the Q4 buckets: the Q4 twin of prefill_buckets.hip.  The block multiply of prefill.hip with the A operand
// de-quantised on the fly, so a Q4 model prefills with no f16 core of a Q4 bundle in memory, and its caches hold the K / V a Q4 decode
// at effort 1.0 would write.
//
//   q4_gemm_rows        out[r] = U4[e] * f16(x[r]) for rows r of a block, U4 the un-bucketed matrix of expert e (below)
//   q4_outlier_rows     out[r][o] += sum over the handle's outliers on output o of value * x[r][input]  (f32 x, as calcOutliers)
//   q4_dense_check      decides once per handle whether a bundle IS un-bucketable, and writes the compact f16 means
//
// U4.  Bucket row i = 8 j + r of an expert holds rank r of input j: outDim / 32 16-bit words, word x four nibbles, the first in bits
// 15 .. 12, nibble n = sign << 3 | pos naming output 32 x + 8 n + pos.  U4[32 x + 8 n + pos][j] = +-f16(m), m = stats[i].y (the lane
// prepareDispatchQ4 reads), a clear sign bit +.  A bundle is un-bucketable iff the eight ranks of every (e, j, x, n) name eight
// different positions and every mean is a finite f16 number stored as f32: every element of U4 is then named exactly once.
//
// CONTRACT: the bits are effort_dense_gemm_rows's with U4[e] as its matrix -- prefill_buckets.hip's CONTRACT word for word: pf_split's
// k split, reduce_splits_kernel, every accumulator's MFMA steps in ascending (stage of 256, chunk of 64, u) order, for step (chunk, u)
// lane group g on elements 64 chunk + 16 g + 8 u + 0 .. 7, f16(x) from rows_to_f16_kernel, a dead token column and a k past inDim zero
// operands, the dead steps of a last stage still taken.  The outlier term is added afterwards, per (output, token) by one lane,
// fmaf by fmaf in the order of the handle's outlier index (OutlierIndex: an output's entries in table order): a function of the
// handle and the row alone, never of `rows`.
//
// The tiling.  A workgroup owns kQbWords = 16 consecutive words of every bucket row -- 32 bytes, 512 outputs -- and one k split; the
// other choice, 64 bytes and 1024 outputs, needs a 147 KB tile and halves the workgroups of a kernel that already has too few
// (outDim / 512 per split).  Per chunk of 64 k the 8 x 64 bucket rows are 512: ONE ROW PER THREAD, its 32 bytes and its mean -- two
// 16-byte loads where every piece is one (pitch % 16 == 0, 16-byte aligned buckets, words % 8 == 0), sixteen 2-byte loads otherwise
// (a row of an odd word count -- outDim 32, 96, 1056 -- is only 2-byte aligned).  The thread scatters its 64 nibbles as sign ^ f16(m)
// into the LDS tile [512 outputs][64 k] (2-byte stores, pitch 144 bytes as in prefill_buckets.hip), the 8 waves read their A fragments
// back as 16-byte LDS reads.  Every tile element of a live k and a live word is written exactly once per chunk, so the tile is
// zeroed ONCE, at kernel start: a column k >= inDim of a last chunk keeps what the chunk before left (finite) and meets zero x
// operands; the rows of a ragged last workgroup's dead words stay +0 and are never stored.  Nothing outside the expert's payload is
// read: the descriptor ends with its last row, a piece is asked for only when it lies inside the row.
//
// Measured (profiles/r13_prefill_q4.json; core / FP16 bucket kernel / this multiply / with the 2 % outliers' pass, us per call at 64
// rows): 4096 x 4096 19.5 / 104.4 / 67.1 / 150.3; 14336 -> 4096 50.1 / 322.5 / 255.7 / 569.7.  The multiply is bound by the scatter
// and the small grid as the FP16 bucket kernel is; the outlier pass, a gather of one f32 of x per outlier and token, costs as much again.
#include "prefill.h"

namespace effort {

constexpr uint32_t kQbWords = 16;                   // 16-bit words of a bucket row a workgroup owns
constexpr uint32_t kQbRows = 32u * kQbWords;        // ... the outputs they name
constexpr uint32_t kQbWaves = 8, kQbThreads = 64u * kQbWaves;
constexpr uint32_t kQbTiles = kQbRows / 16u / kQbWaves;   // 16-row MFMA tiles per wave
constexpr uint32_t kQbK = 64;                       // k per LDS stage: one chunk of the core kernel's stage
constexpr uint32_t kQbPitch = kQbK * 2u + 16u;      // bytes per tile row (and per staged token row)
constexpr uint32_t kQbTileBytes = kQbRows * kQbPitch;
constexpr uint32_t kQbLds = kQbTileBytes + 64u * kQbPitch;      // the A tile, then up to 64 token rows
static_assert(kPfStage % kQbK == 0 && kQbTileBytes % (16u * kQbThreads) == 0, "whole chunks per stage; the fill is whole 16-byte stores");
static_assert(8u * kQbK == kQbThreads, "one bucket row of a chunk per thread");

// grid = (groups of kQbWords words, splits).  NT = token tiles (of 16), AUX = cache policy of the bucket loads (0, or 2 = nt), WIDE =
// 16-byte row pieces.  B = ONE expert's buckets (bucket row i at byte i * pitch, `words` payload words each), means = its f16 row
// means (one u16 per bucket row).  dst = out when there is one split, else the partial sums [splits][rows][outDim].
template <int NT, int AUX, bool WIDE>
__global__ __launch_bounds__(kQbThreads) void q4_gemm_rows_kernel(const uint16_t* __restrict__ B, uint32_t pitch, uint32_t words,
                                                                  const uint16_t* __restrict__ means, const uint16_t* __restrict__ xh,
                                                                  float* __restrict__ dst, uint32_t inDim, uint32_t outDim, uint32_t rows,
                                                                  uint32_t per) {
    extern __shared__ __attribute__((aligned(16))) unsigned char qb_lds[];
    constexpr uint32_t kXPieces = NT * 16u * (kQbK / 8u);                               // 16-byte pieces of the staged token rows
    constexpr int kXLoads = (int)((kXPieces + kQbThreads - 1u) / kQbThreads);
    constexpr int kDepth = 2;                                                           // chunks of loads in flight
    unsigned char* const tile = qb_lds;
    unsigned char* const xs = qb_lds + kQbTileBytes;
    float* const o = dst + (size_t)blockIdx.y * rows * outDim;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t g = lane >> 4, r16 = lane & 15u, w0 = blockIdx.x * kQbWords, jj = tid >> 3;
    // the descriptor ends with the payload of the expert's last bucket row
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(B), 0, (int)((8u * inDim - 1u) * pitch + words * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t mr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(means), 0, (int)(8u * inDim * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(xh), 0, (int)(rows * inDim * 2u), 0x00020000);
    const uint32_t chunks = (inDim + kPfStage - 1u) / kPfStage * (kPfStage / kQbK);    // every chunk of every stage, the dead ones of the last stage too
    const uint32_t q0 = blockIdx.y * per * (kPfStage / kQbK), q1 = min(q0 + per * (kPfStage / kQbK), chunks);

    uint32_t heldA[kDepth][kQbWords / 2u], heldM[kDepth];
    uint4 heldX[kDepth][kXLoads];
    // bucket row 8 (64 q) + tid of the chunk: rank tid & 7 of input 64 q + jj.  Words past the row's payload, a row past inDim: not asked for.
    auto ask_a = [&](uint32_t q, uint32_t (&a)[kQbWords / 2u], uint32_t& m) {
#pragma unroll
        for (int i = 0; i < (int)(kQbWords / 2u); i++) a[i] = 0u;
        m = 0u;
        if (q * kQbK + jj >= inDim) return;
        const uint32_t brow = q * (8u * kQbK) + tid, off = brow * pitch + w0 * 2u;
        if constexpr (WIDE) {                                                            // (words % 8 == 0: a piece is inside the payload or outside)
#pragma unroll
            for (int h = 0; h < 2; h++)
                if (w0 + 8u * h + 8u <= words) {
                    const auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, off + 16u * h, 0, AUX);
                    a[4 * h] = w[0]; a[4 * h + 1] = w[1]; a[4 * h + 2] = w[2]; a[4 * h + 3] = w[3];
                }
        } else {
#pragma unroll
            for (int i = 0; i < (int)kQbWords; i++)
                if (w0 + (uint32_t)i < words) a[i / 2] |= (uint32_t)__builtin_amdgcn_raw_buffer_load_b16(rs, off + 2u * i, 0, AUX) << (16 * (i & 1));
        }
        m = __builtin_amdgcn_raw_buffer_load_b16(mr, brow * 2u, 0, 0);
    };
    auto ask_x = [&](uint32_t q, uint4 (&nextX)[kXLoads]) {
#pragma unroll
        for (int i = 0; i < kXLoads; i++) {
            const uint32_t idx = tid + (uint32_t)i * kQbThreads, tok = idx / (kQbK / 8u), e = q * kQbK + (idx % (kQbK / 8u)) * 8u;
            nextX[i] = make_uint4(0u, 0u, 0u, 0u);
            if (idx < kXPieces && tok < rows && e < inDim) {                             // a dead column, a k past inDim: zeros are staged (inDim % 8 == 0)
                const auto x = __builtin_amdgcn_raw_buffer_load_b128(xr, tok * inDim * 2u + e * 2u, 0, 0);
                nextX[i] = make_uint4(x[0], x[1], x[2], x[3]);
            }
        }
    };
    // nibble n of word i names tile row 32 i + 8 n + pos (< kQbRows); its value is the row's mean with the nibble's sign
    auto scatter = [&](uint32_t q, const uint32_t (&a)[kQbWords / 2u], uint32_t m, const uint4 (&nextX)[kXLoads]) {
        if (q * kQbK + jj < inDim) {
#pragma unroll
            for (int i = 0; i < (int)kQbWords; i++) {
                if (w0 + (uint32_t)i >= words) continue;
                const uint32_t w = (a[i / 2] >> (16 * (i & 1))) & 0xFFFFu;
#pragma unroll
                for (int n = 0; n < 4; n++) {
                    const uint32_t nib = (w >> (12 - 4 * n)) & 15u, row = 32u * i + 8u * n + (nib & 7u);
                    *reinterpret_cast<uint16_t*>(tile + row * kQbPitch + jj * 2u) = (uint16_t)(m ^ ((nib & 8u) << 12));
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kXLoads; i++) {
            const uint32_t idx = tid + (uint32_t)i * kQbThreads;
            if (idx < kXPieces) *reinterpret_cast<uint4*>(xs + (idx / (kQbK / 8u)) * kQbPitch + (idx % (kQbK / 8u)) * 16u) = nextX[i];
        }
    };

    pf_f32x4 acc[kQbTiles][NT];
#pragma unroll
    for (int m = 0; m < (int)kQbTiles; m++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[m][t] = pf_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // one chunk: scatter what `slot` holds, ask for chunk q + kDepth into the freed slot, multiply
    auto chunk = [&](uint32_t q, auto slotTag) {
        constexpr int slot = decltype(slotTag)::value;
        scatter(q, heldA[slot], heldM[slot], heldX[slot]);
        __syncthreads();
        if (q + kDepth < q1) { ask_a(q + kDepth, heldA[slot], heldM[slot]); ask_x(q + kDepth, heldX[slot]); }   // the later chunks' loads run under this chunk's products
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 2; u++) {
            pf_half8 bf[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) bf[t] = *reinterpret_cast<const pf_half8*>(xs + (t * 16u + r16) * kQbPitch + (g * 2u + u) * 16u);
#pragma unroll
            for (int m = 0; m < (int)kQbTiles; m++) {
                const pf_half8 af = *reinterpret_cast<const pf_half8*>(tile + ((wave * kQbTiles + m) * 16u + r16) * kQbPitch + (g * 2u + u) * 16u);
#pragma unroll
                for (int t = 0; t < NT; t++) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[t], acc[m][t], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                                                 // the tile and the token rows are rewritten by the next chunk
    };
    ask_a(q0, heldA[0], heldM[0]);
    ask_x(q0, heldX[0]);
    if (q0 + 1u < q1) { ask_a(q0 + 1u, heldA[1], heldM[1]); ask_x(q0 + 1u, heldX[1]); }
#pragma unroll
    for (int i = 0; i < (int)(kQbTileBytes / (16u * kQbThreads)); i++)                  // ONCE: what no entry ever lands on must not be NaN or Inf
        *reinterpret_cast<uint4*>(tile + (tid + (uint32_t)i * kQbThreads) * 16u) = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    for (uint32_t q = q0; q < q1; q += 2u) {                                             // (uniform; the slots alternate with static indices: registers)
        chunk(q, std::integral_constant<int, 0>{});
        if (q + 1u < q1) chunk(q + 1u, std::integral_constant<int, 1>{});
    }
    // Accumulator register i of lane l is tile row 4 * (l >> 4) + i, token l & 15.
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t tok = t * 16u + r16;
#pragma unroll
        for (int m = 0; m < (int)kQbTiles; m++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t row = w0 * 32u + (wave * kQbTiles + m) * 16u + g * 4u + i;
                if (tok < rows && row < outDim) o[(size_t)tok * outDim + row] = acc[m][t][i];
            }
    }
}

// The outlier term, after the splits were reduced.  grid = (blocks of 64 outputs, groups of 4 * kOlTok tokens), 4 waves; a wave takes
// one block of the index and kOlTok tokens, lane i the output of rank i: it walks that output's entries in the index's order (step k
// of the block is one contiguous load, lane i <-> rank i, the cursor advancing by the step's population -- ol_jds_kernel's layout)
// and adds value * x[token][input] to ITS sums by fmaf, starting from what the multiply wrote.  No atomics; a lane whose output has no
// outlier writes nothing.  x is the f32 input.
constexpr uint32_t kOlTok = 4;
__global__ __launch_bounds__(256) void q4_outlier_rows_kernel(OutlierIndex ol, const float* __restrict__ x, float* __restrict__ out, uint32_t inDim,
                                                              uint32_t outDim, uint32_t rows) {
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), b = blockIdx.x;
    const uint32_t t0 = (blockIdx.y * 4u + wave) * kOlTok;
    if (t0 >= rows) return;                                                              // (uniform per wave)
    const uint32_t meta = ol.meta[(size_t)b * 64u + lane], len = meta >> 8, outIdx = b * 64u + (meta & 255u);
    const uint32_t steps = (uint32_t)__builtin_amdgcn_readfirstlane((int)len);          // rank 0 has the most entries
    if (steps == 0u) return;
    const bool mine = len > 0u && outIdx < outDim;
    uint32_t tok[kOlTok];
    float acc[kOlTok];
#pragma unroll
    for (int t = 0; t < (int)kOlTok; t++) {
        tok[t] = min(t0 + (uint32_t)t, rows - 1u);                                       // a token past the block re-reads the last one; not written
        acc[t] = mine ? out[(size_t)tok[t] * outDim + outIdx] : 0.0f;
    }
    uint32_t cur = __builtin_amdgcn_readfirstlane(ol.blockPtr[b]);
    for (uint32_t k = 0; k < steps; k++) {                                               // (uniform)
        const bool active = len > k;
        if (active) {
            const uint32_t ent = ol.entry[cur + lane];
            const float val = half_bits_to_float((uint16_t)(ent >> 16));
            const uint32_t in = min(ent & 0xFFFFu, inDim - 1u);
#pragma unroll
            for (int t = 0; t < (int)kOlTok; t++) acc[t] = fmaf(val, x[(size_t)tok[t] * inDim + in], acc[t]);
        }
        cur += (uint32_t)__popcll(__ballot(active));
    }
    if (!mine) return;
#pragma unroll
    for (int t = 0; t < (int)kOlTok; t++)
        if (t0 + (uint32_t)t < rows) out[(size_t)(t0 + t) * outDim + outIdx] = acc[t];
}

// Is the bundle un-bucketable?  One thread per (word, input, expert) reads its 8 ranks' word (2-byte loads: rows may be 2-byte
// aligned) and marks the positions of the four nibbles; a position named twice raises bad[0] (8 ranks on 8 positions: no duplicate
// IS a permutation).  The threads of word 0 also judge the 8 means of their input -- lane .y of the f32 x 2 stats, the only lane read
// -- and write them as f16 to means16: a mean that is not a finite f16 number raises bad[1].  Only payload bytes are read.
__global__ __launch_bounds__(256) void q4_dense_check_kernel(const uint16_t* __restrict__ B, uint32_t pitch, uint32_t words, const float* __restrict__ stats,
                                                             uint32_t inDim, uint16_t* __restrict__ means16, int* bad) {
    const uint32_t x = blockIdx.x * 256u + threadIdx.x, j = blockIdx.y, e = blockIdx.z;
    if (x >= words) return;
    const size_t row0 = ((size_t)e * inDim + j) * 8u;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(B) + row0 * pitch + x * 2u;
    uint32_t seen = 0u, dup = 0u;
    for (uint32_t r = 0; r < 8u; r++) {
        const uint32_t w = *reinterpret_cast<const uint16_t*>(base + (size_t)r * pitch);
        const uint32_t bits = 1u << ((w >> 12) & 7u) | 1u << (8u + ((w >> 8) & 7u)) | 1u << (16u + ((w >> 4) & 7u)) | 1u << (24u + (w & 7u));
        dup |= seen & bits;
        seen |= bits;
    }
    if (dup) atomicOr(bad, 1);
    if (x != 0u) return;
    for (uint32_t r = 0; r < 8u; r++) {
        const float m = stats[(row0 + r) * 2u + 1u];
        const __half h = __float2half_rn(m);
        if (!(fabsf(m) <= 65504.0f) || __half2float(h) != m) atomicOr(bad + 1, 1);       // (NaN fails the first test)
        means16[row0 + r] = __half_as_ushort(h);
    }
}

// bad[0], bad[1] (zeroed by the caller): a position named twice; a mean that is no finite f16 number.  means16: u16 per bucket row of the stack.
hipError_t launch_q4_dense_check(const uint16_t* B, uint32_t pitch, uint32_t words, const float* stats, uint32_t inDim, uint32_t numExperts,
                                 uint16_t* means16, int* bad, hipStream_t st) {
    hipLaunchKernelGGL(q4_dense_check_kernel, dim3((words + 255u) / 256u, inDim, numExperts), dim3(256), 0, st, B, pitch, words, stats, inDim, means16, bad);
    return hipGetLastError();
}

// B, means16: ONE expert's buckets (bucket rows `pitch` bytes apart) and compact means; xh, part: launch_dense_gemm_rows's scratch, the
// same sizes; ol: the handle's outlier index (blockPtr null: none, nothing extra is launched)
hipError_t launch_q4_gemm_rows(const uint16_t* B, uint32_t pitch, const uint16_t* means16, const OutlierIndex& ol, const float* x, uint16_t* xh, float* part,
                               float* out, uint32_t inDim, uint32_t outDim, uint32_t rows, hipStream_t st) {
    const uint32_t words = outDim / 32u;
    const bool wide = pitch % 16u == 0 && reinterpret_cast<uintptr_t>(B) % 16u == 0 && words % 8u == 0;
    hipError_t e = pf_block_call(PfCall{x, xh, part, out, inDim, outDim, rows}, st, [&](auto aux, const PfMul& m) {
        return pf_with_either<0, 1>(wide, [&](auto w) {
            return pf_with_tiles(rows, [&](auto nt) {
                auto kernel = &q4_gemm_rows_kernel<decltype(nt)::value, decltype(aux)::value, decltype(w)::value != 0>;
                const hipError_t a = allow_full_lds(reinterpret_cast<const void*>(kernel));
                if (a != hipSuccess) return a;
                hipLaunchKernelGGL(kernel, dim3((words + kQbWords - 1u) / kQbWords, m.sp.splits), dim3(kQbThreads), kQbLds, st, B, pitch, words, means16, xh,
                                   m.dst, inDim, outDim, rows, m.sp.per);
                return hipGetLastError();
            });
        });
    });
    if (e != hipSuccess || !ol.blockPtr) return e;
    hipLaunchKernelGGL(q4_outlier_rows_kernel, dim3((outDim + 63u) / 64u, (rows + 4u * kOlTok - 1u) / (4u * kOlTok)), dim3(256), 0, st, ol, x, out, inDim, outDim,
                       rows);
    return hipGetLastError();
}

}  // namespace effort
