// Prompt prefill straight from the BUCKETED weights: the block multiply of prefill.hip with the A operand un-bucketed on the fly, so a
// model that dropped its f16 cores (the second copy of every matrix) still prefills in one pass per block.
//
//   bucket_gemm_rows          out[r] = U[e] * f16(x[r]) for rows r of a block, U the un-bucketed matrix of expert e (below)
//   bucket_gemm_rows_routed   the same body for a Mixtral block, as dense_gemm_rows_routed_kernel wraps gemm_rows_body
//   bucket_dense_check        decides once per handle whether a bundle IS un-bucketable
//
// U.  At percentLoad 16 the buckets hold the whole matrix: for input j and bucket column c the 16 rank rows (bucket row r * inDim + j,
// r = 0 .. 15) hold the 16 weights of outputs 16 c .. 16 c + 15, each with its output position in its low four mantissa bits
// (convert.hip: (value & 0xFFF0) | pos).  U[16 c + (w & 15)][j] = w for every entry w != 0x0000 -- the position bits stay in the
// value, exactly as bucketMul multiplies them --, +0 where no entry names the element.  Two non-zero entries of one (j, c) with the
// same position (the literal preBucketize path can write them) make the bundle NOT un-bucketable: refused, never guessed.
//
// CONTRACT: the bits are effort_dense_gemm_rows's with U[e] as its matrix.  The k split is pf_split's, the splits are summed by
// reduce_splits_kernel, every accumulator takes its MFMA steps in ascending (stage of 256, chunk of 64, u) order, for step (chunk, u)
// lane group g holds elements 64 chunk + 16 g + 8 u + 0 .. 7 -- gemm_rows_body's operand slots --, f16(x) comes from
// rows_to_f16_kernel, a dead token column and a k past inDim are zero operands, and the steps of a last stage that lie wholly past
// inDim are still taken (on zeros), as the core kernel takes them.
//
// The tiling.  Consecutive k of one output are a bucket-row pitch apart in memory; only the bucket columns are contiguous.  A
// workgroup therefore owns kBkCols = 32 consecutive columns -- 64 contiguous bytes of each bucket row, 512 outputs -- and one k split.
// Per chunk of 64 k it loads the 16 ranks' 64 pieces (64 KB), scatters every 16-bit entry into an LDS tile [512 outputs][64 k] at row
// 16 c + (w & 15) (2-byte LDS stores; the tile is zero-filled first, 0x0000 entries are never stored; pitch 144 bytes: 16-byte reads
// of 16 consecutive rows fall on different banks), and its 8 waves -- four 16-row tiles each -- read their A fragments back as
// 16-byte LDS reads in the slot order above.  f16(x) of the chunk is staged beside it, as the core kernel stages it.  The later
// chunks' global loads are asked for before the current chunk's products and land under them (two chunks ahead with 16-byte loads).
// The row pieces are 16-byte loads where every piece is one (pitch % 16 == 0, the buckets 16-byte aligned, columns % 8 == 0) and
// 4-byte loads otherwise (pitches are multiples of 4 bytes; an even column count makes a dword two entries of the payload): no byte
// of a row outside its 2 * columns payload is read, whatever the padding holds.
// 32 columns is the narrowest piece that still reads half a 128-byte line of every row; it gives outDim / 512 workgroups per split
// (8 x 4 splits for 4096 x 4096), which is why this kernel does not load the chip the way the core kernel's 64-row groups do.
#include "prefill.h"

namespace effort {

constexpr uint32_t kBkCols = 32;                    // bucket columns a workgroup owns
constexpr uint32_t kBkRows = 16u * kBkCols;         // ... the outputs they hold
constexpr uint32_t kBkWaves = 8, kBkThreads = 64u * kBkWaves;
constexpr uint32_t kBkTiles = kBkRows / 16u / kBkWaves;   // 16-row MFMA tiles per wave
constexpr uint32_t kBkK = 64;                       // k per LDS stage: one chunk of the core kernel's stage
constexpr uint32_t kBkPitch = kBkK * 2u + 16u;      // bytes per tile row (and per staged token row)
constexpr uint32_t kBkTileBytes = kBkRows * kBkPitch;
constexpr uint32_t kBkLds = kBkTileBytes + 64u * kBkPitch;      // the A tile, then up to 64 token rows
static_assert(kPfStage % kBkK == 0 && kBkTileBytes % (16u * kBkThreads) == 0, "whole chunks per stage; the fill is whole 16-byte stores");

// The block multiply's body.  NT = token tiles (of 16), AUX = cache policy of the bucket loads (0, or 2 = nt), VEC = dwords per load of
// a row piece (4 or 1), ROUTED as gemm_rows_body: column t is assignment col[t], reads row col[t] >> xShift of xh, writes row col[t].
// B = this expert's buckets (bucket row r * inDim + j at byte (r * inDim + j) * pitch), cols = its bucket columns.
template <int NT, int AUX, int VEC, bool ROUTED>
__device__ __forceinline__ void bucket_rows_body(unsigned char* __restrict__ lds, const uint16_t* __restrict__ B, uint32_t pitch, uint32_t cols,
                                                 const uint16_t* __restrict__ xh, float* __restrict__ o, uint32_t inDim, uint32_t outDim, uint32_t live,
                                                 uint32_t xRows, uint32_t per, const uint32_t* col, uint32_t xShift) {
    constexpr uint32_t kPiecesPerRow = kBkCols * 2u / (4u * VEC);                       // loads per bucket row piece of 64 bytes
    constexpr int kLoads = (int)(16u * kBkK * kPiecesPerRow / kBkThreads);              // per thread and chunk: 8 (VEC 4) or 32 (VEC 1)
    constexpr uint32_t kXPieces = NT * 16u * (kBkK / 8u);                               // 16-byte pieces of the staged token rows
    constexpr int kXLoads = (int)((kXPieces + kBkThreads - 1u) / kBkThreads);
    unsigned char* const tile = lds;
    unsigned char* const xs = lds + kBkTileBytes;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t g = lane >> 4, r16 = lane & 15u, c0 = blockIdx.x * kBkCols;
    // the descriptor ends with the payload of the expert's last bucket row
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(B), 0, (int)((16u * inDim - 1u) * pitch + cols * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(xh), 0, (int)(xRows * inDim * 2u), 0x00020000);
    const uint32_t chunks = (inDim + kPfStage - 1u) / kPfStage * (kPfStage / kBkK);    // every chunk of every stage, the dead ones of the last stage too
    const uint32_t q0 = blockIdx.y * per * (kPfStage / kBkK), q1 = min(q0 + per * (kPfStage / kBkK), chunks);

    // kDepth chunks of loads are in flight: two where the pieces are 16-byte loads (a chunk's 64 KB then arrive under the scatter and the
    // products of the chunk before it; measured 4096 x 4096 at 64 rows: 107.9 us with one chunk in flight), one where they are 4-byte
    // loads (32 registers a chunk: a second set does not fit in 256) and in the routed kernel (its four bodies share one register file:
    // with a second set the compiler spilled 596 bytes a lane)
    constexpr int kDepth = VEC == 4 && !ROUTED ? 2 : 1;
    uint32_t heldA[kDepth][kLoads][VEC];
    uint4 heldX[kDepth][kXLoads];
    // load i of thread tid: piece p of bucket row (rank, jj) of the chunk
    auto ask_a = [&](uint32_t q, uint32_t (&nextA)[kLoads][VEC]) {
#pragma unroll
        for (int i = 0; i < kLoads; i++) {
            const uint32_t idx = tid + (uint32_t)i * kBkThreads, brow = idx / kPiecesPerRow, p = idx % kPiecesPerRow;
            const uint32_t rank = brow / kBkK, j = q * kBkK + brow % kBkK, cFirst = c0 + p * 2u * VEC;
#pragma unroll
            for (int v = 0; v < VEC; v++) nextA[i][v] = 0u;
            if (j < inDim && cFirst + 2u * VEC <= cols) {                                // (cols is a multiple of 2 VEC: a piece is inside the payload or outside)
                const uint32_t off = (rank * inDim + j) * pitch + cFirst * 2u;
                if constexpr (VEC == 4) {
                    const auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, AUX);
                    nextA[i][0] = w[0]; nextA[i][1] = w[1]; nextA[i][2] = w[2]; nextA[i][3] = w[3];
                } else {
                    nextA[i][0] = __builtin_amdgcn_raw_buffer_load_b32(rs, off, 0, AUX);
                }
            }
        }
    };
    auto x_row = [&](uint32_t tok) -> uint32_t {
        if constexpr (ROUTED) return tok < live ? col[tok] >> xShift : 0u;
        else return min(tok, live - 1u);
    };
    auto ask_x = [&](uint32_t q, uint4 (&nextX)[kXLoads]) {
#pragma unroll
        for (int i = 0; i < kXLoads; i++) {
            const uint32_t idx = tid + (uint32_t)i * kBkThreads, tok = idx / (kBkK / 8u), e = q * kBkK + (idx % (kBkK / 8u)) * 8u;
            nextX[i] = make_uint4(0u, 0u, 0u, 0u);
            if (idx < kXPieces && tok < live && e < inDim) {                             // a dead column, a k past inDim: zeros are staged (inDim % 8 == 0)
                const auto x = __builtin_amdgcn_raw_buffer_load_b128(xr, x_row(tok) * inDim * 2u + e * 2u, 0, 0);
                nextX[i] = make_uint4(x[0], x[1], x[2], x[3]);
            }
        }
    };
    auto scatter = [&](const uint32_t (&nextA)[kLoads][VEC], const uint4 (&nextX)[kXLoads]) {
#pragma unroll
        for (int i = 0; i < kLoads; i++) {
            const uint32_t idx = tid + (uint32_t)i * kBkThreads, brow = idx / kPiecesPerRow, p = idx % kPiecesPerRow;
            const uint32_t jj = brow % kBkK, cLocal = p * 2u * VEC;
#pragma unroll
            for (int v = 0; v < VEC; v++)
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const uint32_t w = (nextA[i][v] >> (16 * h)) & 0xFFFFu;
                    const uint32_t row = (cLocal + 2u * v + h) * 16u + (w & 15u);       // < kBkRows
                    if (w != 0u) *reinterpret_cast<uint16_t*>(tile + row * kBkPitch + jj * 2u) = (uint16_t)w;
                }
        }
#pragma unroll
        for (int i = 0; i < kXLoads; i++) {
            const uint32_t idx = tid + (uint32_t)i * kBkThreads;
            if (idx < kXPieces) *reinterpret_cast<uint4*>(xs + (idx / (kBkK / 8u)) * kBkPitch + (idx % (kBkK / 8u)) * 16u) = nextX[i];
        }
    };

    pf_f32x4 acc[kBkTiles][NT];
#pragma unroll
    for (int m = 0; m < (int)kBkTiles; m++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[m][t] = pf_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // one chunk: fill, scatter what `slot` holds, ask for chunk q + kDepth into the freed slot, multiply
    auto chunk = [&](uint32_t q, auto slotTag) {
        constexpr int slot = decltype(slotTag)::value;
#pragma unroll
        for (int i = 0; i < (int)(kBkTileBytes / (16u * kBkThreads)); i++)              // +0 wherever no entry lands
            *reinterpret_cast<uint4*>(tile + (tid + (uint32_t)i * kBkThreads) * 16u) = make_uint4(0u, 0u, 0u, 0u);
        __syncthreads();
        scatter(heldA[slot], heldX[slot]);
        __syncthreads();
        if (q + kDepth < q1) { ask_a(q + kDepth, heldA[slot]); ask_x(q + kDepth, heldX[slot]); }   // the later chunks' loads run under this chunk's products
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 2; u++) {
            pf_half8 bf[NT];
#pragma unroll
            for (int t = 0; t < NT; t++) bf[t] = *reinterpret_cast<const pf_half8*>(xs + (t * 16u + r16) * kBkPitch + (g * 2u + u) * 16u);
#pragma unroll
            for (int m = 0; m < (int)kBkTiles; m++) {
                const pf_half8 af = *reinterpret_cast<const pf_half8*>(tile + ((wave * kBkTiles + m) * 16u + r16) * kBkPitch + (g * 2u + u) * 16u);
#pragma unroll
                for (int t = 0; t < NT; t++) acc[m][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf[t], acc[m][t], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();                                                                 // the tile and the token rows are rewritten by the next chunk
    };
    ask_a(q0, heldA[0]);
    ask_x(q0, heldX[0]);
    if constexpr (kDepth == 2) {
        if (q0 + 1u < q1) { ask_a(q0 + 1u, heldA[1]); ask_x(q0 + 1u, heldX[1]); }
        for (uint32_t q = q0; q < q1; q += 2u) {                                         // (uniform; the slots alternate with static indices: registers)
            chunk(q, std::integral_constant<int, 0>{});
            if (q + 1u < q1) chunk(q + 1u, std::integral_constant<int, 1>{});
        }
    } else {
        for (uint32_t q = q0; q < q1; q++) chunk(q, std::integral_constant<int, 0>{});   // (uniform)
    }
    // Accumulator register i of lane l is tile row 4 * (l >> 4) + i, token l & 15.
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t tok = t * 16u + r16;
        uint32_t orow = tok;
        if constexpr (ROUTED) orow = tok < live ? col[tok] : 0u;
#pragma unroll
        for (int m = 0; m < (int)kBkTiles; m++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t row = c0 * 16u + (wave * kBkTiles + m) * 16u + g * 4u + i;
                if (tok < live && row < outDim) o[(size_t)orow * outDim + row] = acc[m][t][i];
            }
    }
}

// grid = (groups of kBkCols columns, splits).  dst = out when there is one split, else the partial sums [splits][rows][outDim].
template <int NT, int AUX, int VEC>
__global__ __launch_bounds__(kBkThreads) void bucket_gemm_rows_kernel(const uint16_t* __restrict__ B, uint32_t pitch, uint32_t cols,
                                                                      const uint16_t* __restrict__ xh, float* __restrict__ dst, uint32_t inDim,
                                                                      uint32_t outDim, uint32_t rows, uint32_t per) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bk_lds[];
    bucket_rows_body<NT, AUX, VEC, false>(bk_lds, B, pitch, cols, xh, dst + (size_t)blockIdx.y * rows * outDim, inDim, outDim, rows, rows, per, nullptr, 0u);
}

// grid = (groups of columns, splits, experts): dense_gemm_rows_routed_kernel's walk -- an expert nobody picked leaves at once, none of its
// buckets asked for; otherwise its columns 64 at a time, each walk through the body at ITS tile count.  Expert e's bucket rows start
// at row 16 * inDim * e (a 64-bit add: the descriptor covers one expert).
template <int AUX, int VEC>
__global__ __launch_bounds__(kBkThreads) void bucket_gemm_rows_routed_kernel(const uint16_t* __restrict__ B, uint32_t pitch, uint32_t cols,
                                                                             const uint16_t* __restrict__ xh, float* __restrict__ dst,
                                                                             const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ list,
                                                                             uint32_t inDim, uint32_t outDim, uint32_t assigns, uint32_t xRows,
                                                                             uint32_t xShift, uint32_t per) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bk_lds[];
    __shared__ uint32_t col[64];
    const uint32_t e = blockIdx.z, n = __builtin_amdgcn_readfirstlane(min(cnt[e], kPfMaxAssign));
    if (n == 0u) return;
    const uint16_t* Be = reinterpret_cast<const uint16_t*>(reinterpret_cast<const unsigned char*>(B) + (size_t)e * 16u * inDim * pitch);
    float* o = dst + (size_t)blockIdx.y * assigns * outDim;
    for (uint32_t a0 = 0; a0 < n; a0 += 64u) {                                           // (uniform)
        const uint32_t live = min(n - a0, 64u);
        if (threadIdx.x < live) col[threadIdx.x] = min(list[e * kPfMaxAssign + a0 + threadIdx.x], assigns - 1u);
        __syncthreads();
        switch ((live + 15u) / 16u) {
            case 1: bucket_rows_body<1, AUX, VEC, true>(bk_lds, Be, pitch, cols, xh, o, inDim, outDim, live, xRows, per, col, xShift); break;
            case 2: bucket_rows_body<2, AUX, VEC, true>(bk_lds, Be, pitch, cols, xh, o, inDim, outDim, live, xRows, per, col, xShift); break;
            case 3: bucket_rows_body<3, AUX, VEC, true>(bk_lds, Be, pitch, cols, xh, o, inDim, outDim, live, xRows, per, col, xShift); break;
            default: bucket_rows_body<4, AUX, VEC, true>(bk_lds, Be, pitch, cols, xh, o, inDim, outDim, live, xRows, per, col, xShift); break;
        }
        __syncthreads();                                                                 // col and the LDS are rewritten by the next walk
    }
}

// Is the bundle un-bucketable?  One thread per (bucket column pair, input, expert) reads its 16 ranks' dword and marks the positions
// of the non-zero entries; a position named twice raises *bad.  Only payload bytes are read.
__global__ __launch_bounds__(256) void bucket_dense_check_kernel(const uint16_t* __restrict__ B, uint32_t pitch, uint32_t cols, uint32_t inDim, int* bad) {
    const uint32_t cp = blockIdx.x * 256u + threadIdx.x, j = blockIdx.y, e = blockIdx.z;
    if (cp >= cols / 2u) return;
    const unsigned char* base = reinterpret_cast<const unsigned char*>(B) + ((size_t)e * 16u * inDim + j) * pitch + cp * 4u;
    uint32_t seen0 = 0u, seen1 = 0u, dup = 0u;
    for (uint32_t r = 0; r < 16u; r++) {
        const uint32_t w = *reinterpret_cast<const uint32_t*>(base + (size_t)r * inDim * pitch), w0 = w & 0xFFFFu, w1 = w >> 16;
        const uint32_t b0 = w0 ? 1u << (w0 & 15u) : 0u, b1 = w1 ? 1u << (w1 & 15u) : 0u;
        dup |= (seen0 & b0) | (seen1 & b1);
        seen0 |= b0; seen1 |= b1;
    }
    if (dup) atomicOr(bad, 1);
}

bool bucket_gemm_rows_supported(uint32_t inDim, uint32_t outDim) {
    return dense_gemm_rows_supported(inDim, outDim) && outDim % 32u == 0 && outDim <= 16384u;
}

// *bad (zeroed by the caller) becomes non-zero when two entries of one (expert, input, column) name the same position
hipError_t launch_bucket_dense_check(const uint16_t* B, uint32_t pitch, uint32_t cols, uint32_t inDim, uint32_t numExperts, int* bad, hipStream_t st) {
    hipLaunchKernelGGL(bucket_dense_check_kernel, dim3((cols / 2u + 255u) / 256u, inDim, numExperts), dim3(256), 0, st, B, pitch, cols, inDim, bad);
    return hipGetLastError();
}

// 16-byte row pieces (VEC 4) where every piece is one, 4-byte pieces (VEC 1) otherwise.  (Every expert's base is a multiple of
// 16 * inDim * pitch bytes behind B: 16-byte aligned with B when the pitch is.)
static bool bucket_wide(const uint16_t* B, uint32_t pitch, uint32_t cols) {
    return pitch % 16u == 0 && reinterpret_cast<uintptr_t>(B) % 16u == 0 && cols % 8u == 0;
}

// ---- the two launchers: pf_block_call (prefill.h) around the bucket kernels
// kernel<...> on `grid` with the bucket kernels' block and all of the LDS
template <class K, class... Args>
static hipError_t launch_bk(K kernel, dim3 grid, hipStream_t st, Args... args) {
    const hipError_t e = allow_full_lds(reinterpret_cast<const void*>(kernel));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kernel, grid, dim3(kBkThreads), kBkLds, st, args...);
    return hipGetLastError();
}

// B: ONE expert's buckets (percentLoad 16), bucket rows `pitch` bytes apart; xh, part: launch_dense_gemm_rows's scratch, the same sizes
hipError_t launch_bucket_gemm_rows(const uint16_t* B, uint32_t pitch, const float* x, uint16_t* xh, float* part, float* out, uint32_t inDim,
                                   uint32_t outDim, uint32_t rows, hipStream_t st) {
    const uint32_t cols = outDim / 16u;
    return pf_block_call(PfCall{x, xh, part, out, inDim, outDim, rows}, st, [&](auto aux, const PfMul& m) {
        return pf_with_either<1, 4>(bucket_wide(B, pitch, cols), [&](auto vec) {
            return pf_with_tiles(rows, [&](auto nt) {
                return launch_bk(&bucket_gemm_rows_kernel<decltype(nt)::value, decltype(aux)::value, decltype(vec)::value>,
                                 dim3((cols + kBkCols - 1u) / kBkCols, m.sp.splits), st, B, pitch, cols, xh, m.dst, inDim, outDim, rows, m.sp.per);
            });
        });
    });
}
// B: the whole stack's buckets; xh, part, groups: launch_dense_gemm_rows_routed's scratch, the same sizes.  out f32 [rows][2][outDim].
hipError_t launch_bucket_gemm_rows_routed(const uint16_t* B, uint32_t pitch, uint32_t numExperts, const uint32_t* idx2, const float* x, uint32_t xPerSlot,
                                          uint16_t* xh, float* part, uint32_t* groups, float* out, uint32_t inDim, uint32_t outDim, uint32_t rows,
                                          hipStream_t st) {
    const uint32_t cols = outDim / 16u;
    return pf_block_call(PfCall{x, xh, part, out, inDim, outDim, rows, true, idx2, groups, numExperts, xPerSlot}, st, [&](auto aux, const PfMul& m) {
        return pf_with_either<1, 4>(bucket_wide(B, pitch, cols), [&](auto vec) {
            return launch_bk(&bucket_gemm_rows_routed_kernel<decltype(aux)::value, decltype(vec)::value>, dim3((cols + kBkCols - 1u) / kBkCols, m.sp.splits, numExperts),
                             st, B, pitch, cols, xh, m.dst, m.cnt, m.list, inDim, outDim, m.assigns, m.xRows, m.xShift, m.sp.per);
        });
    });
}

}  // namespace effort
