// Prompt prefill: the dense path for a BLOCK of tokens (up to kPrefillMaxRows = EFFORT_PREFILL_MAX_ROWS), beside the token step.
// A GEMV-per-token loop streams every weight from HBM once per prompt token; the tokens of a prompt are independent inside a
// layer's multiplies, so a block of them can share one pass over each matrix.
//
//   dense_gemm_rows   out[r] = W * f16(x[r]) for rows r of a block: basicMul's arithmetic (helpers/mps.swift:14-47: x rounded to f16
//                     once, exact f16 products, f32 sums) on v_mfma_f32_16x16x32_f16.  An MFMA tile is 16 rows of W (A operand) by 16
//                     tokens (B operand); up to four token tiles share every weight fragment.
//   dense_gemm_rows_routed   the same body for a Mixtral block: assignment 2 r + s (token r, slot s of its top-2) multiplies the expert
//                     it picked.  The assignments are grouped by expert on the device; an expert's workgroups stream its matrix once
//                     for all its token columns, an expert nobody picked is not read.  Per assignment the plain kernel's bits.
//
// The block multiply.  The weight stream is what it is bound by, and a lane's A fragment is 16 contiguous bytes of a weight row, so
// weights go from global memory straight into the MFMA operand -- no LDS.  K is walked in stages of kPfStage = 256 elements; inside
// each 64-element chunk (one 128-byte line of each row) lane group g = lane >> 4 takes elements 16g .. 16g+15 as the fragments of
// TWO MFMA steps (u = 0, 1: elements 16g + 8u + j), so the four lanes of a row cover a whole line with two 16-byte loads each.  The
// B operand takes the same permutation: 16 contiguous bytes of f16(x[token]).
// f16(x) is written ONCE per call by rows_to_f16_kernel into context scratch (64 x 14336 halves are 1.8 MB: no LDS holds that).  A
// workgroup is kPfWaves = 4 waves on four consecutive 16-row tiles (64 rows of W) and the SAME k range: a stage of f16(x) (up to 64
// tokens x 256 elements, 32 KB) is staged in LDS once per workgroup -- double-buffered, the next stage's token pieces and the next
// stage's weight fragments (8 loads per lane) asked for before the current stage is multiplied -- and read by all four waves.
// 64 rows per workgroup are too few workgroups for the chip (64 for 4096 rows), so K is also split over blockIdx.y into `splits`
// ranges of whole stages; with more than one split every range writes its partial sums to context scratch and reduce_splits_kernel
// adds them.
// Measured at 64 rows, us per call on 4096 x 4096 / 4096 -> 14336 (profiles/r09_prefill.json; the GEMV: 8.1 / 21.0): this tiling
// 19.7 / 50.1; eight waves on 128 rows with 128-element stages 22.6 / 58.6; the first version -- a workgroup of 16 rows whose eight
// waves split K, every wave reading its token fragments from L2 (128 MB of L2 reads beside a 32 MB matrix) -- 25.7 / 83.4.
//
// The order of the sums does not depend on the number of rows: `splits` and the stages of a split follow from (inDim, outDim) alone;
// element (row, token) is the sum over the splits s = 0, 1, ..., in that order, of an accumulator that took its split's MFMA steps in
// ascending stage, chunk, u order.  A token column that is not live is a zero operand (zeros are staged for it: no x row at or
// beyond `rows` is read, nor the scratch's stale halves); a k step past inDim multiplies zeros.  So a row's bits are the same for
// every `rows` and every position in the block.
#include "prefill.h"

namespace effort {

// (kPrefillMaxRows, kPfStage, kPfKeepBytes and the k split are prefill.h's: the bucket kernel of prefill_buckets.hip shares them)
constexpr int kPfWaves = 4;               // waves per workgroup: one 16-row tile of W each
constexpr int kPfChunks = kPfStage / 64;  // 64-element chunks (128-byte lines of a row) per stage
constexpr uint32_t kPfQ = kPfStage / 8;   // 16-byte pieces of a token row per stage
constexpr uint32_t kPfPitch = kPfStage / 8 + 1;   // uint4 per staged token row: 256 bytes + 16 of padding (a 256-byte pitch puts every token on the same banks)
constexpr uint32_t kPfMaxSplits = 16, kPfTargetGroups = 256;

// x.asFloat16() (mps.swift:19) of the live rows, once per call
__global__ void rows_to_f16_kernel(const float* __restrict__ x, uint16_t* __restrict__ xh, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) xh[i] = __half_as_ushort(__float2half_rn(x[i]));
}

// out[i] = part[0][i] + part[1][i] + ... in that order
__global__ void reduce_splits_kernel(const float* __restrict__ part, float* __restrict__ out, uint32_t n, uint32_t splits) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (uint32_t k = 1; k < splits; k++) s += part[(size_t)k * n + i];
    out[i] = s;
}

// The k split of a shape: stages per split and the number of splits (a function of the shape alone -- never of rows).
PfSplit pf_split(uint32_t inDim, uint32_t outDim) {
    const uint32_t stages = (inDim + kPfStage - 1u) / kPfStage, groups = (outDim + 16u * kPfWaves - 1u) / (16u * kPfWaves);
    uint32_t want = (kPfTargetGroups + groups - 1u) / groups;
    if (want > kPfMaxSplits) want = kPfMaxSplits;
    if (want > stages) want = stages;
    const uint32_t per = (stages + want - 1u) / want;
    return PfSplit{per, (stages + per - 1u) / per};
}

// The block multiply's body, shared by the plain and the routed front end.  NT = token tiles (of 16) of the columns it serves; AUX =
// cache policy of the weight loads (0, or 2 = nt); `cols` columns are live.  xs is the workgroup's LDS, [2][NT * 16][kPfPitch] pieces.
// Plain (ROUTED = false): column t is row t of xh and of dst.  Routed: column t is assignment a = col[t] (LDS, `cols` entries): it reads
// row a >> xShift of xh and writes row a of dst -- nothing else differs, so a column's sums run in the plain kernel's order.
// xh has xRows rows; dst = out when there is one split, else this split's slab of the partial sums.
template <int NT, int AUX, bool ROUTED>
__device__ __forceinline__ void gemm_rows_body(uint4* __restrict__ xs, const uint16_t* __restrict__ W, const uint16_t* __restrict__ xh,
                                               float* __restrict__ o, uint32_t inDim, uint32_t outDim, uint32_t cols, uint32_t xRows, uint32_t per,
                                               const uint32_t* col, uint32_t xShift) {
    auto slot = [&](uint32_t buf, uint32_t tok, uint32_t q) -> uint4& { return xs[(buf * (NT * 16u) + tok) * kPfPitch + q]; };
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t g = lane >> 4, r16 = lane & 15u, row0 = (blockIdx.x * kPfWaves + wave) * 16u;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(W), 0, (int)min((size_t)0xFFFFFFFFu, (size_t)outDim * inDim * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(xh), 0, (int)(xRows * inDim * 2u), 0x00020000);
    const uint32_t aOff = min(row0 + r16, outDim - 1u) * inDim * 2u;           // a row past the end re-reads the last one (W < 4 GiB)
    const uint32_t stages = (inDim + kPfStage - 1u) / kPfStage;
    const uint32_t s0 = blockIdx.y * per, s1 = min(s0 + per, stages);           // (the host made every split non-empty)
    // staging: thread `tid` moves 16-byte piece q = idx % kPfQ of token idx / kPfQ, idx = tid + 64 kPfWaves i
    constexpr int kPieces = (NT * 16 * kPfQ + 64 * kPfWaves - 1) / (64 * kPfWaves);
    uint4 nextB[kPieces], curA[kPfChunks][2], nextA[kPfChunks][2];
    auto x_row = [&](uint32_t tok) -> uint32_t {                                 // the row of xh a column reads (a dead column: any row, masked in put_b)
        if constexpr (ROUTED) return tok < cols ? col[tok] >> xShift : 0u;
        else return min(tok, cols - 1u);
    };
    auto ask_b = [&](uint32_t s) {
#pragma unroll
        for (int i = 0; i < kPieces; i++) {
            const uint32_t idx = tid + i * 64u * kPfWaves, tok = idx / kPfQ, e = s * kPfStage + (idx % kPfQ) * 8u;
            const auto x = __builtin_amdgcn_raw_buffer_load_b128(xr, x_row(tok) * inDim * 2u + min(e, inDim - 8u) * 2u, 0, 0);    // clamped: masked in put_b
            nextB[i] = make_uint4(x[0], x[1], x[2], x[3]);
        }
    };
    auto put_b = [&](uint32_t s, uint32_t buf) {       // (the masks are applied HERE, not beside the loads: a use right behind a load makes it wait)
#pragma unroll
        for (int i = 0; i < kPieces; i++) {
            const uint32_t idx = tid + i * 64u * kPfWaves, tok = idx / kPfQ, e = s * kPfStage + (idx % kPfQ) * 8u;
            const uint32_t m = (tok < cols && e < inDim) ? 0xFFFFFFFFu : 0u;    // a dead column, a k past inDim: zeros are staged
            if (idx < NT * 16u * kPfQ) slot(buf, tok, idx % kPfQ) = make_uint4(nextB[i].x & m, nextB[i].y & m, nextB[i].z & m, nextB[i].w & m);
        }
    };
    auto ask_a = [&](uint32_t s, uint4 (&a)[kPfChunks][2]) {
#pragma unroll
        for (int c = 0; c < kPfChunks; c++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const uint32_t e = s * kPfStage + c * 64u + g * 16u + u * 8u;
                const auto w = __builtin_amdgcn_raw_buffer_load_b128(rs, aOff + min(e, inDim - 8u) * 2u, 0, AUX);   // clamped, branch-free (inDim % 32 == 0)
                a[c][u] = make_uint4(w[0], w[1], w[2], w[3]);
            }
    };
    pf_f32x4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) acc[t] = pf_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    ask_a(s0, curA);
    ask_b(s0);
    put_b(s0, 0);
    __syncthreads();
    for (uint32_t s = s0; s < s1; s++) {                                          // (uniform)
        const uint32_t buf = (s - s0) & 1u;
        const bool more = s + 1u < s1;
        if (more) { ask_a(s + 1u, nextA); ask_b(s + 1u); }                        // the next stage's loads run under this stage's products
        __builtin_amdgcn_sched_barrier(0);             // (left to itself the scheduler sinks the loads to their first use)
#pragma unroll
        for (int c = 0; c < kPfChunks; c++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const uint32_t m = s * kPfStage + c * 64u + g * 16u + u * 8u < inDim ? 0xFFFFFFFFu : 0u;    // a clamped lane holds a copy of other data: a zero operand
                const pf_half8 af = __builtin_bit_cast(pf_half8, make_uint4(curA[c][u].x & m, curA[c][u].y & m, curA[c][u].z & m, curA[c][u].w & m));
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const pf_half8 bf = __builtin_bit_cast(pf_half8, slot(buf, t * 16 + r16, c * 8 + g * 2 + u));
                    acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, bf, acc[t], 0, 0, 0);
                }
            }
        __builtin_amdgcn_sched_barrier(0);
        if (more) {
            put_b(s + 1u, buf ^ 1u);                        // (read last in the stage before this one: every wave passed that stage's barrier)
#pragma unroll
            for (int c = 0; c < kPfChunks; c++)
#pragma unroll
                for (int u = 0; u < 2; u++) curA[c][u] = nextA[c][u];
        }
        __syncthreads();
    }
    // Accumulator register i of lane l is W row 4 * (l >> 4) + i, token l & 15.
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t tok = t * 16u + r16;
        uint32_t orow = tok;
        if constexpr (ROUTED) orow = tok < cols ? col[tok] : 0u;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t row = row0 + g * 4u + i;
            if (tok < cols && row < outDim) o[(size_t)orow * outDim + row] = acc[t][i];
        }
    }
}

// grid = (groups of 16 * kPfWaves = 64 rows, splits).  dst = out when there is one split, else the partial sums [splits][rows][outDim].
template <int NT, int AUX>
__global__ __launch_bounds__(64 * kPfWaves, 2) void dense_gemm_rows_kernel(const uint16_t* __restrict__ W, const uint16_t* __restrict__ xh,
                                                                           float* __restrict__ dst, uint32_t inDim, uint32_t outDim, uint32_t rows,
                                                                           uint32_t per) {
    __shared__ uint4 xs[2 * NT * 16 * kPfPitch];
    gemm_rows_body<NT, AUX, false>(xs, W, xh, dst + (size_t)blockIdx.y * rows * outDim, inDim, outDim, rows, rows, per, nullptr, 0u);
}

// ---- the routed front end: every assignment a = 2 r + s (token r, slot s) of a Mixtral block multiplies the expert it picked.
// Assignments are grouped by expert ON THE DEVICE (the expert numbers never reach the host), in assignment order: cnt[e] and
// list[e][0 .. cnt[e]).  kPfMaxAssign = 2 * kPrefillMaxRows entries per expert (prefill.h).

// The prologue of a routed call, ONE launch: blocks 0 .. gridDim.x - 2 write f16(x) (rows_to_f16_kernel's element each), the last block
// groups.  Thread e of it walks the 2 * rows clamped expert numbers (LDS) in ascending a: deterministic, no atomics.
// No idx2 entry at or past 2 * rows is read.
__global__ __launch_bounds__(256) void routed_prologue_kernel(const float* __restrict__ x, uint16_t* __restrict__ xh, uint32_t n,
                                                              const uint32_t* __restrict__ idx2, uint32_t assigns, uint32_t numExperts,
                                                              uint32_t* __restrict__ cnt, uint32_t* __restrict__ list) {
    if (blockIdx.x + 1u < gridDim.x) {
        const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
        if (i < n) xh[i] = __half_as_ushort(__float2half_rn(x[i]));
        return;
    }
    __shared__ uint32_t ex[kPfMaxAssign];
    if (threadIdx.x < assigns) ex[threadIdx.x] = min(idx2[threadIdx.x], numExperts - 1u);      // effort_dense_gemv_expert's clamp
    __syncthreads();
    if (threadIdx.x >= numExperts) return;
    uint32_t k = 0;
    for (uint32_t a = 0; a < assigns; a++)
        if (ex[a] == threadIdx.x) list[threadIdx.x * kPfMaxAssign + k++] = a;
    cnt[threadIdx.x] = k;
}

// grid = (groups of 64 rows, splits, experts).  An expert nobody picked leaves at once: none of its weights is asked for.  Otherwise its
// columns are walked 64 at a time (a real routing gives an expert at most 64; 65 .. 128 come from duplicates or clamping alone), each walk
// through the body at ITS tile count -- the count is a device value, so the switch over NT sits here, uniform per workgroup, and an
// expert with 9 columns runs the one-tile code the plain kernel runs for 9 rows.  dst rows are assignments: [splits][assigns][outDim].
template <int AUX>
__global__ __launch_bounds__(64 * kPfWaves, 2) void dense_gemm_rows_routed_kernel(const uint16_t* __restrict__ W, const uint16_t* __restrict__ xh,
                                                                                  float* __restrict__ dst, const uint32_t* __restrict__ cnt,
                                                                                  const uint32_t* __restrict__ list, uint32_t inDim, uint32_t outDim,
                                                                                  uint32_t assigns, uint32_t xRows, uint32_t xShift, uint32_t per) {
    __shared__ uint4 xs[2 * 4 * 16 * kPfPitch];
    __shared__ uint32_t col[64];
    const uint32_t e = blockIdx.z, n = __builtin_amdgcn_readfirstlane(min(cnt[e], kPfMaxAssign));
    if (n == 0u) return;
    const uint16_t* We = W + (size_t)e * outDim * inDim;                          // a 64-bit add: only ONE expert's matrix is under the descriptor's 4 GiB
    float* o = dst + (size_t)blockIdx.y * assigns * outDim;
    for (uint32_t c0 = 0; c0 < n; c0 += 64u) {                                     // (uniform)
        const uint32_t cols = min(n - c0, 64u);
        if (threadIdx.x < cols) col[threadIdx.x] = min(list[e * kPfMaxAssign + c0 + threadIdx.x], assigns - 1u);
        __syncthreads();
        switch ((cols + 15u) / 16u) {
            case 1: gemm_rows_body<1, AUX, true>(xs, We, xh, o, inDim, outDim, cols, xRows, per, col, xShift); break;
            case 2: gemm_rows_body<2, AUX, true>(xs, We, xh, o, inDim, outDim, cols, xRows, per, col, xShift); break;
            case 3: gemm_rows_body<3, AUX, true>(xs, We, xh, o, inDim, outDim, cols, xRows, per, col, xShift); break;
            default: gemm_rows_body<4, AUX, true>(xs, We, xh, o, inDim, outDim, cols, xRows, per, col, xShift); break;
        }
        __syncthreads();                                                           // col and xs are rewritten by the next walk
    }
}

bool dense_gemm_rows_supported(uint32_t inDim, uint32_t outDim) {
    return inDim % 32u == 0 && inDim >= 32u && inDim <= 65536u && outDim >= 1u && outDim <= (1u << 24) && (size_t)outDim * inDim * 2u <= 0xFFFFFFFFull;
}
// floats of context scratch the partial sums of a call need (0: one split, the kernel writes out itself)
size_t dense_gemm_rows_partial_floats(uint32_t inDim, uint32_t outDim, uint32_t rows) {
    const PfSplit sp = pf_split(inDim, outDim);
    return sp.splits > 1u ? (size_t)sp.splits * rows * outDim : 0;
}

// floats of context scratch the partial sums of a routed call need: 2 * rows assignment rows per split
size_t dense_gemm_rows_routed_partial_floats(uint32_t inDim, uint32_t outDim, uint32_t rows) {
    return dense_gemm_rows_partial_floats(inDim, outDim, 2u * rows);
}
size_t dense_gemm_rows_routed_group_words() { return (size_t)kPfMaxExperts * (1u + kPfMaxAssign); }

// ---- the launches around the multiply (prefill.h), shared with prefill_buckets.hip
hipError_t launch_rows_to_f16(const float* x, uint16_t* xh, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(rows_to_f16_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, x, xh, n);
    return hipGetLastError();
}
hipError_t launch_reduce_splits(const float* part, float* out, uint32_t n, uint32_t splits, hipStream_t st) {
    hipLaunchKernelGGL(reduce_splits_kernel, dim3((n + 255u) / 256u), dim3(256), 0, st, part, out, n, splits);
    return hipGetLastError();
}
hipError_t launch_routed_prologue(const float* x, uint16_t* xh, uint32_t n, const uint32_t* idx2, uint32_t assigns, uint32_t numExperts, uint32_t* cnt,
                                  uint32_t* list, hipStream_t st) {
    hipLaunchKernelGGL(routed_prologue_kernel, dim3((n + 255u) / 256u + 1u), dim3(256), 0, st, x, xh, n, idx2, assigns, numExperts, cnt, list);
    return hipGetLastError();
}

// ---- the two launchers: pf_block_call (prefill.h) around the core kernels
// xh: scratch of rows * inDim halves; part: scratch of dense_gemm_rows_partial_floats floats
hipError_t launch_dense_gemm_rows(const uint16_t* W, const float* x, uint16_t* xh, float* part, float* out, uint32_t inDim, uint32_t outDim, uint32_t rows,
                                  hipStream_t st) {
    return pf_block_call(PfCall{x, xh, part, out, inDim, outDim, rows}, st, [&](auto aux, const PfMul& m) {
        return pf_with_tiles(rows, [&](auto nt) {
            hipLaunchKernelGGL((dense_gemm_rows_kernel<decltype(nt)::value, decltype(aux)::value>), dim3((outDim + 16u * kPfWaves - 1u) / (16u * kPfWaves), m.sp.splits),
                               dim3(64 * kPfWaves), 0, st, W, xh, m.dst, inDim, outDim, rows, m.sp.per);
            return hipGetLastError();
        });
    });
}
// xh: scratch of (xPerSlot ? 2 * rows : rows) * inDim halves; part: dense_gemm_rows_routed_partial_floats floats; groups:
// dense_gemm_rows_routed_group_words words (the counts, then the lists).  out f32 [rows][2][outDim].
hipError_t launch_dense_gemm_rows_routed(const uint16_t* W, uint32_t numExperts, const uint32_t* idx2, const float* x, uint32_t xPerSlot, uint16_t* xh,
                                         float* part, uint32_t* groups, float* out, uint32_t inDim, uint32_t outDim, uint32_t rows, hipStream_t st) {
    return pf_block_call(PfCall{x, xh, part, out, inDim, outDim, rows, true, idx2, groups, numExperts, xPerSlot}, st, [&](auto aux, const PfMul& m) {
        hipLaunchKernelGGL((dense_gemm_rows_routed_kernel<decltype(aux)::value>), dim3((outDim + 16u * kPfWaves - 1u) / (16u * kPfWaves), m.sp.splits, numExperts),
                           dim3(64 * kPfWaves), 0, st, W, xh, m.dst, m.cnt, m.list, inDim, outDim, m.assigns, m.xRows, m.xShift, m.sp.per);
        return hipGetLastError();
    });
}

}  // namespace effort
