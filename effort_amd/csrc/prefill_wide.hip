// Prompt prefill, WIDE blocks: out[r] = W * f16(x[r]) for up to kPrefillWideMaxRows = EFFORT_PREFILL_WIDE_MAX_ROWS = 256 rows in ONE pass
// over W.  prefill.hip's kernel stops at 64 rows: each of its waves owns one 16-row tile of W and reads every token fragment from LDS
// once per MFMA, so at sixteen token tiles four waves would ask the LDS pipe for four times what it gives, and a 256-element stage of
// 256 tokens would be 128 KB per buffer.  This unit is the tile design for the rows beyond: more tokens share each pass.
//
// CONTRACT: row r of out has, bit for bit, the bits effort_dense_gemm_rows writes for that row.  An element's sum sees only
//   - the k split: pf_split(inDim, outDim), counted in prefill.hip's 64-row groups and 256-element stages -- whatever a workgroup owns here;
//   - the order inside a split: ascending stage, chunk, u -- here ascending 128-element half stages, which is the same sequence of steps;
//   - the k permutation of a step: step (c, u) of a 64-element chunk feeds elements 64c + 16g + 8u + j into k slot 8g + j, W as the A
//     operand and the tokens as B of v_mfma_f32_16x16x32_f16;
//   - zero operands for dead token columns and for k past inDim (those steps are still taken);
//   - reduce_splits_kernel over the splits, s = 0, 1, ...
// and all of these are prefill.hip's.  How W rows and token columns are dealt to workgroups and waves is free, and is what differs.
//
// The tiling.  A workgroup is 4 waves on 128 rows of W and up to 128 token columns.  A WAVE owns 2 W tiles (32 rows) and ALL the
// workgroup's token tiles (up to 8): a token fragment read from LDS once feeds 2 MFMAs, a W fragment held in registers feeds up to 8 --
// 16 MFMAs per 8 LDS reads where prefill.hip's wave issues 4 per 4.  No second wave needs a wave's W rows, so W goes from global
// memory straight into the A operand, as there: 16 contiguous bytes of a row per lane, 8 loads per lane and half stage.
// f16(x) is staged in LDS in half stages of 128 k x 128 tokens (32 KB, pitch 17 x 16 bytes against bank conflicts), double-buffered:
// the next half stage's token pieces and weight fragments are asked for before the current one is multiplied.  Two buffers are 68 KB,
// so two workgroups fit a CU's 160 KB, and the accumulators (2 x 8 tiles x 4 = 64 registers), two sets of W fragments (2 x 32) and the
// staged pieces (32) stay below the 256 registers that two waves per SIMD leave each.
// The token columns are dealt to ceil(tiles / 8) token groups of equal width (130 rows: 80 + 50, not 128 + 2); a workgroup runs the
// body at ITS live tile count NT = 1 .. 8 (a uniform switch), so 65 rows cost five token tiles, not eight.  Token groups of the same
// W rows are neighbours in blockIdx.x: they are dispatched together and the second reader of a W line finds it in L2 -- which the nt
// stream of a matrix above 64 MiB needs, since nt lines are the first to leave.
#include "prefill.h"

namespace effort {

constexpr int kPwWaves = 4;                        // waves per workgroup
constexpr int kPwWT = 2;                           // 16-row W tiles per wave
constexpr int kPwMaxNT = 8;                        // token tiles per workgroup (every wave multiplies all of them)
constexpr uint32_t kPwRows = 16u * kPwWT * kPwWaves;      // W rows per workgroup: 128
constexpr uint32_t kPwHalf = 128;                  // k elements per LDS stage: half of kPfStage
constexpr int kPwChunks = kPwHalf / 64;            // 64-element chunks per half stage
constexpr uint32_t kPwQ = kPwHalf / 8;             // 16-byte pieces of a token row per half stage
constexpr uint32_t kPwPitch = kPwQ + 1;            // uint4 per staged token row: 256 bytes + 16 of padding
static_assert(kPfStage % kPwHalf == 0, "a split's stages are walked in whole half stages");

// The body at NT live token tiles.  xs: [2][NT * 16][kPwPitch] pieces.  Token column t of the workgroup is row tok0 + t of xh and of o;
// `cols` of them are live.  o = out when there is one split, else this split's slab of the partial sums.
template <int NT, int AUX>
__device__ __forceinline__ void gemm_rows_wide_body(uint4* __restrict__ xs, const uint16_t* __restrict__ W, const uint16_t* __restrict__ xh,
                                                    float* __restrict__ o, uint32_t inDim, uint32_t outDim, uint32_t rows, uint32_t tok0, uint32_t cols,
                                                    uint32_t rowGroup, uint32_t per) {
    auto slot = [&](uint32_t buf, uint32_t tok, uint32_t q) -> uint4& { return xs[(buf * (NT * 16u) + tok) * kPwPitch + q]; };
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t g = lane >> 4, r16 = lane & 15u, row0 = rowGroup * kPwRows + wave * (16u * kPwWT);
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(W), 0, (int)min((size_t)0xFFFFFFFFu, (size_t)outDim * inDim * 2u), 0x00020000);
    const __amdgpu_buffer_rsrc_t xr = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(xh), 0, (int)(rows * inDim * 2u), 0x00020000);
    uint32_t aOff[kPwWT];                                                       // a row past the end re-reads the last one (W < 4 GiB)
#pragma unroll
    for (int w = 0; w < kPwWT; w++) aOff[w] = min(row0 + w * 16u + r16, outDim - 1u) * inDim * 2u;
    const uint32_t stages = (inDim + kPfStage - 1u) / kPfStage;
    const uint32_t s0 = blockIdx.y * per, s1 = min(s0 + per, stages);           // the split's stages (the host made every split non-empty)
    const uint32_t h0 = s0 * (kPfStage / kPwHalf), h1 = s1 * (kPfStage / kPwHalf);   // ... as half stages
    // staging: thread `tid` moves 16-byte piece q = idx % kPwQ of token idx / kPwQ, idx = tid + 256 i: NT * 16 * 16 pieces, NT per thread
    uint4 nextB[NT], curA[kPwWT][kPwChunks][2], nextA[kPwWT][kPwChunks][2];
    auto ask_b = [&](uint32_t h) {
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const uint32_t idx = tid + i * 64u * kPwWaves, tok = idx / kPwQ, e = h * kPwHalf + (idx % kPwQ) * 8u;
            const auto x = __builtin_amdgcn_raw_buffer_load_b128(xr, (tok0 + min(tok, cols - 1u)) * inDim * 2u + min(e, inDim - 8u) * 2u, 0, 0);   // clamped: masked in put_b
            nextB[i] = make_uint4(x[0], x[1], x[2], x[3]);
        }
    };
    auto put_b = [&](uint32_t h, uint32_t buf) {       // (the masks are applied HERE, not beside the loads: a use right behind a load makes it wait)
#pragma unroll
        for (int i = 0; i < NT; i++) {
            const uint32_t idx = tid + i * 64u * kPwWaves, tok = idx / kPwQ, e = h * kPwHalf + (idx % kPwQ) * 8u;
            const uint32_t m = (tok < cols && e < inDim) ? 0xFFFFFFFFu : 0u;    // a dead column, a k past inDim: zeros are staged
            slot(buf, tok, idx % kPwQ) = make_uint4(nextB[i].x & m, nextB[i].y & m, nextB[i].z & m, nextB[i].w & m);
        }
    };
    auto ask_a = [&](uint32_t h, uint4 (&a)[kPwWT][kPwChunks][2]) {
#pragma unroll
        for (int w = 0; w < kPwWT; w++)
#pragma unroll
            for (int c = 0; c < kPwChunks; c++)
#pragma unroll
                for (int u = 0; u < 2; u++) {
                    const uint32_t e = h * kPwHalf + c * 64u + g * 16u + u * 8u;
                    const auto v = __builtin_amdgcn_raw_buffer_load_b128(rs, aOff[w] + min(e, inDim - 8u) * 2u, 0, AUX);   // clamped, branch-free (inDim % 32 == 0)
                    a[w][c][u] = make_uint4(v[0], v[1], v[2], v[3]);
                }
    };
    pf_f32x4 acc[kPwWT][NT];
#pragma unroll
    for (int w = 0; w < kPwWT; w++)
#pragma unroll
        for (int t = 0; t < NT; t++) acc[w][t] = pf_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    ask_a(h0, curA);
    ask_b(h0);
    put_b(h0, 0);
    __syncthreads();
    for (uint32_t h = h0; h < h1; h++) {                                          // (uniform)
        const uint32_t buf = (h - h0) & 1u;
        const bool more = h + 1u < h1;
        if (more) { ask_a(h + 1u, nextA); ask_b(h + 1u); }                        // the next half stage's loads run under this one's products
        __builtin_amdgcn_sched_barrier(0);             // (left to itself the scheduler sinks the loads to their first use)
#pragma unroll
        for (int c = 0; c < kPwChunks; c++)
#pragma unroll
            for (int u = 0; u < 2; u++) {
                const uint32_t m = h * kPwHalf + c * 64u + g * 16u + u * 8u < inDim ? 0xFFFFFFFFu : 0u;    // a clamped lane holds a copy of other data: a zero operand
                pf_half8 af[kPwWT];
#pragma unroll
                for (int w = 0; w < kPwWT; w++)
                    af[w] = __builtin_bit_cast(pf_half8, make_uint4(curA[w][c][u].x & m, curA[w][c][u].y & m, curA[w][c][u].z & m, curA[w][c][u].w & m));
#pragma unroll
                for (int t = 0; t < NT; t++) {
                    const pf_half8 bf = __builtin_bit_cast(pf_half8, slot(buf, t * 16 + r16, c * 8 + g * 2 + u));
#pragma unroll
                    for (int w = 0; w < kPwWT; w++) acc[w][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[w], bf, acc[w][t], 0, 0, 0);
                }
            }
        __builtin_amdgcn_sched_barrier(0);
        if (more) {
            put_b(h + 1u, buf ^ 1u);                        // (read last in the half stage before this one: every wave passed that one's barrier)
#pragma unroll
            for (int w = 0; w < kPwWT; w++)
#pragma unroll
                for (int c = 0; c < kPwChunks; c++)
#pragma unroll
                    for (int u = 0; u < 2; u++) curA[w][c][u] = nextA[w][c][u];
        }
        __syncthreads();
    }
    // Accumulator register i of lane l is W row 4 * (l >> 4) + i, token l & 15.
#pragma unroll
    for (int t = 0; t < NT; t++) {
        const uint32_t tok = t * 16u + r16;
#pragma unroll
        for (int w = 0; w < kPwWT; w++)
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t row = row0 + w * 16u + g * 4u + i;
                if (tok < cols && row < outDim) o[(size_t)(tok0 + tok) * outDim + row] = acc[w][t][i];
            }
    }
}

// grid = (groups of 128 W rows * token groups, splits): blockIdx.x = rowGroup * tokGroups + tokGroup, so the readers of the same W rows are
// neighbours.  Token group j owns columns j * tokPer .. (tokPer: a multiple of 16, at most 128; the last group may hold fewer).
// dst = out when there is one split, else the partial sums [splits][rows][outDim].
template <int AUX>
__global__ __launch_bounds__(64 * kPwWaves, 2) void dense_gemm_rows_wide_kernel(const uint16_t* __restrict__ W, const uint16_t* __restrict__ xh,
                                                                                float* __restrict__ dst, uint32_t inDim, uint32_t outDim, uint32_t rows,
                                                                                uint32_t per, uint32_t tokGroups, uint32_t tokPer) {
    __shared__ uint4 xs[2 * kPwMaxNT * 16 * kPwPitch];
    const uint32_t rowGroup = blockIdx.x / tokGroups, tok0 = (blockIdx.x % tokGroups) * tokPer;
    const uint32_t cols = min(rows - tok0, tokPer);                              // (the host made every token group non-empty)
    float* o = dst + (size_t)blockIdx.y * rows * outDim;
#define EFFORT_PW_CASE(N) case N: gemm_rows_wide_body<N, AUX>(xs, W, xh, o, inDim, outDim, rows, tok0, cols, rowGroup, per); break
    switch ((cols + 15u) / 16u) {                                                // (uniform per workgroup)
        EFFORT_PW_CASE(1); EFFORT_PW_CASE(2); EFFORT_PW_CASE(3); EFFORT_PW_CASE(4);
        EFFORT_PW_CASE(5); EFFORT_PW_CASE(6); EFFORT_PW_CASE(7);
        default: gemm_rows_wide_body<8, AUX>(xs, W, xh, o, inDim, outDim, rows, tok0, cols, rowGroup, per); break;
    }
#undef EFFORT_PW_CASE
}

size_t dense_gemm_rows_wide_partial_floats(uint32_t inDim, uint32_t outDim, uint32_t rows) {
    const PfSplit sp = pf_split(inDim, outDim);
    return sp.splits > 1u ? (size_t)sp.splits * rows * outDim : 0;
}

// xh: scratch of rows * inDim halves; part: scratch of dense_gemm_rows_wide_partial_floats floats.  The sequence is pf_block_call's plain
// one -- convert, multiply into out or the partial sums, reduce -- with this unit's kernel and row limit.
// (More than one split means fewer than 256 64-row groups, outDim < 16384: rows * outDim of the reduce is far below 2^32.)
hipError_t launch_dense_gemm_rows_wide(const uint16_t* W, const float* x, uint16_t* xh, float* part, float* out, uint32_t inDim, uint32_t outDim,
                                       uint32_t rows, hipStream_t st) {
    if (rows < 1u || rows > (uint32_t)kPrefillWideMaxRows) return hipErrorInvalidValue;
    const PfSplit sp = pf_split(inDim, outDim);
    hipError_t e = launch_rows_to_f16(x, xh, rows * inDim, st);
    if (e != hipSuccess) return e;
    const uint32_t tiles = (rows + 15u) / 16u, tokGroups = (tiles + kPwMaxNT - 1u) / kPwMaxNT, tokPer = (tiles + tokGroups - 1u) / tokGroups * 16u;
    const uint32_t liveGroups = (rows + tokPer - 1u) / tokPer;                   // (== tokGroups: equal widths leave no group empty)
    const dim3 grid((outDim + kPwRows - 1u) / kPwRows * liveGroups, sp.splits);
    float* dst = sp.splits > 1u ? part : out;
    e = pf_with_either<0, 2>((size_t)inDim * outDim * 2u > kPfKeepBytes, [&](auto aux) {
        hipLaunchKernelGGL((dense_gemm_rows_wide_kernel<decltype(aux)::value>), grid, dim3(64 * kPwWaves), 0, st, W, xh, dst, inDim, outDim, rows, sp.per,
                           liveGroups, tokPer);
        return hipGetLastError();
    });
    if (e != hipSuccess || sp.splits == 1u) return e;
    return launch_reduce_splits(part, out, rows * outDim, sp.splits, st);
}

}  // namespace effort
