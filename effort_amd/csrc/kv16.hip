// The compact f16 KV cache: its writers and the split decode attention over it.
//
//   K, V: _Float16 [maxTokens][numHeadsKV][headDim], row t = token t.  KV head g serves query heads g R .. g R + R - 1, R = numHeads /
//   numHeadsKV.  Against the f32 cache [maxTokens][numHeads][headDim] of decode.hip (a KV head stored once per query head it serves) that
//   is 1 / (2 R) of the memory -- an eighth at Mistral's R = 4 -- and of the bytes a prefill writes, and half the bytes the split
//   attention of attention_split.hip reads, which already fetches one copy per group.  maxTokens to 32768.
//
// Writers.  rope_kv_f16_kernel / rope_kv_rows_f16_kernel: grid numHeads + numHeadsKV (x rows), block headDim.  Rows below numHeads rope
// one query head into qOut (f32: rope_kv_row's expression, its bits); the others rope one KV head's k and store half_rn of the f32
// value rope_kv_row stores, and half_rn(xv), at cache row pos -- each element written once.  Overflow stores +-inf.
//
// attention_split_f16_kernel has attention_split_kernel's contract (attention_split.hip: grid (numHeadsKV, S), 256 threads, the key
// tiles of split s from *pos through attention_split_tiles, a partial state (m, l, acc) per (head, split) into the same scratch, merged
// by attention_merge_kernel; no atomics, flags or waiting; a key at or past nTok clamped to row nTok - 1 and its score SELECTED to
// -inf) and its wave / tile / softmax / merge structure.  What the format changes inside a wave, per tile of 64 keys:
//   scores   headDim / 8 lanes per key as there, but a lane's 8 dims are ONE 16-byte load: a tile is headDim / 8 passes of 4 registers
//            -- 32 / 64 / 128 at headDim 64 / 128 / 256, half of the f32 kernel's.  So EVERY key load of a tile is in flight before the
//            first is consumed at headDim 64 and 128 (the f32 kernel batches 8 of 16 passes); headDim 256 goes in two batches of 16.
//   values   R <= 4: headDim / 8 lanes per key, one 16-byte load each into 8 accumulators per head and lane; R = 8: headDim / 4 lanes
//            per key, one 8-byte load each into 4 (8 x 8 accumulators beside 8 x 8 query values left no room for a tile of keys).  32
//            registers of value loads go out beside the tile's first key loads, under the scores and the softmax.
// The halves are widened in registers (v_cvt_f32_f16), q stays f32, both products are f32 FMA chains: the only rounding beyond the f32
// kernel's is the cache's own.  No instantiation has a scratch segment (DESIGN 4.4c has the table).
//
// A clamped key adds fmaf(0, v[nTok - 1], acc), as in the f32 kernel.  This format stores +-inf where a value overflows, so with an inf
// in V's last live row a tile with clamped keys turns the accumulator NaN (0 * inf) where the row's own weight would have made it inf:
// non-finite either way, but not the same non-finite value.
// Reads: q, *pos, rows 0 .. nTok - 1 of KV head g, nTok = min(pos + 1, maxTokens).  Writes: the scratch only (the merge: out).  The
// output's bits are a function of q, cache rows 0 .. pos, pos, S and R, and repeat run to run.
#include "attention_split.h"
#include "effort_internal.h"
#include "kv16_device.h"

namespace effort {

// ---- writers
__global__ void rope_kv_f16_kernel(const float* __restrict__ xq, const float* __restrict__ xk, const float* __restrict__ xv,
                                   float* __restrict__ qOut, _Float16* __restrict__ kCache, _Float16* __restrict__ vCache,
                                   const uint32_t* __restrict__ posPtr, uint32_t numHeads, uint32_t numHeadsKV, float logBase,
                                   uint32_t maxTokens, int* __restrict__ status) {
    const uint32_t pos = posPtr[0];
    if (pos >= maxTokens) {                            // past the cache: nothing is written, the context's status word says so
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    rope_kv_f16_row(xq, xk, xv, qOut, kCache, vCache, pos, pos, blockIdx.x, numHeads, numHeadsKV, logBase);
}
// row blockIdx.y of the block at position pos0 + blockIdx.y (no guard: the host checked the range)
__global__ void rope_kv_rows_f16_kernel(const float* __restrict__ xq, const float* __restrict__ xk, const float* __restrict__ xv,
                                        float* __restrict__ qOut, _Float16* __restrict__ kCache, _Float16* __restrict__ vCache,
                                        uint32_t pos0, uint32_t numHeads, uint32_t numHeadsKV, float logBase) {
    const size_t qOff = (size_t)blockIdx.y * numHeads * blockDim.x, kvOff = (size_t)blockIdx.y * numHeadsKV * blockDim.x;
    rope_kv_f16_row(xq + qOff, xk + kvOff, xv + kvOff, qOut + qOff, kCache, vCache, pos0 + blockIdx.y, pos0 + blockIdx.y, blockIdx.x,
                    numHeads, numHeadsKV, logBase);
}

// ---- the split decode attention
template <int HD, int R>
__global__ __launch_bounds__(64 * kAsWaves) void attention_split_f16_kernel(const float* __restrict__ q, const _Float16* __restrict__ kCache,
                                                                            const _Float16* __restrict__ vCache, const uint32_t* __restrict__ posPtr,
                                                                            float* __restrict__ scratch, uint32_t numHeads, uint32_t maxTokens) {
    constexpr int LPK = HD / 8, KPP = 64 / LPK, KB = LPK < 16 ? LPK : 16, NKB = LPK / KB;   // lanes per key, keys per pass; a tile is LPK passes, in batches of KB
    constexpr int VD = R <= 4 ? 8 : 4, VW = VD / 2;                              // values: dims per lane, words per load
    constexpr int LPV = HD / VD, KPV = 64 / LPV, VB = 64 / VD, NVB = LPV / VB;   // ... a tile is LPV passes, in batches of VB (32 registers)
    __shared__ alignas(16) float sc[kAsWaves][64][R];                            // a wave's strip: scores, then probabilities, of its tile
    __shared__ alignas(16) float ob[kAsWaves][R][HD];
    __shared__ float ms[kAsWaves][R], ls[kAsWaves][R];
    const uint32_t g = blockIdx.x, s = blockIdx.y, S = gridDim.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), head0 = g * R;
    const uint32_t sub = lane % LPK, kk = lane / LPK;                            // scores: this lane's 8 dims, its key of a pass
    const uint32_t dv = (lane % LPV) * VD, kv = lane / LPV;                      // values: this lane's VD dims, its key of a pass
    float* ml = scratch + (size_t)numHeads * S * HD;

    // the queries do not depend on the position: asked for beside it
    float q8[R][8];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const float4* qp = reinterpret_cast<const float4*>(q + (size_t)(head0 + r) * HD + sub * 8u);
        const float4 a = qp[0], b = qp[1];
        q8[r][0] = a.x; q8[r][1] = a.y; q8[r][2] = a.z; q8[r][3] = a.w; q8[r][4] = b.x; q8[r][5] = b.y; q8[r][6] = b.z; q8[r][7] = b.w;
    }
    const uint32_t nTok = min(posPtr[0] + 1u, maxTokens);
    uint32_t t0, t1;
    attention_split_tiles(nTok, S, s, t0, t1);
    if (t0 >= t1) {                                                              // (uniform) nothing to do: the neutral state
        if (tid < (uint32_t)R) { ml[((size_t)(head0 + tid) * S + s) * 2u] = -INFINITY; ml[((size_t)(head0 + tid) * S + s) * 2u + 1u] = 0.0f; }
        return;
    }
    const uint32_t last = nTok - 1u;
    const size_t rowStride = (size_t)gridDim.x * HD;                             // numHeadsKV heads per row
    const _Float16* kBase = kCache + (size_t)g * HD + sub * 8u;
    const _Float16* vBase = vCache + (size_t)g * HD + dv;
    const float scale = 1.0f / sqrtf((float)HD);

    float m[R], l[R], acc[R][VD];
#pragma unroll
    for (int r = 0; r < R; r++) {
        m[r] = -INFINITY; l[r] = 0.0f;
#pragma unroll
        for (int i = 0; i < VD; i++) acc[r][i] = 0.0f;
    }

    for (uint32_t t = t0 + ((wave + 4u - (t0 & 3u)) & 3u); t < t1; t += kAsWaves) {       // (uniform in the wave)
        const uint32_t key0 = t * kSplitTile;
        uint32_t vw[VB][VW];
#pragma unroll
        for (int kb = 0; kb < NKB; kb++) {
            uint32_t kw[KB][4];
#pragma unroll
            for (int u = 0; u < KB; u++) {
                const uint32_t key = key0 + (uint32_t)(kb * KB + u) * KPP + kk;
                kv_load<4>(kBase + (size_t)min(key, last) * rowStride, kw[u]);
            }
            if (kb == 0) {
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    const uint32_t key = key0 + (uint32_t)u * KPV + kv;
                    kv_load<VW>(vBase + (size_t)min(key, last) * rowStride, vw[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < KB; u++) {
                const uint32_t kt = (uint32_t)(kb * KB + u) * KPP + kk;                   // key within the tile
                const bool live = key0 + kt < nTok;
                float kf[8];
                kv_widen<4>(kw[u], kf);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    float dot = q8[r][0] * kf[0];
#pragma unroll
                    for (int i = 1; i < 8; i++) dot = fmaf(q8[r][i], kf[i], dot);
                    dot = as_key_sum<LPK>(dot);
                    if (sub == (uint32_t)(LPK - 1)) sc[wave][kt][r] = live ? dot * scale : -INFINITY;   // masked by selection
                }
            }
        }
        as_wave_sync();
        {
            float sv[R];
#pragma unroll
            for (int r = 0; r < R; r++) sv[r] = sc[wave][lane][r];
#pragma unroll
            for (int r = 0; r < R; r++) {
                const float mn = fmaxf(m[r], wave_max_f32(sv[r]));
                const float alpha = mn == -INFINITY ? 1.0f : expf(m[r] - mn);
                const float p = sv[r] == -INFINITY ? 0.0f : expf(sv[r] - mn);
                l[r] = l[r] * alpha + wave_sum_f32(p);
                m[r] = mn;
                if (alpha != 1.0f) {                                                      // (uniform; x * 1 is x: skipping it changes no bit)
#pragma unroll
                    for (int i = 0; i < VD; i++) acc[r][i] *= alpha;
                }
                sv[r] = p;
            }
#pragma unroll
            for (int r = 0; r < R; r++) sc[wave][lane][r] = sv[r];
        }
        as_wave_sync();
#pragma unroll
        for (int vb = 0; vb < NVB; vb++) {
            if (vb > 0) {
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    const uint32_t key = key0 + (uint32_t)(vb * VB + u) * KPV + kv;
                    kv_load<VW>(vBase + (size_t)min(key, last) * rowStride, vw[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < VB; u++) {
                const uint32_t kt = (uint32_t)(vb * VB + u) * KPV + kv;
                float vf[VD];
                kv_widen<VW>(vw[u], vf);
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float p = sc[wave][kt][r];                                      // (a clamped key: an exact 0 on the last live row)
#pragma unroll
                    for (int i = 0; i < VD; i++) acc[r][i] = fmaf(p, vf[i], acc[r][i]);
                }
            }
        }
        as_wave_sync();                                                                   // the strip is rewritten by the next tile
    }

    // the key phases of a wave share m: their accumulators add up (one fixed tree); then the waves' states through LDS, in wave order
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
        for (int i = 0; i < VD; i++) {
#pragma unroll
            for (int off = LPV; off < 64; off <<= 1) acc[r][i] += __shfl_xor(acc[r][i], off);
            if (kv == 0u) ob[wave][r][dv + i] = acc[r][i];
        }
        if (lane == 0u) { ms[wave][r] = m[r]; ls[wave][r] = l[r]; }
    }
    __syncthreads();
    for (uint32_t idx = tid; idx < (uint32_t)(R * HD); idx += 64u * kAsWaves) {
        const uint32_t r = idx / HD, d = idx % HD;
        float M = ms[0][r];                                                               // (the split has a tile and the tile a live key: M is finite)
#pragma unroll
        for (int w = 1; w < kAsWaves; w++) M = fmaxf(M, ms[w][r]);
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int w = 0; w < kAsWaves; w++) {
            const float e = ms[w][r] == -INFINITY ? 0.0f : expf(ms[w][r] - M);           // a wave without a tile: an exact zero
            num += ob[w][r][d] * e;
            den += ls[w][r] * e;
        }
        const size_t slot = (size_t)(head0 + r) * S + s;
        scratch[slot * HD + d] = num;
        if (d == 0u) { ml[slot * 2u] = M; ml[slot * 2u + 1u] = den; }
    }
}

hipError_t launch_rope_kv_f16(const float* xq, const float* xk, const float* xv, float* qOut, _Float16* kCache, _Float16* vCache,
                              const uint32_t* pos, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, float ropeBase, uint32_t maxTokens,
                              int* status, hipStream_t st) {
    hipLaunchKernelGGL(rope_kv_f16_kernel, dim3(numHeads + numHeadsKV), dim3(headDim), 0, st, xq, xk, xv, qOut, kCache, vCache, pos, numHeads,
                       numHeadsKV, logf(ropeBase), maxTokens, status);
    return hipGetLastError();
}
hipError_t launch_rope_kv_rows_f16(const float* xq, const float* xk, const float* xv, float* qOut, _Float16* kCache, _Float16* vCache,
                                   uint32_t pos0, uint32_t rows, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, float ropeBase,
                                   hipStream_t st) {
    hipLaunchKernelGGL(rope_kv_rows_f16_kernel, dim3(numHeads + numHeadsKV, rows), dim3(headDim), 0, st, xq, xk, xv, qOut, kCache, vCache, pos0,
                       numHeads, numHeadsKV, logf(ropeBase));
    return hipGetLastError();
}
// the caller checked: kv16_shape_ok (R in {1, 2, 4, 8}, headDim 64 / 128 / 256, 1 <= maxTokens <= 32768), 1 <= S <= kSplitMax
hipError_t launch_attention_split_f16(const float* q, const _Float16* kCache, const _Float16* vCache, const uint32_t* pos, float* out,
                                      float* scratch, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, uint32_t maxTokens, uint32_t S,
                                      hipStream_t st) {
    const dim3 grid(numHeadsKV, S), block(64 * kAsWaves);
    const uint32_t R = numHeads / numHeadsKV;
#define EFFORT_AS_CASE(HD_, R_)                                                                                                              \
    if (headDim == HD_ && R == R_) {                                                                                                         \
        hipLaunchKernelGGL((attention_split_f16_kernel<HD_, R_>), grid, block, 0, st, q, kCache, vCache, pos, scratch, numHeads, maxTokens); \
    } else
#define EFFORT_AS_HD(HD_) EFFORT_AS_CASE(HD_, 1) EFFORT_AS_CASE(HD_, 2) EFFORT_AS_CASE(HD_, 4) EFFORT_AS_CASE(HD_, 8)
    EFFORT_AS_HD(64) EFFORT_AS_HD(128) EFFORT_AS_HD(256) return hipErrorInvalidValue;
#undef EFFORT_AS_HD
#undef EFFORT_AS_CASE
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_attention_merge(scratch, out, numHeads, headDim, S, st);
}

}  // namespace effort
