// Decode attention for long contexts: the keys of a step split across workgroups, ONE cache copy read per KV group.
//
//   out[h] = softmax(q[h] . K[t] / sqrt(headDim)) . V[t],  t = 0 .. pos,  for the one query of a token step
//
// rope_attention_kernel / attention_kernel (decode.hip) are one workgroup per query head -- 32 workgroups on 256 CUs -- and each reads
// its own copy of K / V from the expanded cache [maxTokens][numHeads][headDim], although the R = numHeads / numHeadsKV heads of a group
// hold the same bits (rope_kv_row writes them).  Here the step is two plain launches in stream order:
//
//   attention_split_kernel  grid (numHeadsKV, S), 256 threads.  Workgroup (g, s) serves the R query heads of KV group g over the key
//                           tiles of split s (attention_split.h: tiles of 64 keys from token 0, ceil(tiles / S) consecutive tiles per
//                           split, computed on the device from *pos: the grid does not depend on the position, so a captured step
//                           replays at every position).  It reads the cache copy of head g * R ALONE and leaves, per (head, split), a
//                           partial online-softmax state (m, l, acc[headDim]) in the caller's scratch.  A split without tiles writes
//                           m = -inf, l = 0 and returns before any cache load.
//   attention_merge_kernel  grid numHeads, block headDim: M = max m_s, out = sum acc_s e^(m_s - M) / sum l_s e^(m_s - M) over the
//                           splits in ascending s, an empty split SELECTED out (its weight is a literal 0, e^(-inf + inf) is not asked for).
// No workgroup waits for another inside a launch: no atomics, counters or flags.
//
// Inside a workgroup a wave owns whole tiles: tile t (absolute index) belongs to wave t % 4, a wave takes its tiles in ascending order.
// Per tile:
//   scores   headDim / 8 lanes per key, two 16-byte loads each (rope_attention_kernel's layout), so a pass of the wave covers
//            512 / headDim keys and a tile is headDim / 8 passes.  The loads of 8 passes (16 KB per wave) are issued before any is
//            consumed -- NOT the whole tile: at headDim 128 that would be 128 registers of keys beside the R x 8 query values, and 256
//            at headDim 256; 64 keeps every instantiation clear of scratch (the figures are in DESIGN 4.4b).  A fetched row is
//            multiplied against all R queries out of registers; a key's lanes are summed on DPP (row_shr within 8 or 16 lanes; headDim
//            256 adds one cross-row exchange) and the key's last lane writes R scores into the wave's LDS strip [64][R].
//            A key at or past nTok is CLAMPED to row nTok - 1 and its score selected to -inf.
//   softmax  lane = key.  attention_block's rule per head: mn = max(m, tile max), alpha = e^(m - mn) (1 while nothing is live),
//            p = e^(s - mn) or a selected 0, l = l alpha + sum p, and the accumulator is rescaled only where the max moved.
//   values   headDim / 4 lanes per key, ONE 16-byte load each into R float4 accumulators per lane (p read back from the strip); the
//            first 16 passes' loads are issued beside the tile's first key loads, under the scores and the softmax.
// At the end the key phases of a wave add up over xor exchanges (one fixed tree), the four waves' states merge through LDS in wave order.
// LDS: R KB of strips + 16 R headDim bytes for the merge -- 12 KB at R = 4, headDim 128 -- whatever maxTokens and the position are.
//
// Reads: q, *pos, and rows 0 .. nTok - 1 of head g * R's copy, nTok = min(pos + 1, maxTokens).  Writes: the scratch only (the merge: out).
// The output's bits are a function of q, cache rows 0 .. pos, pos, S and R; they repeat run to run and are NOT effort_attention's.
#include "attention_split.h"
#include "effort_internal.h"

namespace effort {

template <int HD, int R>
__global__ __launch_bounds__(64 * kAsWaves) void attention_split_kernel(const float* __restrict__ q, const float* __restrict__ kCache,
                                                                        const float* __restrict__ vCache, const uint32_t* __restrict__ posPtr,
                                                                        float* __restrict__ scratch, uint32_t numHeads, uint32_t maxTokens) {
    constexpr int LPK = HD / 8, KPP = 64 / LPK, KB = 8, NKB = LPK / KB;        // lanes per key, keys per pass; a tile is LPK passes, in batches of KB
    constexpr int LPV = HD / 4, KPV = 64 / LPV, VB = 16, NVB = LPV / VB;       // ... of the values: a tile is LPV passes, in batches of VB
    __shared__ alignas(16) float sc[kAsWaves][64][R];                            // a wave's strip: scores, then probabilities, of its tile
    __shared__ alignas(16) float ob[kAsWaves][R][HD];
    __shared__ float ms[kAsWaves][R], ls[kAsWaves][R];
    const uint32_t g = blockIdx.x, s = blockIdx.y, S = gridDim.y, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6), head0 = g * R;
    const uint32_t sub = lane % LPK, kk = lane / LPK;                            // scores: this lane's 8 dims, its key of a pass
    const uint32_t d4 = (lane % LPV) * 4u, kv = lane / LPV;                      // values: this lane's 4 dims, its key of a pass
    float* ml = scratch + (size_t)numHeads * S * HD;

    // the queries do not depend on the position: asked for beside it
    float4 qa[R], qb[R];
#pragma unroll
    for (int r = 0; r < R; r++) {
        const float4* qp = reinterpret_cast<const float4*>(q + (size_t)(head0 + r) * HD + sub * 8u);
        qa[r] = qp[0]; qb[r] = qp[1];
    }
    const uint32_t nTok = min(posPtr[0] + 1u, maxTokens);
    uint32_t t0, t1;
    attention_split_tiles(nTok, S, s, t0, t1);
    if (t0 >= t1) {                                                              // (uniform) nothing to do: the neutral state
        if (tid < (uint32_t)R) { ml[((size_t)(head0 + tid) * S + s) * 2u] = -INFINITY; ml[((size_t)(head0 + tid) * S + s) * 2u + 1u] = 0.0f; }
        return;
    }
    const uint32_t last = nTok - 1u;
    const size_t rowStride = (size_t)numHeads * HD;
    const float* kBase = kCache + (size_t)head0 * HD + sub * 8u;
    const float* vBase = vCache + (size_t)head0 * HD + d4;
    const float scale = 1.0f / sqrtf((float)HD);

    float m[R], l[R];
    float4 acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) { m[r] = -INFINITY; l[r] = 0.0f; acc[r] = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }

    for (uint32_t t = t0 + ((wave + 4u - (t0 & 3u)) & 3u); t < t1; t += kAsWaves) {       // (uniform in the wave)
        const uint32_t key0 = t * kSplitTile;
        float4 vf[VB];
#pragma unroll
        for (int kb = 0; kb < NKB; kb++) {
            float4 ka[KB], kc[KB];
#pragma unroll
            for (int u = 0; u < KB; u++) {
                const uint32_t key = key0 + (uint32_t)(kb * KB + u) * KPP + kk;
                const float4* kp = reinterpret_cast<const float4*>(kBase + (size_t)min(key, last) * rowStride);
                ka[u] = kp[0]; kc[u] = kp[1];
            }
            if (kb == 0) {
#pragma unroll
                for (int u = 0; u < VB; u++) {
                    const uint32_t key = key0 + (uint32_t)u * KPV + kv;
                    vf[u] = *reinterpret_cast<const float4*>(vBase + (size_t)min(key, last) * rowStride);
                }
            }
#pragma unroll
            for (int u = 0; u < KB; u++) {
                const uint32_t kt = (uint32_t)(kb * KB + u) * KPP + kk;                   // key within the tile
                const bool live = key0 + kt < nTok;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    float dot = qa[r].x * ka[u].x + qa[r].y * ka[u].y + qa[r].z * ka[u].z + qa[r].w * ka[u].w +
                                qb[r].x * kc[u].x + qb[r].y * kc[u].y + qb[r].z * kc[u].z + qb[r].w * kc[u].w;
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
                    acc[r].x *= alpha; acc[r].y *= alpha; acc[r].z *= alpha; acc[r].w *= alpha;
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
                    vf[u] = *reinterpret_cast<const float4*>(vBase + (size_t)min(key, last) * rowStride);
                }
            }
#pragma unroll
            for (int u = 0; u < VB; u++) {
                const uint32_t kt = (uint32_t)(vb * VB + u) * KPV + kv;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float p = sc[wave][kt][r];                                      // (a clamped key: an exact 0 on a finite row)
                    acc[r].x += p * vf[u].x; acc[r].y += p * vf[u].y; acc[r].z += p * vf[u].z; acc[r].w += p * vf[u].w;
                }
            }
        }
        as_wave_sync();                                                                   // the strip is rewritten by the next tile
    }

    // the key phases of a wave share m: their accumulators add up (one fixed tree); then the waves' states through LDS, in wave order
#pragma unroll
    for (int r = 0; r < R; r++) {
#pragma unroll
        for (int off = LPV; off < 64; off <<= 1) {
            acc[r].x += __shfl_xor(acc[r].x, off); acc[r].y += __shfl_xor(acc[r].y, off);
            acc[r].z += __shfl_xor(acc[r].z, off); acc[r].w += __shfl_xor(acc[r].w, off);
        }
        if (kv == 0u) *reinterpret_cast<float4*>(&ob[wave][r][d4]) = acc[r];
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

// grid = numHeads, block = headDim (>= 64 >= S)
__global__ __launch_bounds__(256) void attention_merge_kernel(const float* __restrict__ scratch, float* __restrict__ out, uint32_t S) {
    __shared__ float ms[kSplitMax], ls[kSplitMax], ws[kSplitMax];
    const uint32_t head = blockIdx.x, numHeads = gridDim.x, d = threadIdx.x, HD = blockDim.x;
    const float* acc = scratch + (size_t)head * S * HD + d;
    const float* ml = scratch + (size_t)numHeads * S * HD + (size_t)head * S * 2u;
    if (d < S) { ms[d] = ml[2u * d]; ls[d] = ml[2u * d + 1u]; }
    __syncthreads();
    if (d < S) {
        float M = ms[0];                                                                  // (split 0 owns tile 0 and key 0 is live: M is finite)
        for (uint32_t s = 1; s < S; s++) M = fmaxf(M, ms[s]);
        ws[d] = ms[d] == -INFINITY ? 0.0f : expf(ms[d] - M);
    }
    __syncthreads();
    float num = 0.0f, den = 0.0f;
    for (uint32_t s = 0; s < S; s++) {
        if (ms[s] == -INFINITY) continue;                                                 // (uniform) an empty split: selected out, its acc never read
        num += acc[(size_t)s * HD] * ws[s];
        den += ls[s] * ws[s];
    }
    out[head * HD + d] = num / den;
}

hipError_t launch_attention_merge(const float* scratch, float* out, uint32_t numHeads, uint32_t headDim, uint32_t S, hipStream_t st) {
    hipLaunchKernelGGL(attention_merge_kernel, dim3(numHeads), dim3(headDim), 0, st, scratch, out, S);
    return hipGetLastError();
}

// the caller checked: R = numHeads / numHeadsKV in {1, 2, 4, 8}, headDim 64 / 128 / 256, 1 <= S <= kSplitMax, 1 <= maxTokens <= 8192
hipError_t launch_attention_split(const float* q, const float* kCache, const float* vCache, const uint32_t* pos, float* out, float* scratch,
                                  uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, uint32_t maxTokens, uint32_t S, hipStream_t st) {
    const dim3 grid(numHeadsKV, S), block(64 * kAsWaves);
    const uint32_t R = numHeads / numHeadsKV;
#define EFFORT_AS_CASE(HD_, R_)                                                                                                          \
    if (headDim == HD_ && R == R_) {                                                                                                     \
        hipLaunchKernelGGL((attention_split_kernel<HD_, R_>), grid, block, 0, st, q, kCache, vCache, pos, scratch, numHeads, maxTokens); \
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
