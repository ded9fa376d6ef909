// Token attention over the compact f16 KV cache in ONE launch, for short contexts: rope, the cache write and the attention over tokens
// 0 .. pos (the f16 cache's rope_attention_kernel, decode.hip).  kv16.hip's token step is three launches -- the cache write, the split
// partial states, their merge -- which below a few hundred keys is three dependent launches around almost no work.
//
//   K, V: _Float16 [cacheRows][numHeadsKV][headDim], the plain cache (row t = token t) or the ring while pos < window and pos <
//   ringRows (token t is row t there too, nothing is masked).  The kernel never sees cacheRows: it touches rows 0 .. pos < maxKeys <=
//   cacheRows (the host's check).
//
// Work split.  One workgroup of 256 threads per QUERY head (grid numHeads), not per KV group: at these lengths a step is a chain of
// dependent round trips, and 32 short chains beat 8 that are four times as long.  The R heads of a group read the same rows: L2 traffic
// of tens of KB.
// Who writes.  Every head ropes its own q and its KV head's k (redundant, cheap); the head with head % R == 0 alone stores row pos of
// both caches, each element once, no other row: rope_kv_f16_row's bits (the f32 rope pinned in a register, then ONE conversion, +-inf on
// overflow).
// The newest token.  EVERY head takes the newest token's k and v from LDS, as the ROUNDED value -- the half the cache receives, widened
// back -- never from the row being written: no head waits for another, and the output is a function of what the cache holds after the
// call.  Keys are clamped to row pos - 1, so row pos is not even asked for (at pos 0: row 0, asked for and selected away).
// Data movement.  A key's 8 dims per lane are one 16-byte load of halves: LPK = headDim / 8 lanes per key, KPP = 256 / LPK keys per pass
// (32 / 16 / 8 at headDim 64 / 128 / 256), widened in registers; q stays f32; both products are f32 FMA chains.  A key's lanes are
// summed on DPP (as_key_sum: at headDim 128 one row of 16 lanes).  The values take the same lane map: 8 dims of key kk per lane into 8
// accumulators, the KPP phases added through LDS.
// The dependent chain.  xq / xk / xv of this head are asked for beside the position; the first kPre key passes (clamped to pos) go out
// before the rotation's arithmetic and its barrier; from there keys and values move in batches of kBatch passes (32 registers of halves
// -- what four passes of f32 rows cost rope_attention_kernel), the first batch of value rows going out before the softmax.
// Scores: dynamic LDS [maxKeys] f32 (<= 8 KB).  Softmax and weighted sum as in rope_attention_kernel.
// Guard: *pos >= maxKeys (uniform) writes nothing and raises bit 0 of the decode status.
// A surplus lane (key > pos) carries weight 0 on the newest token's v from LDS, never on a cache row.
#include "attention_split.h"
#include "effort_internal.h"
#include "kv16_device.h"

namespace effort {

constexpr int kShortPre = 4, kShortBatch = 8;          // key passes asked for before the rotation; passes per batch

// the workgroup's maximum / sum, the same value in every thread (red [4]; the barrier in front protects its previous use)
template <bool MAX>
__device__ __forceinline__ float short_block_reduce(float x, float* red) {
    x = MAX ? wave_max_f32(x) : wave_sum_f32(x);
    __syncthreads();
    if ((threadIdx.x & 63u) == 0u) red[threadIdx.x >> 6] = x;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < 4; w++) r = MAX ? fmaxf(r, red[w]) : r + red[w];
    return r;
}

template <int HD>
__global__ __launch_bounds__(256) void rope_attention_f16_kernel(const float* __restrict__ xq, const float* __restrict__ xk,
                                                                 const float* __restrict__ xv, _Float16* __restrict__ kCache,
                                                                 _Float16* __restrict__ vCache, const uint32_t* __restrict__ posPtr,
                                                                 float* __restrict__ out, uint32_t numHeadsKV, uint32_t R, uint32_t maxKeys,
                                                                 float logBase, int* __restrict__ status) {
    constexpr int LPK = HD / 8, KPP = 256 / LPK, PRE = kShortPre, KB = kShortBatch, HALF = HD / 2;
    extern __shared__ float sc[];                      // [maxKeys] scores, then probabilities
    __shared__ float red[4];
    __shared__ alignas(16) float qs[HD], ks[HD], vs[HD];   // this head's roped q; the newest token's k and v AS THE CACHE HOLDS THEM
    __shared__ alignas(16) float part[KPP][HD];        // the phases' weighted sums
    const uint32_t head = blockIdx.x, tid = threadIdx.x, g = head / R;
    const uint32_t sub = tid % LPK, kk = tid / LPK;    // this lane's 8 dims, its key of a pass
    // this head's q / k / v do not depend on the position: asked for beside it, not after it
    float qa = 0.0f, qb = 0.0f, ka = 0.0f, kb = 0.0f, vv = 0.0f, freq = 0.0f;
    if (tid < (uint32_t)HD) {
        const uint32_t d = tid, j = d % HALF, dp = d < (uint32_t)HALF ? d + HALF : d - HALF;
        const float* q = xq + head * HD;
        const float* k = xk + g * HD;
        qa = q[d]; qb = q[dp]; ka = k[d]; kb = k[dp];
        vv = xv[g * HD + d];
        freq = (float)exp((double)logBase * (-(double)j / (double)HALF));
    }
    const uint32_t pos = posPtr[0];
    if (pos >= maxKeys) {                              // past this kernel's range (uniform): nothing is written, the status word says so
        if (head == 0u && tid == 0u) atomicOr(status, 1);
        return;
    }
    const uint32_t nTok = pos + 1u, last = pos ? pos - 1u : 0u;                  // last: the newest row that is NOT being written
    const size_t rowStride = (size_t)numHeadsKV * HD;
    const _Float16* kBase = kCache + (size_t)g * HD + sub * 8u;
    const _Float16* vBase = vCache + (size_t)g * HD + sub * 8u;
    // the first key passes need only the position: asked for here, under the rotation's arithmetic and its barrier
    uint32_t kw[KB][4];
#pragma unroll
    for (int u = 0; u < PRE; u++) kv_load<4>(kBase + (size_t)min((uint32_t)u * KPP + kk, last) * rowStride, kw[u]);
    if (tid < (uint32_t)HD) {
        const uint32_t d = tid;
        const float angle = (float)pos * freq;
        const float c = cosf(angle), s = sinf(angle);
        const float qr = d < (uint32_t)HALF ? qa * c - qb * s : qa * c + qb * s;
        float kr = d < (uint32_t)HALF ? ka * c - kb * s : ka * c + kb * s;
        asm volatile("" : "+v"(kr));                   // the f32 value first, then ONE conversion (rope_kv_f16_row)
        const _Float16 kh = (_Float16)kr, vh = (_Float16)vv;
        qs[d] = qr; ks[d] = (float)kh; vs[d] = (float)vh;
        if (head % R == 0u) {                          // (uniform) one writer per KV head
            const size_t slot = ((size_t)pos * numHeadsKV + g) * HD + d;
            kCache[slot] = kh; vCache[slot] = vh;
        }
    }
#pragma unroll
    for (int u = PRE; u < KB; u++) kv_load<4>(kBase + (size_t)min((uint32_t)u * KPP + kk, last) * rowStride, kw[u]);
    __syncthreads();
    const float scale = 1.0f / sqrtf((float)HD);
    float q8[8], n8[8];                                // this lane's dims of q; of the newest k, then of the newest v
    {
        const float4 a = *reinterpret_cast<const float4*>(qs + sub * 8u), b = *reinterpret_cast<const float4*>(qs + sub * 8u + 4u);
        q8[0] = a.x; q8[1] = a.y; q8[2] = a.z; q8[3] = a.w; q8[4] = b.x; q8[5] = b.y; q8[6] = b.z; q8[7] = b.w;
        const float4 e = *reinterpret_cast<const float4*>(ks + sub * 8u), f = *reinterpret_cast<const float4*>(ks + sub * 8u + 4u);
        n8[0] = e.x; n8[1] = e.y; n8[2] = e.z; n8[3] = e.w; n8[4] = f.x; n8[5] = f.y; n8[6] = f.z; n8[7] = f.w;
    }
    // scores: a batch of KB passes is in flight before the first is consumed
    for (uint32_t t0 = 0u;;) {
#pragma unroll
        for (int u = 0; u < KB; u++) {
            const uint32_t t = t0 + (uint32_t)u * KPP + kk;
            float kf[8];
            kv_widen<4>(kw[u], kf);
            float dot = q8[0] * (t >= pos ? n8[0] : kf[0]);                      // the newest token (and a surplus lane): from LDS, by selection
#pragma unroll
            for (int i = 1; i < 8; i++) dot = fmaf(q8[i], t >= pos ? n8[i] : kf[i], dot);
            dot = as_key_sum<LPK>(dot);                                          // the key's total sits in its last lane
            if (sub == (uint32_t)(LPK - 1) && t < nTok) sc[t] = dot * scale;
        }
        t0 += (uint32_t)(KB * KPP);
        if (t0 >= nTok) break;                                                   // (uniform)
#pragma unroll
        for (int u = 0; u < KB; u++) kv_load<4>(kBase + (size_t)min(t0 + (uint32_t)u * KPP + kk, last) * rowStride, kw[u]);
    }
    // the first batch of value rows does not depend on the scores: asked for HERE, its round trip runs under the softmax
    uint32_t vw[KB][4];
#pragma unroll
    for (int u = 0; u < KB; u++) kv_load<4>(vBase + (size_t)min((uint32_t)u * KPP + kk, last) * rowStride, vw[u]);
    {
        const float4 e = *reinterpret_cast<const float4*>(vs + sub * 8u), f = *reinterpret_cast<const float4*>(vs + sub * 8u + 4u);
        n8[0] = e.x; n8[1] = e.y; n8[2] = e.z; n8[3] = e.w; n8[4] = f.x; n8[5] = f.y; n8[6] = f.z; n8[7] = f.w;
    }
    __syncthreads();
    float m = -INFINITY;
    for (uint32_t t = tid; t < nTok; t += 256u) m = fmaxf(m, sc[t]);
    m = short_block_reduce<true>(m, red);
    float sum = 0.0f;
    for (uint32_t t = tid; t < nTok; t += 256u) { const float e = expf(sc[t] - m); sc[t] = e; sum += e; }
    sum = short_block_reduce<false>(sum, red);          // (its barriers order the probabilities before the reads below)
    const float inv = 1.0f / sum;
    // weighted sum: phase kk takes keys kk, kk + KPP, ...; 8 dims of a key per lane
    float acc[8];
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = 0.0f;
    for (uint32_t t0 = 0u;;) {
#pragma unroll
        for (int u = 0; u < KB; u++) {
            const uint32_t t = t0 + (uint32_t)u * KPP + kk;
            const float p = t < nTok ? sc[t] : 0.0f;
            float vf[8];
            kv_widen<4>(vw[u], vf);
#pragma unroll
            for (int i = 0; i < 8; i++) acc[i] = fmaf(p, t >= pos ? n8[i] : vf[i], acc[i]);
        }
        t0 += (uint32_t)(KB * KPP);
        if (t0 >= nTok) break;                                                   // (uniform)
#pragma unroll
        for (int u = 0; u < KB; u++) kv_load<4>(vBase + (size_t)min(t0 + (uint32_t)u * KPP + kk, last) * rowStride, vw[u]);
    }
    *reinterpret_cast<float4*>(&part[kk][sub * 8u]) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    *reinterpret_cast<float4*>(&part[kk][sub * 8u + 4u]) = make_float4(acc[4], acc[5], acc[6], acc[7]);
    __syncthreads();
    if (tid < (uint32_t)HD) {
        float s2 = 0.0f;
#pragma unroll
        for (int ph = 0; ph < KPP; ph++) s2 += part[ph][tid];
        out[head * HD + tid] = s2 * inv;
    }
}

// the caller checked: kv16_shape_ok on cacheRows, 1 <= maxKeys <= min(cacheRows, kShortMaxKeys)
hipError_t launch_rope_attention_f16(const float* xq, const float* xk, const float* xv, _Float16* kCache, _Float16* vCache, const uint32_t* pos,
                                     float* out, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, uint32_t maxKeys, float ropeBase,
                                     int* status, hipStream_t st) {
    const uint32_t R = numHeads / numHeadsKV;
    const size_t lds = (size_t)maxKeys * sizeof(float);
#define EFFORT_SHORT_CASE(HD_)                                                                                                              \
    if (headDim == HD_) {                                                                                                                   \
        hipLaunchKernelGGL((rope_attention_f16_kernel<HD_>), dim3(numHeads), dim3(256), lds, st, xq, xk, xv, kCache, vCache, pos, out,      \
                           numHeadsKV, R, maxKeys, logf(ropeBase), status);                                                                 \
    } else
    EFFORT_SHORT_CASE(64) EFFORT_SHORT_CASE(128) EFFORT_SHORT_CASE(256) return hipErrorInvalidValue;
#undef EFFORT_SHORT_CASE
    return hipGetLastError();
}

}  // namespace effort
