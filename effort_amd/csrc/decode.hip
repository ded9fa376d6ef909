// Glue kernels of the decode loop around bucketMul (runNetwork.swift:68-316) -- the callers either side of the hot
// path, SURVEY section 8f row 1.  Everything a token needs between two multiplies, with the token position and the
// token id kept in DEVICE memory so that a whole token step can be replayed from one hipGraph (the reference's loop
// spends ~15 ms/token in gaps between its ~25 dispatches per layer, runNetwork.swift:91-103).
//   add_rmsnorm_mul  h += delta; out = h / sqrt(mean(h^2) + 1e-5) * w     rmsNorm32fast + mulVec32by16 + add (aux.metal:113-152,268-274)
//   rope_kv          rope_mx on q and on the 4x repeated k, repeat4x32 of k and v, written at cache[pos]   (aux.metal:218-261)
//   attention        dotSetScore2 (/sqrt(headDim)) + softmax + sumScores32 over tokens 0..pos, one workgroup per head (aux.metal:185-198,379-447)
//   silu_mul         x3 * x1 / (1 + exp(-x1))                              silu32b (matrix.metal:25-35)
//   fetch_row        tok_embeddings row (f16) -> f32                       fetchRow16to32 (aux.metal:355)
//   top2_softmax     Mixtral gate: top-2 experts + softmax of their logits (mpsTopK + softmax, runNetwork.swift:186-189); mix2: weighted sum
//   moe_route        Mixtral routing in ONE launch: rmsNorm * ffnNorm -> dense gate GEMV -> top-2 + softmax (runNetwork.swift:173-175,185-189),
//                    bit for bit what add_rmsnorm_mul -> dense_gemv_kernel<1, 0> -> top2_softmax write in a row
//   mix2_add         h += f0 * val[0] + f1 * val[1]: mix2 and the residual add the next norm would have done (runNetwork.swift:190-199)
//   argmax           greedy pick of the next token (the reference takes mpsTopK[0], helpers/mps.swift:52-84), pos += 1
// add_rmsnorm_mul, rope_kv, attention, fetch_row, moe_route and mix2_add each have a block form (*_rows) over `rows` tokens for prompt prefill: one workgroup
// (fetch: one grid row) per token, running the SAME body as the token form -- per token it writes the token form's bits.
#include "effort_internal.h"

namespace effort {

__device__ __forceinline__ float block_sum(float x, float* red /* [17] */) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    x = wave_sum_f32(x);                              // (DPP scan order; the multiply's fused rmsNorm prologue sums the same way)
    __syncthreads();                                  // red may still be read from a previous call
    if (lane == 0) red[wave] = x;
    __syncthreads();
    float s = 0.0f;
    for (int w = 0; w < nw; w++) s += red[w];         // same order in every thread: identical result everywhere
    return s;
}

__device__ __forceinline__ float block_max(float x, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    x = wave_max_f32(x);
    __syncthreads();
    if (lane == 0) red[wave] = x;
    __syncthreads();
    float s = red[0];
    for (int w = 1; w < nw; w++) s = fmaxf(s, red[w]);
    return s;
}

// One row of n elements, block = 1024; delta may be null (nothing is added, h is not written).
__device__ __forceinline__ void add_rmsnorm_mul_row(float* __restrict__ h, const float* __restrict__ delta, const uint16_t* __restrict__ w,
                                                    float* __restrict__ out, uint32_t n, float* red /* [17] */) {
    // One memory round trip: every load (h, delta, the norm weights) is issued before anything is used, the updated state
    // stays in registers for the second half (n <= 4 * 1024 elements per register slot; a longer state takes the loop
    // below).  This kernel sits on the decode loop's dependent chain twice per layer.
    constexpr int K = 4;
    if (n <= K * 1024u) {
        float x[K], d[K], wf[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const uint32_t i = min(k * 1024u + threadIdx.x, n - 1u);               // clamped, branch-free
            x[k] = h[i];
            d[k] = delta ? delta[i] : 0.0f;
            wf[k] = half_bits_to_float(w[i]);
        }
        float ss = 0.0f;
#pragma unroll
        for (int k = 0; k < K; k++) {
            const bool live = k * 1024u + threadIdx.x < n;
            x[k] += d[k];
            if (live && delta) h[k * 1024u + threadIdx.x] = x[k];
            ss += live ? x[k] * x[k] : 0.0f;
        }
        const float inv = 1.0f / sqrtf(block_sum(ss, red) / (float)n + 1e-5f);            // aux.metal:150
#pragma unroll
        for (int k = 0; k < K; k++)
            if (k * 1024u + threadIdx.x < n) out[k * 1024u + threadIdx.x] = (x[k] * inv) * wf[k];
        return;
    }
    float ss = 0.0f;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        float x = h[i];
        if (delta) { x += delta[i]; h[i] = x; }
        ss += x * x;
    }
    const float inv = 1.0f / sqrtf(block_sum(ss, red) / (float)n + 1e-5f);                // aux.metal:150
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) out[i] = (h[i] * inv) * half_bits_to_float(w[i]);
}

__global__ __launch_bounds__(1024) void add_rmsnorm_mul_kernel(float* __restrict__ h, const float* __restrict__ delta,
                                                               const uint16_t* __restrict__ w, float* __restrict__ out, uint32_t n) {
    __shared__ float red[17];
    add_rmsnorm_mul_row(h, delta, w, out, n, red);
}
// grid = rows, block = 1024: row blockIdx.x of h, delta and out
__global__ __launch_bounds__(1024) void add_rmsnorm_mul_rows_kernel(float* __restrict__ h, const float* __restrict__ delta,
                                                                    const uint16_t* __restrict__ w, float* __restrict__ out, uint32_t n) {
    __shared__ float red[17];
    const size_t row = (size_t)blockIdx.x * n;
    add_rmsnorm_mul_row(h + row, delta ? delta + row : nullptr, w, out + row, n, red);
}

// One head of one token at position pos, block = headDim; q, k, v and qOut point at this head's (k, v: its kv head's) headDim values.
// freq_j = base^(-2j/headDim) (createFreqsCis2, model.swift:693-717: logspace with base 1e-6 <=> theta 1e6), rotate_half
// convention of rope_mx.
__device__ __forceinline__ void rope_kv_row(const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                            float* __restrict__ qOut, float* __restrict__ kCache, float* __restrict__ vCache,
                                            uint32_t pos, uint32_t head, uint32_t numHeads, float logBase) {
    const uint32_t d = threadIdx.x, headDim = blockDim.x, half = headDim / 2;
    const uint32_t j = d % half;
    const float freq = (float)exp((double)logBase * (-(double)j / (double)half));          // Float(freq), model.swift:707
    const float angle = (float)pos * freq;
    const float c = cosf(angle), s = sinf(angle);
    const float qr = d < half ? q[d] * c - q[d + half] * s : q[d] * c + q[d - half] * s;
    const float kr = d < half ? k[d] * c - k[d + half] * s : k[d] * c + k[d - half] * s;
    const size_t slot = ((size_t)pos * numHeads + head) * headDim + d;
    qOut[d] = qr;
    kCache[slot] = kr;
    vCache[slot] = v[d];
}

// grid = numHeads, block = headDim
__global__ void rope_kv_kernel(const float* __restrict__ xq, const float* __restrict__ xk, const float* __restrict__ xv,
                               float* __restrict__ qOut, float* __restrict__ kCache, float* __restrict__ vCache,
                               const uint32_t* __restrict__ posPtr, uint32_t numHeads, uint32_t kvRepeats, float logBase,
                               uint32_t maxTokens, int* __restrict__ status) {
    const uint32_t head = blockIdx.x, headDim = blockDim.x, pos = posPtr[0];
    if (pos >= maxTokens) {                            // past the cache: nothing is written, the context's status word says so
        if (head == 0 && threadIdx.x == 0) atomicOr(status, 1);
        return;
    }
    const uint32_t kvOff = (head / kvRepeats) * headDim;                                   // repeat4x32: kv head y feeds heads 4y..4y+3
    rope_kv_row(xq + head * headDim, xk + kvOff, xv + kvOff, qOut + head * headDim, kCache, vCache, pos, head, numHeads, logBase);
}
// grid = (numHeads, rows), block = headDim: row blockIdx.y at position pos0 + blockIdx.y (no guard: the host checked the range)
__global__ void rope_kv_rows_kernel(const float* __restrict__ xq, const float* __restrict__ xk, const float* __restrict__ xv,
                                    float* __restrict__ qOut, float* __restrict__ kCache, float* __restrict__ vCache,
                                    uint32_t pos0, uint32_t numHeads, uint32_t kvRepeats, float logBase) {
    const uint32_t head = blockIdx.x, r = blockIdx.y, headDim = blockDim.x;
    const size_t qOff = (size_t)r * numHeads * headDim + head * headDim;
    const size_t kvOff = (size_t)r * (numHeads / kvRepeats) * headDim + (head / kvRepeats) * headDim;
    rope_kv_row(xq + qOff, xk + kvOff, xv + kvOff, qOut + qOff, kCache, vCache, pos0 + r, head, numHeads, logBase);
}

// One head of one query over tokens 0 .. nTok - 1, block = 256; qh points at this head's query, out at the token's output row.
// exp(x - max) / sum exp(x - max) == the reference's exp(x) / sum exp(x).
__device__ __forceinline__ void attention_row(const float* __restrict__ qh, const float* __restrict__ kCache, const float* __restrict__ vCache,
                                              uint32_t nTok, float* __restrict__ out, uint32_t head, uint32_t numHeads, uint32_t headDim,
                                              float* sc /* [nTok] scores, then probabilities */, float* red /* [17] */, float* part /* [256] */) {
    const uint32_t tid = threadIdx.x;
    const float scale = 1.0f / sqrtf((float)headDim);
    const int lane = tid & 63, wave = tid >> 6;
    // one wave per token: lanes stride the head dimension
    for (uint32_t t = wave; t < nTok; t += 4) {
        const float* kh = kCache + ((size_t)t * numHeads + head) * headDim;
        float dot = 0.0f;
        for (uint32_t d = lane; d < headDim; d += 64) dot += qh[d] * kh[d];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) dot += __shfl_xor(dot, off);
        if (lane == 0) sc[t] = dot * scale;
    }
    __syncthreads();
    float m = -INFINITY;
    for (uint32_t t = tid; t < nTok; t += 256) m = fmaxf(m, sc[t]);
    m = block_max(m, red);
    float sum = 0.0f;
    for (uint32_t t = tid; t < nTok; t += 256) { const float e = expf(sc[t] - m); sc[t] = e; sum += e; }
    sum = block_sum(sum, red);
    const float inv = 1.0f / sum;
    // sumScores32: out[head][d] = sum_t p_t * v[t][head][d]; threads = (token phase, d)
    const uint32_t d = tid % headDim, ph = tid / headDim, nph = 256 / headDim;
    float acc = 0.0f;
    if (ph < nph)
        for (uint32_t t = ph; t < nTok; t += nph) acc += sc[t] * vCache[((size_t)t * numHeads + head) * headDim + d];
    part[tid] = acc;
    __syncthreads();
    if (tid < headDim) {
        float s2 = 0.0f;
        for (uint32_t p = 0; p < nph; p++) s2 += part[p * headDim + tid];
        out[head * headDim + tid] = s2 * inv;
    }
}

// grid = numHeads, block = 256.  Tokens 0..pos.
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ q, const float* __restrict__ kCache,
                                                        const float* __restrict__ vCache, const uint32_t* __restrict__ posPtr,
                                                        float* __restrict__ out, uint32_t numHeads, uint32_t headDim, uint32_t maxTokens) {
    extern __shared__ float sc[];                      // [maxTokens] scores, then probabilities
    __shared__ float red[17];
    __shared__ float part[256];
    const uint32_t head = blockIdx.x, nTok = min(posPtr[0] + 1u, maxTokens);
    attention_row(q + head * headDim, kCache, vCache, nTok, out, head, numHeads, headDim, sc, red, part);
}
// grid = (numHeads, rows), block = 256: query row blockIdx.y over tokens 0 .. pos0 + blockIdx.y.  Every query of the block reads its
// keys and values from the cache again (no sharing among the block's queries).
__global__ __launch_bounds__(256) void attention_rows_kernel(const float* __restrict__ q, const float* __restrict__ kCache,
                                                             const float* __restrict__ vCache, uint32_t pos0, float* __restrict__ out,
                                                             uint32_t numHeads, uint32_t headDim) {
    extern __shared__ float sc[];                      // [pos0 + rows] scores, then probabilities
    __shared__ float red[17];
    __shared__ float part[256];
    const uint32_t head = blockIdx.x, r = blockIdx.y;
    const size_t row = (size_t)r * numHeads * headDim;
    attention_row(q + row + head * headDim, kCache, vCache, pos0 + r + 1u, out + row, head, numHeads, headDim, sc, red, part);
}

// rope_kv + attention in ONE launch (one workgroup per query head): the head ropes its q and its kv head's k, stores k / v
// at cache[pos], and attends over tokens 0..pos, the newest token straight from LDS.  Saves a dependent launch per layer.
__global__ __launch_bounds__(256) void rope_attention_kernel(const float* __restrict__ xq, const float* __restrict__ xk,
                                                             const float* __restrict__ xv, float* __restrict__ kCache,
                                                             float* __restrict__ vCache, const uint32_t* __restrict__ posPtr,
                                                             float* __restrict__ out, uint32_t numHeads, uint32_t kvRepeats,
                                                             uint32_t headDim, uint32_t maxTokens, float logBase, int* __restrict__ status) {
    extern __shared__ float sc[];                      // [maxTokens] scores, then probabilities
    __shared__ float red[17];
    __shared__ float qs[256], ks[256], vs[256];        // this head's roped q, roped k and v of the newest token
    const uint32_t head = blockIdx.x, tid = threadIdx.x, half = headDim / 2;
    // this head's q / k / v do not depend on the position: asked for beside it, not after it (one dependent round trip less)
    float qa = 0.0f, qb = 0.0f, ka = 0.0f, kb = 0.0f, vv = 0.0f, freq = 0.0f;
    if (tid < headDim) {
        const uint32_t d = tid, j = d % half, dp = d < half ? d + half : d - half;
        const float* q = xq + head * headDim;
        const float* k = xk + (head / kvRepeats) * headDim;
        qa = q[d]; qb = q[dp]; ka = k[d]; kb = k[dp];
        vv = xv[(head / kvRepeats) * headDim + d];
        freq = (float)exp((double)logBase * (-(double)j / (double)half));
    }
    if (posPtr[0] >= maxTokens) {                      // past the cache (uniform): nothing is written, the status word says so
        if (head == 0 && tid == 0) atomicOr(status, 1);
        return;
    }
    const uint32_t pos = posPtr[0], nTok = pos + 1u;
    // the first pass of key rows needs only the position: asked for here, under the rotation's arithmetic and its barrier
    const uint32_t lpt = headDim / 8u, tokPerPass = 256u / lpt, sub = tid % lpt, tk = tid / lpt;
    float4 ka0[4], kb0[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const uint32_t t = min((uint32_t)u * tokPerPass + tk, pos);
        const float4* kh = reinterpret_cast<const float4*>(kCache + ((size_t)t * numHeads + head) * headDim + sub * 8u);
        ka0[u] = kh[0]; kb0[u] = kh[1];
    }
    if (tid < headDim) {
        const uint32_t d = tid;
        const float angle = (float)pos * freq;
        const float c = cosf(angle), s = sinf(angle);
        const float qr = d < half ? qa * c - qb * s : qa * c + qb * s;
        const float kr = d < half ? ka * c - kb * s : ka * c + kb * s;
        const size_t slot = ((size_t)pos * numHeads + head) * headDim + d;
        qs[d] = qr; ks[d] = kr; vs[d] = vv;
        kCache[slot] = kr; vCache[slot] = vv;
    }
    __syncthreads();
    // scores: headDim/8 threads per token, 8 dims each as two float4 loads; four token passes are issued before any is
    // consumed, so the cache reads overlap instead of costing one memory round trip per token
    const float scale = 1.0f / sqrtf((float)headDim);
    float q8[8];
#pragma unroll
    for (int i = 0; i < 8; i++) q8[i] = qs[sub * 8u + i];
    for (uint32_t t0 = 0; t0 < nTok; t0 += tokPerPass * 4u) {
        float4 ka[4], kb[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t t = min(t0 + u * tokPerPass + tk, pos);           // clamped: surplus lanes re-read the newest row
            const float4* kh = reinterpret_cast<const float4*>(kCache + ((size_t)t * numHeads + head) * headDim + sub * 8u);
            if (t0 == 0u) { ka[u] = ka0[u]; kb[u] = kb0[u]; }                  // (uniform: the first pass was asked for before the rotation)
            else { ka[u] = kh[0]; kb[u] = kh[1]; }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t t = t0 + u * tokPerPass + tk;
            float dot;
            if (t >= pos) {                                                   // the newest token: from LDS (its cache row is being written)
                dot = 0.0f;
#pragma unroll
                for (int i = 0; i < 8; i++) dot += q8[i] * ks[sub * 8u + i];
            } else {
                dot = q8[0] * ka[u].x + q8[1] * ka[u].y + q8[2] * ka[u].z + q8[3] * ka[u].w +
                      q8[4] * kb[u].x + q8[5] * kb[u].y + q8[6] * kb[u].z + q8[7] * kb[u].w;
            }
            if (lpt == 16u) {                                                  // (uniform) headDim 128: a token's 16 lanes are one DPP row -- no LDS round trips
                dot = row16_sum_f32(dot);                                      // the row's total sits in its lane 15
                if (sub == 15u && t < nTok) sc[t] = dot * scale;
            } else {
                for (uint32_t off = lpt / 2u; off >= 1u; off >>= 1) dot += __shfl_xor(dot, (int)off);
                if (sub == 0 && t < nTok) sc[t] = dot * scale;
            }
        }
    }
    // the first eight tokens' value rows of this thread's phase do not depend on the scores: asked for HERE, their round trip runs
    // under the softmax instead of after it (a decode step's attention is a chain of dependent round trips: position, q/k/v,
    // keys, values)
    const uint32_t tpr = headDim / 4u, nph = 256u / tpr, d4 = (tid % tpr) * 4u, ph = tid / tpr;
    float4 vv0[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
        const uint32_t tc = min(ph + (uint32_t)u * nph, pos);
        vv0[u] = *reinterpret_cast<const float4*>(vCache + ((size_t)tc * numHeads + head) * headDim + d4);
    }
    __syncthreads();
    float m = -INFINITY;
    for (uint32_t t = tid; t < nTok; t += 256) m = fmaxf(m, sc[t]);
    m = block_max(m, red);
    float sum = 0.0f;
    for (uint32_t t = tid; t < nTok; t += 256) { const float e = expf(sc[t] - m); sc[t] = e; sum += e; }
    sum = block_sum(sum, red);
    const float inv = 1.0f / sum;
    // weighted sum: headDim/4 threads per token phase (one float4 of the head each), 256/(headDim/4) phases; eight
    // tokens' loads in flight per thread
    float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t t0 = ph; t0 < nTok; t0 += nph * 8u) {
        float4 vv[8]; float p8[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t t = t0 + u * nph;
            const uint32_t tc = min(t, pos);
            if (t0 == ph) vv[u] = vv0[u];                                   // (the first pass was asked for before the softmax)
            else vv[u] = *reinterpret_cast<const float4*>(vCache + ((size_t)tc * numHeads + head) * headDim + d4);
            p8[u] = t < nTok ? sc[t] : 0.0f;
            if (t == pos) vv[u] = make_float4(vs[d4], vs[d4 + 1], vs[d4 + 2], vs[d4 + 3]);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) { acc.x += p8[u] * vv[u].x; acc.y += p8[u] * vv[u].y; acc.z += p8[u] * vv[u].z; acc.w += p8[u] * vv[u].w; }
    }
    __shared__ float4 part4[256];
    part4[tid] = acc;
    __syncthreads();
    if (tid < tpr) {
        float4 s2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        for (uint32_t p = 0; p < nph; p++) { const float4 x = part4[p * tpr + tid]; s2.x += x.x; s2.y += x.y; s2.z += x.z; s2.w += x.w; }
        *reinterpret_cast<float4*>(out + head * headDim + d4) = make_float4(s2.x * inv, s2.y * inv, s2.z * inv, s2.w * inv);
    }
}

__global__ void silu_mul_kernel(const float* __restrict__ x1, const float* __restrict__ x3, float* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = x3[i] * x1[i] / (1.0f + expf(-x1[i]));
}

// out[i] = table row idPtr[0], element i
__device__ __forceinline__ void fetch_row_elem(const uint16_t* __restrict__ emb, const uint32_t* __restrict__ idPtr, float* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = half_bits_to_float(emb[(size_t)idPtr[0] * n + i]);
}
__global__ void fetch_row_kernel(const uint16_t* __restrict__ emb, const uint32_t* __restrict__ idPtr, float* __restrict__ out, uint32_t n) {
    fetch_row_elem(emb, idPtr, out, n);
}
// grid = (n / 256, rows): row ids[blockIdx.y] into row blockIdx.y of out
__global__ void fetch_rows_kernel(const uint16_t* __restrict__ emb, const uint32_t* __restrict__ ids, float* __restrict__ out, uint32_t n) {
    fetch_row_elem(emb, ids + blockIdx.y, out + (size_t)blockIdx.y * n, n);
}

// one workgroup: greedy next token = index of the largest logit (lowest index on ties); advances the position
__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ logits, uint32_t n, uint32_t* __restrict__ idOut,
                                                      uint32_t* __restrict__ posPtr, uint32_t* __restrict__ history,
                                                      uint32_t historyLen, int* __restrict__ status) {
    __shared__ float bv[16];
    __shared__ uint32_t bi[16];
    float best = -INFINITY; uint32_t idx = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const float x = logits[i];
        if (x > best || (x == best && i < idx)) { best = x; idx = i; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off); const uint32_t oi = (uint32_t)__shfl_xor((int)idx, off);
        if (ob > best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if ((threadIdx.x & 63) == 0) { bv[threadIdx.x >> 6] = best; bi[threadIdx.x >> 6] = idx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (uint32_t w = 1; w < (blockDim.x >> 6); w++)
            if (bv[w] > best || (bv[w] == best && bi[w] < idx)) { best = bv[w]; idx = bi[w]; }
        if (idx >= n) { idx = 0; atomicOr(status, 2); }           // every logit NaN: a valid id all the same (the next fetch_row reads row idx)
        idOut[0] = idx;
        if (history) {
            if (posPtr[0] < historyLen) history[posPtr[0]] = idx;
            else atomicOr(status, 1);                                 // past the history buffer: not written
        }
        posPtr[0] += 1u;
    }
}

// Mixtral routing (runNetwork.swift:185-199): mpsTopK(topK: 2) of the gate logits, softmax over the two picked values.
__device__ __forceinline__ void top2_softmax_scan(const float* gate, uint32_t n, uint32_t* __restrict__ idx, float* __restrict__ val) {
    uint32_t i0 = 0xFFFFFFFFu, i1 = 0xFFFFFFFFu; float v0 = -INFINITY, v1 = -INFINITY;
    for (uint32_t i = 0; i < n; i++) {
        const float x = gate[i];
        if (x > v0) { v1 = v0; i1 = i0; v0 = x; i0 = i; }     // (the first hit hands on i0's "none yet", not an index)
        else if (x > v1) { v1 = x; i1 = i; }
    }
    if (i0 == 0xFFFFFFFFu) i0 = 0;                            // nothing above -inf: a valid index all the same
    if (i1 == 0xFFFFFFFFu) { i1 = i0; v1 = v0; }              // no runner-up (one expert): the winner twice, 0.5 / 0.5
    const float e1 = expf(v1 - v0), inv = 1.0f / (1.0f + e1);
    idx[0] = i0; idx[1] = i1; val[0] = inv; val[1] = e1 * inv;
}
__global__ void top2_softmax_kernel(const float* __restrict__ gate, uint32_t n, uint32_t* __restrict__ idx, float* __restrict__ val) {
    if (threadIdx.x != 0) return;
    top2_softmax_scan(gate, n, idx, val);
}
// out = f0 * val[0] + f1 * val[1]   (ffnOut[i].mul(by: gateVals[i]); h.add(by: ffnOut[i]) -- the add rides in the next norm)
__global__ void mix2_kernel(const float* __restrict__ f0, const float* __restrict__ f1, const float* __restrict__ val,
                            float* __restrict__ out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = f0[i] * val[0] + f1[i] * val[1];
}

// h += f0 * val[0] + f1 * val[1]: mix2_kernel's expression, then the one f32 add the next add_rmsnorm_mul would have performed
__device__ __forceinline__ void mix2_add_row(float* __restrict__ h, const float* __restrict__ f0, const float* __restrict__ f1,
                                             const float* __restrict__ val, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) h[i] = h[i] + (f0[i] * val[0] + f1[i] * val[1]);
}
__global__ void mix2_add_kernel(float* __restrict__ h, const float* __restrict__ f0, const float* __restrict__ f1,
                                const float* __restrict__ val, uint32_t n) {
    mix2_add_row(h, f0, f1, val, n);
}
// grid = (ceil(n / 256), rows): row blockIdx.y of h [rows][n], f [rows][2][n] (f0 = f[r][0], f1 = f[r][1]) and val [rows][2]
__global__ void mix2_add_rows_kernel(float* __restrict__ h, const float* __restrict__ f, const float* __restrict__ val, uint32_t n) {
    const size_t r = blockIdx.y;
    mix2_add_row(h + r * n, f + 2u * r * n, f + (2u * r + 1u) * n, val + 2u * r, n);
}

// Mixtral routing in ONE launch of one workgroup (16 waves): x = rmsNorm(h) * w -> gate[e] = gateW[e] . f16(x) -> top-2 + softmax.
// The three kernels it replaces sit on the token's dependent chain, each a launch that reads a few KB and waits for the one before.
// Every sum runs in THEIR order, so idx / val (and the logits) are theirs bit for bit:
//   norm   thread t squares elements t, t + 1024, ... in that order; block_sum; (x * inv) * w      (add_rmsnorm_mul_kernel, both its paths)
//   gate   a lane owns 8 consecutive halves of every 512-element chunk: an fmaf chain from 0 over the 8, chunk sums added to the lane's
//          accumulator in ascending chunk order (the chunk straddling n masked per lane), the xor butterfly 32 .. 1   (dense_gemv_kernel<1, 0>)
//   top-2  top2_softmax_scan
// A wave owns an expert row (rows beyond 16 go round again).  The gate rows do not depend on the norm: a wave's first eight 16-byte
// row loads per lane are asked for at entry beside h and the norm weights, so the chain is ONE memory round trip, the reduction, the
// LDS hand-over of f16(x) and the dot products.  n % 16 == 0, 16 <= n <= kRouteMaxN, 1 <= numExperts <= kRouteMaxExperts (the launcher's caller checks).
constexpr uint32_t kRouteMaxN = 16384, kRouteMaxExperts = 64;
typedef _Float16 route_half2 __attribute__((ext_vector_type(2)));
// One token, block = 1024.  xh [kRouteMaxN] (16-byte aligned): f16(x), padded with zeros to a multiple of 512; red [17]; logit [kRouteMaxExperts].
__device__ __forceinline__ void moe_route_row(const float* __restrict__ h, const uint16_t* __restrict__ w,
                                              const uint16_t* __restrict__ gateW, uint32_t n, uint32_t numExperts,
                                              float* __restrict__ gateOut, uint32_t* __restrict__ idx, float* __restrict__ val,
                                              uint16_t* xh, float* red, float* logit) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t padded = (n + 511u) / 512u * 512u;
    constexpr int K = 4, U = 8;
    // every load that depends on nothing: this wave's first row (8 chunks of 512), the first 4096 of h and of the norm weights
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint16_t*>(gateW), 0, (int)(numExperts * n * 2u), 0x00020000);
    uint32_t w0[U][4];
    {
        const uint32_t rowOff = __builtin_amdgcn_readfirstlane(min(wave, numExperts - 1u) * n * 2u);     // (a wave without a row re-reads the last one)
#pragma unroll
        for (int u = 0; u < U; u++) {
            const uint32_t e = min(u * 512u + lane * 8u, n - 8u);                // clamped, branch-free (n % 16 == 0)
            const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, e * 2u, rowOff, 0);
            w0[u][0] = t[0]; w0[u][1] = t[1]; w0[u][2] = t[2]; w0[u][3] = t[3];
        }
    }
    float x[K], wf[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t i = min(k * 1024u + tid, n - 1u);
        x[k] = h[i];
        wf[k] = half_bits_to_float(w[i]);
    }
    float ss = 0.0f;
#pragma unroll
    for (int k = 0; k < K; k++) ss += k * 1024u + tid < n ? x[k] * x[k] : 0.0f;
    for (uint32_t i = K * 1024u + tid; i < n; i += 1024u) { const float y = h[i]; ss += y * y; }
    const float inv = 1.0f / sqrtf(block_sum(ss, red) / (float)n + 1e-5f);                // aux.metal:150
    // v.asFloat16(), mps.swift:19.  The f32 product is pinned in a register first: left to itself the compiler folds the last multiply and
    // the conversion into ONE v_fma_mixlo_f16, which does not write the bits the GEMV's v_cvt_f16_f32 of the stored f32 value writes
    auto h16 = [](float y) -> uint16_t { asm volatile("" : "+v"(y)); return __half_as_ushort(__float2half_rn(y)); };
#pragma unroll
    for (int k = 0; k < K; k++)
        if (k * 1024u + tid < n) xh[k * 1024u + tid] = h16((x[k] * inv) * wf[k]);
    for (uint32_t i = K * 1024u + tid; i < n; i += 1024u) xh[i] = h16((h[i] * inv) * half_bits_to_float(w[i]));
    for (uint32_t i = n + tid; i < padded; i += 1024u) xh[i] = 0;
    __syncthreads();
    for (uint32_t row = wave; row < numExperts; row += 16u) {                     // (uniform per wave)
        const uint32_t rowOff = __builtin_amdgcn_readfirstlane(row * n * 2u);
        float acc = 0.0f;
        for (uint32_t c0 = 0; c0 < padded; c0 += 512u * U) {
            uint32_t wr[U][4];
            if (row == wave && c0 == 0u) {
#pragma unroll
                for (int u = 0; u < U; u++) { wr[u][0] = w0[u][0]; wr[u][1] = w0[u][1]; wr[u][2] = w0[u][2]; wr[u][3] = w0[u][3]; }
            } else {
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t e = min(c0 + u * 512u + lane * 8u, n - 8u);
                    const auto t = __builtin_amdgcn_raw_buffer_load_b128(rs, e * 2u, rowOff, 0);
                    wr[u][0] = t[0]; wr[u][1] = t[1]; wr[u][2] = t[2]; wr[u][3] = t[3];
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t e = c0 + u * 512u + lane * 8u;
                const bool live = e < n;                                           // a clamped lane holds a copy of another lane's data
                const uint4 xq = *reinterpret_cast<const uint4*>(xh + min(e, padded - 8u));
                const uint32_t xw[4] = {xq.x, xq.y, xq.z, xq.w};
                float a = 0.0f;
#pragma unroll
                for (int p = 0; p < 4; p++) {                                      // exact f16 products, f32 sums
                    const route_half2 wh = __builtin_bit_cast(route_half2, wr[u][p]), xv = __builtin_bit_cast(route_half2, xw[p]);
                    a = fmaf((float)wh[0], (float)xv[0], a);
                    a = fmaf((float)wh[1], (float)xv[1], a);
                }
                acc += live ? a : 0.0f;                                            // (a chunk past n adds 0, as it does in the GEMV)
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
        if (lane == 0) {
            logit[row] = acc;
            if (gateOut) gateOut[row] = acc;
        }
    }
    __syncthreads();
    if (tid == 0) top2_softmax_scan(logit, numExperts, idx, val);
}
__global__ __launch_bounds__(1024) void moe_route_kernel(const float* __restrict__ h, const uint16_t* __restrict__ w,
                                                         const uint16_t* __restrict__ gateW, uint32_t n, uint32_t numExperts,
                                                         float* __restrict__ gateOut, uint32_t* __restrict__ idx, float* __restrict__ val) {
    __shared__ __attribute__((aligned(16))) uint16_t xh[kRouteMaxN];
    __shared__ float red[17];
    __shared__ float logit[kRouteMaxExperts];
    moe_route_row(h, w, gateW, n, numExperts, gateOut, idx, val, xh, red, logit);
}
// grid = rows, block = 1024: row blockIdx.x of h [rows][n], gateOut [rows][numExperts] (may be null), idx and val [rows][2]
__global__ __launch_bounds__(1024) void moe_route_rows_kernel(const float* __restrict__ h, const uint16_t* __restrict__ w,
                                                              const uint16_t* __restrict__ gateW, uint32_t n, uint32_t numExperts,
                                                              float* __restrict__ gateOut, uint32_t* __restrict__ idx, float* __restrict__ val) {
    __shared__ __attribute__((aligned(16))) uint16_t xh[kRouteMaxN];
    __shared__ float red[17];
    __shared__ float logit[kRouteMaxExperts];
    const size_t r = blockIdx.x;
    moe_route_row(h + r * n, w, gateW, n, numExperts, gateOut ? gateOut + r * numExperts : nullptr, idx + 2u * r, val + 2u * r, xh, red, logit);
}

hipError_t launch_top2_softmax(const float* gate, uint32_t n, uint32_t* idx, float* val, hipStream_t st) {
    hipLaunchKernelGGL(top2_softmax_kernel, dim3(1), dim3(64), 0, st, gate, n, idx, val);
    return hipGetLastError();
}
hipError_t launch_mix2(const float* f0, const float* f1, const float* val, float* out, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(mix2_kernel, dim3((n + 255) / 256), dim3(256), 0, st, f0, f1, val, out, n);
    return hipGetLastError();
}
hipError_t launch_mix2_add(float* h, const float* f0, const float* f1, const float* val, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(mix2_add_kernel, dim3((n + 255) / 256), dim3(256), 0, st, h, f0, f1, val, n);
    return hipGetLastError();
}
bool moe_route_supported(uint32_t n, uint32_t numExperts) {
    return n % 16u == 0 && n >= 16u && n <= kRouteMaxN && numExperts >= 1u && numExperts <= kRouteMaxExperts;
}
hipError_t launch_moe_route(const float* h, const uint16_t* w, const uint16_t* gateW, uint32_t n, uint32_t numExperts, float* gateOut,
                            uint32_t* idx, float* val, hipStream_t st) {
    hipLaunchKernelGGL(moe_route_kernel, dim3(1), dim3(1024), 0, st, h, w, gateW, n, numExperts, gateOut, idx, val);
    return hipGetLastError();
}
hipError_t launch_moe_route_rows(const float* h, const uint16_t* w, const uint16_t* gateW, uint32_t n, uint32_t numExperts, float* gateOut,
                                 uint32_t* idx, float* val, uint32_t rows, hipStream_t st) {
    hipLaunchKernelGGL(moe_route_rows_kernel, dim3(rows), dim3(1024), 0, st, h, w, gateW, n, numExperts, gateOut, idx, val);
    return hipGetLastError();
}
hipError_t launch_mix2_add_rows(float* h, const float* f, const float* val, uint32_t n, uint32_t rows, hipStream_t st) {
    hipLaunchKernelGGL(mix2_add_rows_kernel, dim3((n + 255) / 256, rows), dim3(256), 0, st, h, f, val, n);
    return hipGetLastError();
}
hipError_t launch_add_rmsnorm_mul(float* h, const float* delta, const uint16_t* w, float* out, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(add_rmsnorm_mul_kernel, dim3(1), dim3(1024), 0, st, h, delta, w, out, n);
    return hipGetLastError();
}
hipError_t launch_add_rmsnorm_mul_rows(float* h, const float* delta, const uint16_t* w, float* out, uint32_t n, uint32_t rows, hipStream_t st) {
    hipLaunchKernelGGL(add_rmsnorm_mul_rows_kernel, dim3(rows), dim3(1024), 0, st, h, delta, w, out, n);
    return hipGetLastError();
}
hipError_t launch_rope_kv(const float* xq, const float* xk, const float* xv, float* qOut, float* kCache, float* vCache,
                          const uint32_t* pos, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, float ropeBase, uint32_t maxTokens,
                          int* status, hipStream_t st) {
    hipLaunchKernelGGL(rope_kv_kernel, dim3(numHeads), dim3(headDim), 0, st, xq, xk, xv, qOut, kCache, vCache, pos, numHeads,
                       numHeads / numHeadsKV, logf(ropeBase), maxTokens, status);
    return hipGetLastError();
}
hipError_t launch_rope_kv_rows(const float* xq, const float* xk, const float* xv, float* qOut, float* kCache, float* vCache, uint32_t pos0,
                               uint32_t rows, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, float ropeBase, hipStream_t st) {
    hipLaunchKernelGGL(rope_kv_rows_kernel, dim3(numHeads, rows), dim3(headDim), 0, st, xq, xk, xv, qOut, kCache, vCache, pos0, numHeads,
                       numHeads / numHeadsKV, logf(ropeBase));
    return hipGetLastError();
}
hipError_t launch_attention(const float* q, const float* kCache, const float* vCache, const uint32_t* pos, float* out,
                            uint32_t numHeads, uint32_t headDim, uint32_t maxTokens, hipStream_t st) {
    hipLaunchKernelGGL(attention_kernel, dim3(numHeads), dim3(256), maxTokens * sizeof(float), st, q, kCache, vCache, pos, out, numHeads, headDim, maxTokens);
    return hipGetLastError();
}
hipError_t launch_attention_rows(const float* q, const float* kCache, const float* vCache, uint32_t pos0, uint32_t rows, float* out,
                                 uint32_t numHeads, uint32_t headDim, hipStream_t st) {
    hipLaunchKernelGGL(attention_rows_kernel, dim3(numHeads, rows), dim3(256), (pos0 + rows) * sizeof(float), st, q, kCache, vCache, pos0, out,
                       numHeads, headDim);
    return hipGetLastError();
}
hipError_t launch_rope_attention(const float* xq, const float* xk, const float* xv, float* kCache, float* vCache, const uint32_t* pos,
                                 float* out, uint32_t numHeads, uint32_t numHeadsKV, uint32_t headDim, uint32_t maxTokens, float ropeBase,
                                 int* status, hipStream_t st) {
    hipLaunchKernelGGL(rope_attention_kernel, dim3(numHeads), dim3(256), maxTokens * sizeof(float), st, xq, xk, xv, kCache, vCache, pos, out,
                       numHeads, numHeads / numHeadsKV, headDim, maxTokens, logf(ropeBase), status);
    return hipGetLastError();
}
hipError_t launch_silu_mul(const float* x1, const float* x3, float* out, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(silu_mul_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x1, x3, out, n);
    return hipGetLastError();
}
hipError_t launch_fetch_row(const uint16_t* emb, const uint32_t* id, float* out, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(fetch_row_kernel, dim3((n + 255) / 256), dim3(256), 0, st, emb, id, out, n);
    return hipGetLastError();
}
hipError_t launch_fetch_rows(const uint16_t* emb, const uint32_t* ids, float* out, uint32_t n, uint32_t rows, hipStream_t st) {
    hipLaunchKernelGGL(fetch_rows_kernel, dim3((n + 255) / 256, rows), dim3(256), 0, st, emb, ids, out, n);
    return hipGetLastError();
}
hipError_t launch_argmax(const float* logits, uint32_t n, uint32_t* idOut, uint32_t* pos, uint32_t* history, uint32_t historyLen,
                         int* status, hipStream_t st) {
    hipLaunchKernelGGL(argmax_kernel, dim3(1), dim3(1024), 0, st, logits, n, idOut, pos, history, historyLen, status);
    return hipGetLastError();
}

}  // namespace effort
