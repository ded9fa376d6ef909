// The sampled pick of the decode loop (gfx950): top-K selection of the logits (the reference's mpsTopK, helpers/mps.swift:49-80) and a
// temperature / top-k / top-p draw over the selected, in ONE launch of ONE workgroup that takes argmax_kernel's place in a token step.
//
//   select_topk   the K <= 64 largest of n f32 logits, sorted by value descending, lowest index first among equal values; NaN is never
//                 selected, -inf is an ordinary value, -0.0 == +0.0.  Not K rounds of argmax: four 8-bit radix passes over an
//                 order-preserving 32-bit key (a 256-bin histogram in LDS per pass, 16 copies of each bin) find the K-th largest key T and how many of the
//                 keys equal to T belong to the result; one more pass compacts the keys above T into LDS; the ties AT T are taken in
//                 index order (a counting pass per wave, then a walk that stops at the last one needed); wave 0 sorts the <= 64
//                 survivors by rank counting.  Every wave owns one contiguous range of indices and reads it coalesced; up to n = 32768 a
//                 lane keeps its 32 logits in registers and memory is read once, beyond that every pass reads the logits again (L2
//                 hits), so n is not bounded by registers or LDS.
//   sample_kernel settings from a 32-byte struct in DEVICE memory (effort_sample_params: a captured graph serves every seed and
//                 temperature), the uniform from Philox4x32-10 keyed by the seed at counter (*pos, stream, 0, 0), then what
//                 argmax_kernel writes: the id, history[pos], pos += 1, the status bits.
#include "effort_internal.h"
#include "sample_device.h"
#include "../../include/effort_hip.h"

namespace effort {

constexpr int kSampleThreads = 1024, kSampleWaves = kSampleThreads / kWave, kSampleMaxK = EFFORT_SAMPLE_MAX_K;
static_assert(kSampleMaxK == kWave, "wave 0 sorts the survivors one per lane");
constexpr int kCacheRegs = 32;                               // logits a lane keeps in registers: n <= 32 * 1024 = 32768 is read from memory ONCE
constexpr int kHistCopies = 16;                              // copies of every histogram bin, by lane & 15: a vocabulary's logits share a handful of
                                                             // leading bytes, and LDS atomics of one instruction on one address run one after the other

struct TopkLds {
    uint32_t hist[256 * kHistCopies];                       // [bin][copy]: the copies of a bin lie in different banks
    uint32_t bins[256];                                     // the copies summed
    uint32_t waveTies[kSampleWaves];
    uint32_t selIdx[kSampleMaxK], selKey[kSampleMaxK];      // the survivors, unordered: [0, above) keys > T, [above, K) the ties at T by index
    uint32_t outIdx[kSampleMaxK];                           // sorted
    float outVal[kSampleMaxK];
    float w[kSampleMaxK];
    uint32_t prefix, need, total, cursor;
};

// f32 -> u32 whose unsigned order is the floats' order; the two zeros share a key.  NaN -> 0, below every other key (-inf is 0x007FFFFF;
// the only bits that would map to 0 are a NaN's): key 0 is "not a candidate", for NaN logits and for slots past the end alike.
__device__ __forceinline__ uint32_t order_key(uint32_t u) {
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
    if (u == 0x80000000u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// f(index, key) over the wave's index range [lo, hi), 64 consecutive indices per step, until f returns false (f's answer is uniform over
// the wave).  CACHED: the keys are in the registers r (slots past hi hold key 0); else from memory, four loads in flight.
template <bool CACHED, typename F>
__device__ __forceinline__ void walk(const float* __restrict__ logits, const uint32_t (&r)[kCacheRegs], uint32_t lo, uint32_t hi, uint32_t lane, F&& f) {
    if constexpr (CACHED) {
#pragma unroll
        for (int it = 0; it < kCacheRegs; it++)
            if (!f(lo + it * 64u + lane, r[it])) return;
    } else {
        for (uint32_t base = lo; base < hi; base += 256u) {
            uint32_t u[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { const uint32_t i = base + j * 64u + lane; u[j] = i < hi ? order_key(__float_as_uint(logits[i])) : 0u; }
#pragma unroll
            for (int j = 0; j < 4; j++)
                if (!f(base + j * 64u + lane, u[j])) return;
        }
    }
}

// Every thread of the workgroup calls it (it holds barriers).  Returns the number selected: min(K, non-NaN logits); s.outIdx / s.outVal
// hold them sorted.  1 <= K <= 64.
template <bool CACHED>
__device__ __forceinline__ uint32_t select_topk_t(const float* __restrict__ logits, uint32_t n, uint32_t K, TopkLds& s) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    // the wave's index range [lo, hi): a multiple of 64 long, so that a wave's load is one aligned run of 64 floats
    const uint32_t perWave = ((n + kSampleWaves - 1) / kSampleWaves + 63u) & ~63u;
    const uint32_t lo = min(wave * perWave, n), hi = min(lo + perWave, n);
    uint32_t r[kCacheRegs];
    if constexpr (CACHED) {                                  // (perWave <= 64 * kCacheRegs: the caller's choice of CACHED)
#pragma unroll
        for (int it = 0; it < kCacheRegs; it++) { const uint32_t i = lo + it * 64u + lane; r[it] = i < hi ? order_key(__float_as_uint(logits[i])) : 0u; }
    }

    if (tid < (uint32_t)kSampleMaxK) s.selIdx[tid] = 0;
    uint32_t prefix = 0, need = K;
#pragma unroll 1
    for (int pass = 0; pass < 4; pass++) {
        const int shift = 24 - 8 * pass;
#pragma unroll
        for (int j = 0; j < 256 * kHistCopies / kSampleThreads; j++) s.hist[j * kSampleThreads + tid] = 0;
        __syncthreads();
        walk<CACHED>(logits, r, lo, hi, lane, [&](uint32_t, uint32_t key) {
            if (key != 0u && ((key >> shift) >> 8) == prefix)                   // (pass 0: shift 24, nothing above the digit, prefix 0)
                atomicAdd(&s.hist[((key >> shift) & 255u) * kHistCopies + (lane & (kHistCopies - 1))], 1u);
            return true;
        });
        __syncthreads();
        if (tid < 256) {
            uint32_t c = 0;
#pragma unroll 4
            for (int k = 0; k < kHistCopies; k++) c += s.hist[tid * kHistCopies + ((k + tid) & (kHistCopies - 1))];
            s.bins[tid] = c;
        }
        __syncthreads();
        if (wave == 0) {
            // bins from the top: lane l holds bins 255 - 4l .. 252 - 4l; the bin where the count from the top reaches `need` is the digit
            uint32_t c[4], sum = 0;
#pragma unroll
            for (int j = 0; j < 4; j++) { c[j] = s.bins[255 - (4 * lane + j)]; sum += c[j]; }
            const uint32_t incl = wave_prefix_sum_u32(sum);
            uint32_t want = need;
            if (pass == 0) {
                const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
                want = min(need, total);
                if (lane == 0) { s.total = total; s.need = 0; s.prefix = 0; }
            }
            uint32_t cum = incl - sum;
            if (want > 0 && cum < want && want <= incl) {           // exactly one lane
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    if (cum < want && want <= cum + c[j]) { s.prefix = (prefix << 8) | (255u - (4 * lane + j)); s.need = want - cum; }
                    cum += c[j];
                }
            }
        }
        __syncthreads();
        prefix = s.prefix; need = s.need;
        if (pass == 0) {
            if (s.total == 0) return 0;                              // every logit NaN (uniform: all threads leave)
            K = min(K, s.total);
        }
    }
    // prefix = T, the K-th largest key; `need` of the keys equal to T are in the result, the lowest indices first; K - need keys are above T
    const uint32_t T = prefix, above = K - need;
    if (tid == 0) s.cursor = 0;
    __syncthreads();
    uint32_t ties = 0;
    walk<CACHED>(logits, r, lo, hi, lane, [&](uint32_t i, uint32_t key) {                 // (T > 0: key 0 is neither above nor a tie)
        if (key > T) { const uint32_t slot = atomicAdd(&s.cursor, 1u); if (slot < (uint32_t)kSampleMaxK) s.selIdx[slot] = i; }
        ties += key == T;
        return true;
    });
    ties = wave_sum_u32(ties);
    if (lane == 0) s.waveTies[wave] = ties;
    __syncthreads();
    uint32_t start = 0;
    for (uint32_t w = 0; w < wave; w++) start += s.waveTies[w];
    if (ties > 0 && start < need) {                                  // uniform per wave: this wave holds some of the ties taken
        uint32_t seen = 0;
        walk<CACHED>(logits, r, lo, hi, lane, [&](uint32_t i, uint32_t key) {
            const bool tie = key == T;
            const unsigned long long m = __ballot(tie);
            const uint32_t rank = start + seen + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (tie && rank < need) s.selIdx[above + rank] = i;
            seen += (uint32_t)__popcll(m);
            return start + seen < need && seen < ties;               // stop at the last tie needed / the wave's last tie
        });
    }
    __syncthreads();
    // wave 0 sorts the K survivors: value descending, index ascending among equal keys
    uint32_t myIdx = 0, myKey = 0; float myVal = 0.0f;
    if (tid < K) {
        myIdx = min(s.selIdx[tid], n - 1u); myVal = logits[myIdx];      // (the clamp: no read depends on the bookkeeping above being right)
        myKey = order_key(__float_as_uint(myVal));
        s.selKey[tid] = myKey;
    }
    __syncthreads();
    if (tid < K) {
        uint32_t rank = 0;
        for (uint32_t m = 0; m < K; m++) {
            const uint32_t km = s.selKey[m], im = s.selIdx[m];
            rank += (km > myKey) || (km == myKey && im < myIdx);
        }
        s.outIdx[rank] = myIdx; s.outVal[rank] = myVal;
    }
    __syncthreads();
    return K;
}
// n <= 32768 (every vocabulary of the reference's models): the logits are read once and every pass runs on registers; beyond, every pass
// reads them again (L2 hits).  Uniform over the workgroup.
__device__ __forceinline__ uint32_t select_topk(const float* __restrict__ logits, uint32_t n, uint32_t K, TopkLds& s) {
    if (n <= (uint32_t)(kCacheRegs * kSampleThreads)) return select_topk_t<true>(logits, n, K, s);
    return select_topk_t<false>(logits, n, K, s);
}

// mpsTopK itself: entries past the number of non-NaN logits get index 0xFFFFFFFF and value -inf.
__global__ __launch_bounds__(kSampleThreads) void topk_kernel(const float* __restrict__ logits, uint32_t n, uint32_t k, uint32_t* __restrict__ idxOut,
                                                              float* __restrict__ valOut) {
    __shared__ TopkLds s;
    const uint32_t cnt = select_topk(logits, n, min(k, n), s);
    if (threadIdx.x < k) {
        idxOut[threadIdx.x] = threadIdx.x < cnt ? s.outIdx[threadIdx.x] : 0xFFFFFFFFu;
        valOut[threadIdx.x] = threadIdx.x < cnt ? s.outVal[threadIdx.x] : -INFINITY;
    }
}

__global__ __launch_bounds__(kSampleThreads) void sample_kernel(const float* __restrict__ logits, uint32_t n, const effort_sample_params* __restrict__ params,
                                                                uint32_t* __restrict__ idOut, uint32_t* __restrict__ posPtr, uint32_t* __restrict__ history,
                                                                uint32_t historyLen, int* __restrict__ status, uint32_t* __restrict__ topkIdx,
                                                                float* __restrict__ topkVal) {
    __shared__ TopkLds s;
    // the settings are device values no host could validate: sanitised here
    const uint32_t K = min(max(params->top_k, 1u), min((uint32_t)kSampleMaxK, n));
    const float temperature = params->temperature;
    float topP = params->top_p;
    if (!(topP > 0.0f && topP <= 1.0f)) topP = 1.0f;
    const bool greedy = !(temperature > 0.0f) || isinf(temperature);

    const uint32_t cnt = select_topk(logits, n, K, s);
    const uint32_t tid = threadIdx.x;
    if (tid < K) {
        if (topkIdx) topkIdx[tid] = tid < cnt ? s.outIdx[tid] : 0xFFFFFFFFu;
        if (topkVal) topkVal[tid] = tid < cnt ? s.outVal[tid] : -INFINITY;
    }
    const bool draw = cnt > 1 && !greedy && !isinf(s.outVal[0]);    // (an infinite largest logit, of either sign: rank 0)
    if (draw && tid < cnt) s.w[tid] = expf((s.outVal[tid] - s.outVal[0]) / temperature);
    __syncthreads();
    if (tid == 0) {
        const uint32_t pos = posPtr[0];
        uint32_t idx;
        if (cnt == 0) { idx = 0; atomicOr(status, 2); }              // every logit NaN: token 0, as argmax_kernel
        else if (!draw) idx = s.outIdx[0];
        else {
            // one lane, f32, in rank order: the order is part of the specification
            float c = 0.0f;
            for (uint32_t j = 0; j < cnt; j++) { c += s.w[j]; s.w[j] = c; }
            const float thr = topP * c;
            uint32_t last = cnt - 1;
            for (uint32_t j = 0; j < cnt; j++) if (s.w[j] >= thr) { last = j; break; }      // the nucleus: ranks 0 .. last
            const float S = s.w[last];
            const float u = (float)(philox_x0(params->seed_lo, params->seed_hi, params->stream, pos) >> 8) * 0x1p-24f;
            const float t = u * S;
            uint32_t pick = last;
            for (uint32_t j = 0; j < last; j++) if (s.w[j] > t) { pick = j; break; }
            idx = s.outIdx[pick];
        }
        idOut[0] = idx;
        if (history) {
            if (pos < historyLen) history[pos] = idx;
            else atomicOr(status, 1);                                 // past the history buffer: not written
        }
        posPtr[0] = pos + 1u;
    }
}

hipError_t launch_topk(const float* logits, uint32_t n, uint32_t k, uint32_t* idx, float* val, hipStream_t st) {
    hipLaunchKernelGGL(topk_kernel, dim3(1), dim3(kSampleThreads), 0, st, logits, n, k, idx, val);
    return hipGetLastError();
}

hipError_t launch_sample(const float* logits, uint32_t n, const void* params, uint32_t* idOut, uint32_t* pos, uint32_t* history, uint32_t historyLen,
                         int* status, uint32_t* topkIdx, float* topkVal, hipStream_t st) {
    hipLaunchKernelGGL(sample_kernel, dim3(1), dim3(kSampleThreads), 0, st, logits, n, static_cast<const effort_sample_params*>(params), idOut, pos,
                       history, historyLen, status, topkIdx, topkVal);
    return hipGetLastError();
}

}  // namespace effort
