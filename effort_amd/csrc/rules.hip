// The generation rules of the decode loop (gfx950): repetition / presence / frequency penalties over the recent tokens, a logit bias
// table, min-p and the stop tokens, in ONE launch of ONE workgroup between the LM head and the pick of a token step.  The specification
// is the comment on effort_logit_rules in include/effort_hip.h (restated in numpy by effort_amd/rules.py: rules_reference); every
// arithmetic step is one rounded f32 operation (the library is built -ffp-contract=off, `/` is the correctly rounded divide).
//
//   record + stop  lane 0: seq[pos] = tok (or status bit 0 past seqLen), the first stop position
//   window         thread j holds the j-th of the <= 1024 recent ids and enters it into an open-addressing hash table in LDS (2048 slots:
//                  at most half full, so every probe sequence ends): an integer atomic add counts the id's occurrences, an atomic minimum
//                  finds its first slot j -- both commute, the result does not depend on the order --; the thread of the first slot
//                  gathers in[id] and patches it.  (All pairs out of LDS, the first form, measured 39.4 us per launch for a full window
//                  of 1024 against 5.9 for an empty one, and 125 with 256 biases looking their ids up in it; the table: 5.2 against
//                  4.8, and 14.0 (these three: profiles/r14_decode_rules.json; the first form's record was not kept).)
//   bias           the <= 256 entries in LDS; the entry with the highest index among equal ids wins (all pairs: 256 compares per
//                  thread), looks its id up in the hash table (a penalised value is its base) and adds
//   copy, patch    out = in, a barrier, the window's patches, a barrier, the bias table's patches (they overwrite the window's)
//   min-p          only when the struct asks: a maximum pass and a threshold pass over out (L2 hits)
// Every patch is computed from `in` before anything is stored, so out == in is the same bits.
#include "effort_internal.h"
#include "../../include/effort_hip.h"

namespace effort {

constexpr int kRulesThreads = 1024, kRulesWaves = kRulesThreads / kWave;
static_assert(EFFORT_RULES_MAX_WINDOW <= kRulesThreads && EFFORT_RULES_MAX_BIAS <= kRulesThreads, "one thread per window slot and per bias entry");
static_assert(sizeof(effort_rules_params) == 64, "the struct the host packs");
constexpr int kRulesBatch = 8;                              // loads of a row pass in flight per thread: 8 x 1024 x 4 bytes = a quarter of 32 000 logits
constexpr uint32_t kNoId = 0xFFFFFFFFu;                     // an id that takes no part: >= n (n < 2^31), or a bias entry with a NaN value
constexpr int kHashBits = 11;
constexpr uint32_t kHashSlots = 1u << kHashBits;
static_assert(kHashSlots >= 2 * EFFORT_RULES_MAX_WINDOW, "the table stays at most half full: a probe always meets an empty slot");
__device__ __forceinline__ uint32_t hash_slot(uint32_t id) { return (id * 2654435761u) >> (32 - kHashBits); }

// One step of the specification on a logit: a NaN logit passes every rule unchanged (its bits kept), and a NaN a rule's arithmetic
// makes (inf - inf) is the canonical quiet NaN -- the bits of an invalid operation's result differ between instruction sets.
__device__ __forceinline__ float keep_nan(float before, float after) {
    if (before != before) return before;
    return after != after ? __uint_as_float(0x7FC00000u) : after;
}

__global__ __launch_bounds__(kRulesThreads) void rules_kernel(const float* in, uint32_t n, const effort_rules_params* __restrict__ params,
                                                              const uint32_t* __restrict__ tokPtr, const uint32_t* __restrict__ posPtr,
                                                              uint32_t* __restrict__ seq, uint32_t seqLen, const uint32_t* __restrict__ biasIds,
                                                              const float* __restrict__ biasVals, uint32_t* __restrict__ stopPos, float* out,
                                                              int* __restrict__ status) {
    __shared__ uint32_t hashKey[kHashSlots], hashCount[kHashSlots], hashFirst[kHashSlots];     // an id of the window, its occurrences, its first slot
    __shared__ float winVal[EFFORT_RULES_MAX_WINDOW];        // the patched logit, at the FIRST window slot of every distinct id
    __shared__ uint32_t biasId[EFFORT_RULES_MAX_BIAS];
    __shared__ float biasVal[EFFORT_RULES_MAX_BIAS];
    __shared__ float waveMax[kRulesWaves];
    const uint32_t tid = threadIdx.x;

    // the settings are device values no host could validate: sanitised here
    float rep = params->repetition_penalty, presence = params->presence_penalty, frequency = params->frequency_penalty;
    if (!(rep > 0.0f) || isinf(rep)) rep = 1.0f;
    if (!isfinite(presence)) presence = 0.0f;
    if (!isfinite(frequency)) frequency = 0.0f;
    const float minPLog = params->min_p_log;
    const bool minP = isfinite(minPLog) && minPLog <= 0.0f;
    const uint32_t lastN = min(params->last_n, (uint32_t)EFFORT_RULES_MAX_WINDOW);
    const uint32_t nBias = biasIds ? min(params->n_bias, (uint32_t)EFFORT_RULES_MAX_BIAS) : 0u;
    const uint32_t pos = posPtr[0];
    const bool recorded = seq != nullptr && pos < seqLen;   // (tok and seq come together: the host's refusal)
    const uint32_t tok = tokPtr ? tokPtr[0] : 0u;
    const uint32_t W = recorded ? min(lastN, pos + 1u) : 0u;

    if (tid == 0 && tokPtr) {
        if (recorded) seq[pos] = tok;
        else atomicOr(status, 1);                            // past the buffer: nothing written, the window empty
        if (stopPos && pos >= params->first_pos && stopPos[0] == kNoId) {
            const uint32_t nStop = min(params->n_stop, (uint32_t)EFFORT_RULES_MAX_STOP);
            bool hit = false;
            for (uint32_t k = 0; k < nStop; k++) hit |= params->stop_ids[k] == tok;
            if (hit) stopPos[0] = pos;
        }
    }

    // the window seq[pos + 1 - W .. pos]; its last id is tok, which lane 0 may not have stored yet
    uint32_t myId = kNoId;
    if (tid < W) {
        myId = tid == W - 1u ? tok : seq[pos + 1u - W + tid];
        if (myId >= n) myId = kNoId;
    }
    if (W > 0)                                               // (uniform)
        for (uint32_t i = tid; i < kHashSlots; i += kRulesThreads) { hashKey[i] = kNoId; hashCount[i] = 0u; hashFirst[i] = kNoId; }
    if (tid < nBias) {
        const uint32_t id = biasIds[tid];
        const float v = biasVals[tid];
        biasId[tid] = (id < n && v == v) ? id : kNoId;
        biasVal[tid] = v;
    }
    __syncthreads();

    uint32_t mySlot = 0;
    if (myId != kNoId) {
        mySlot = hash_slot(myId);
        for (;;) {                                           // (no lane waits for another: a claimed slot is final)
            const uint32_t old = atomicCAS(&hashKey[mySlot], kNoId, myId);
            if (old == kNoId || old == myId) break;
            mySlot = (mySlot + 1u) & (kHashSlots - 1u);
        }
        atomicAdd(&hashCount[mySlot], 1u);
        atomicMin(&hashFirst[mySlot], tid);
    }
    bool biasWins = false;                                   // no later entry names this id
    if (tid < nBias && biasId[tid] != kNoId) {
        biasWins = true;
        for (uint32_t k = tid + 1u; k < nBias; k++) biasWins &= biasId[k] != biasId[tid];
    }
    __syncthreads();
    uint32_t myWin = kNoId;                                  // the id this thread patches for the window, if its slot is the id's first
    if (myId != kNoId && hashFirst[mySlot] == tid) {
        const float l0 = in[myId];
        float l = l0;
        if (rep != 1.0f) l = l > 0.0f ? l / rep : l * rep;
        const float scaled = (float)hashCount[mySlot] * frequency;
        const float sub = scaled + presence;
        winVal[tid] = keep_nan(l0, l - sub);
        myWin = myId;
    }
    __syncthreads();
    float myBias = 0.0f;
    if (biasWins) {
        const uint32_t id = biasId[tid];
        uint32_t first = kNoId;
        if (W > 0)
            for (uint32_t h = hash_slot(id);; h = (h + 1u) & (kHashSlots - 1u)) {
                const uint32_t key = hashKey[h];
                if (key == id) first = hashFirst[h];
                if (key == id || key == kNoId) break;
            }
        const float base = first != kNoId ? winVal[first] : in[id];
        myBias = keep_nan(base, base + biasVal[tid]);
    }

    if (out != in) {
        const float* __restrict__ src = in;                  // (two different rows: the loads of a batch need not wait for its stores)
        float* __restrict__ dst = out;
        for (uint32_t base = tid; base < n; base += kRulesBatch * kRulesThreads) {
            float v[kRulesBatch];
#pragma unroll
            for (int j = 0; j < kRulesBatch; j++) { const uint32_t i = base + j * kRulesThreads; v[j] = i < n ? src[i] : 0.0f; }
#pragma unroll
            for (int j = 0; j < kRulesBatch; j++) { const uint32_t i = base + j * kRulesThreads; if (i < n) dst[i] = v[j]; }
        }
    }
    __syncthreads();                                         // every read of `in` is done (out may be in), the copy is in place
    if (myWin != kNoId) out[myWin] = winVal[tid];
    __syncthreads();
    if (biasWins) out[biasId[tid]] = myBias;
    if (!minP) return;                                       // uniform: read from the struct
    __syncthreads();

    float m = -INFINITY;                                     // the largest non-NaN element
    for (uint32_t base = tid; base < n; base += kRulesBatch * kRulesThreads) {
        float v[kRulesBatch];
#pragma unroll
        for (int j = 0; j < kRulesBatch; j++) { const uint32_t i = base + j * kRulesThreads; v[j] = i < n ? out[i] : -INFINITY; }
#pragma unroll
        for (int j = 0; j < kRulesBatch; j++) if (v[j] > m) m = v[j];
    }
    m = wave_max_f32(m);
    if ((tid & 63u) == 0) waveMax[tid >> 6] = m;
    __syncthreads();
    m = waveMax[0];
#pragma unroll
    for (int w = 1; w < kRulesWaves; w++) m = fmaxf(m, waveMax[w]);
    if (!isfinite(m)) return;                                // +inf, or nothing but NaN and -inf: the rule is skipped
    const float thr = m + minPLog;
    for (uint32_t base = tid; base < n; base += kRulesBatch * kRulesThreads) {
        float v[kRulesBatch];
#pragma unroll
        for (int j = 0; j < kRulesBatch; j++) { const uint32_t i = base + j * kRulesThreads; v[j] = i < n ? out[i] : INFINITY; }
#pragma unroll
        for (int j = 0; j < kRulesBatch; j++) if (v[j] < thr) out[base + j * kRulesThreads] = -INFINITY;      // (false for NaN: it stays)
    }
}

hipError_t launch_rules(const float* in, uint32_t n, const void* params, const uint32_t* tok, const uint32_t* pos, uint32_t* seq, uint32_t seqLen,
                        const uint32_t* biasIds, const float* biasVals, uint32_t* stopPos, float* out, int* status, hipStream_t st) {
    hipLaunchKernelGGL(rules_kernel, dim3(1), dim3(kRulesThreads), 0, st, in, n, static_cast<const effort_rules_params*>(params), tok, pos, seq, seqLen,
                       biasIds, biasVals, stopPos, out, status);
    return hipGetLastError();
}

}  // namespace effort
