// What the host and the device share of the split decode attention (attention_split.hip): the limits, the key range of a split and the
// layout of the partial states.  Plain arithmetic, no HIP call: effort_debug_attention_split_range runs the range rule on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#include <hip/hip_runtime.h>
#define EFFORT_HD __host__ __device__
#else
#define EFFORT_HD
#endif

namespace effort {

constexpr uint32_t kSplitTile = 64;          // keys per tile, counted from token 0
constexpr uint32_t kSplitMax = 64;           // splits per call

// The tiles [t0, t1) of split s of S over the nTok live cache rows: tiles of kSplitTile keys from token 0, per = ceil(tiles / S)
// consecutive tiles per split, the last splits possibly empty (t0 == t1).  The ranges are disjoint, ascending and cover every tile.
EFFORT_HD inline void attention_split_tiles(uint32_t nTok, uint32_t S, uint32_t s, uint32_t& t0, uint32_t& t1) {
    const uint32_t nTiles = (nTok + kSplitTile - 1u) / kSplitTile;
    const uint32_t per = (nTiles + S - 1u) / S;
    t0 = s * per < nTiles ? s * per : nTiles;
    t1 = (s + 1u) * per < nTiles ? (s + 1u) * per : nTiles;
}

// The same rule over a WINDOW of keys (kv_window.hip): the query at position pos sees tokens lo .. pos, lo = max(0, pos + 1 - window).
// The tiles stay on absolute multiples of kSplitTile counted from token 0; the live ones are tLo = lo / 64 .. tHi = pos / 64, and split
// s takes per = ceil(live tiles / S) consecutive ones from tLo + s per.  With lo = 0 this is attention_split_tiles(pos + 1, ...).
EFFORT_HD inline uint32_t attention_window_lo(uint32_t pos, uint32_t window) { return pos >= window ? pos - window + 1u : 0u; }
EFFORT_HD inline void attention_window_tiles(uint32_t pos, uint32_t window, uint32_t S, uint32_t s, uint32_t& t0, uint32_t& t1) {
    const uint32_t tLo = attention_window_lo(pos, window) / kSplitTile;
    const uint32_t nTiles = pos / kSplitTile - tLo + 1u;
    const uint32_t per = (nTiles + S - 1u) / S;
    t0 = tLo + (s * per < nTiles ? s * per : nTiles);
    t1 = tLo + ((s + 1u) * per < nTiles ? (s + 1u) * per : nTiles);
}

// The scratch of a call, in floats: acc [numHeads][S][headDim], then (m, l) [numHeads][S][2].
EFFORT_HD inline size_t attention_split_scratch_floats(uint32_t numHeads, uint32_t headDim, uint32_t S) {
    return (size_t)numHeads * S * (headDim + 2u);
}

inline bool attention_split_shape_ok(int numHeads, int numHeadsKV, int headDim) {
    if (numHeads <= 0 || numHeadsKV <= 0 || numHeads % numHeadsKV) return false;
    const int R = numHeads / numHeadsKV;
    return (R == 1 || R == 2 || R == 4 || R == 8) && (headDim == 64 || headDim == 128 || headDim == 256);
}

// What splits = 0 resolves to: one workgroup per CU or a little more (ceil(numCU / numHeadsKV) splits of numHeadsKV workgroups each),
// never more splits than the cache has tiles at maxTokens (a split thinner than a tile is an empty one) and never more than kSplitMax.
inline int attention_split_default(int numCU, int numHeadsKV, int maxTokens) {
    int S = (numCU + numHeadsKV - 1) / numHeadsKV;
    const int tiles = (maxTokens + (int)kSplitTile - 1) / (int)kSplitTile;
    if (S > tiles) S = tiles;
    if (S > (int)kSplitMax) S = (int)kSplitMax;
    return S < 1 ? 1 : S;
}

// The compact f16 cache [maxTokens][numHeadsKV][headDim] (kv16.hip, the *_f16 entry points): the same head geometry, to
// Mistral-7B's max_position_embeddings.
constexpr int kKv16MaxTokens = 32768;
inline bool kv16_shape_ok(int numHeads, int numHeadsKV, int headDim, int maxTokens) {
    return maxTokens >= 1 && maxTokens <= kKv16MaxTokens && attention_split_shape_ok(numHeads, numHeadsKV, headDim);
}

// The rolling cache [ringRows][numHeadsKV][headDim] (kv_window.hip, the *_ring / *_window entry points): token t in row t % ringRows, a
// query sees `window` keys including its own.  A block of `rows` tokens needs window + rows - 1 ring rows (rows = 1: a token step).
constexpr int kWindowMaxPos = 1048576;       // positions stay exact as f32 in the rope
inline bool kv_window_shape_ok(int numHeads, int numHeadsKV, int headDim, int ringRows, int window, int rows) {
    return window >= 1 && window <= ringRows && ringRows <= kKv16MaxTokens && window - 1 <= ringRows - rows &&
           attention_split_shape_ok(numHeads, numHeadsKV, headDim);
}

#if defined(__HIPCC__)
// ---- what the two split kernels (attention_split.hip on the f32 cache, kv16.hip on the f16 one) share on the device
constexpr int kAsWaves = 4;

template <int CTRL>
__device__ __forceinline__ float as_row_shr_add(float x) {
    return x + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xf, 0xf, false));
}
// the sum over the LPK lanes of a key, in the key's LAST lane
template <int LPK>
__device__ __forceinline__ float as_key_sum(float x) {
    x = as_row_shr_add<0x111>(x);
    x = as_row_shr_add<0x112>(x);
    x = as_row_shr_add<0x114>(x);
    if constexpr (LPK >= 16) x = as_row_shr_add<0x118>(x);
    if constexpr (LPK == 32) x += __shfl_xor(x, 16);
    return x;
}
// Orders the wave's LDS writes before its later LDS reads for the compiler (a wave's LDS instructions execute in order).
__device__ __forceinline__ void as_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}
#endif

}  // namespace effort
