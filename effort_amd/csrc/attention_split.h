// What the host and the device share of the split decode attention (attention_split.hip): the limits, the key range of a split and the
// layout of the partial states.  Plain arithmetic, no HIP call: effort_debug_attention_split_range runs the range rule on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
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

}  // namespace effort
