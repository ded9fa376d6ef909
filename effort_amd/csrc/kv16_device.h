// What the kernels on the compact f16 KV format share on the device: kv16.hip (row t = token t) and kv_window.hip (row t % ringRows).
// The rope of one vector, the writer of one row of a token, and the 16- / 8-byte loads of a cache row with their widening.
#pragma once
#include "effort_internal.h"

namespace effort {

// One vector x of headDim values roped at pos, block = headDim: rope_kv_row's expression (decode.hip), term for term.
__device__ __forceinline__ float rope_row(const float* __restrict__ x, uint32_t pos, float logBase) {
    const uint32_t d = threadIdx.x, half = blockDim.x / 2;
    const uint32_t j = d % half;
    const float freq = (float)exp((double)logBase * (-(double)j / (double)half));          // Float(freq), model.swift:707
    const float angle = (float)pos * freq;
    const float c = cosf(angle), s = sinf(angle);
    return d < half ? x[d] * c - x[d + half] * s : x[d] * c + x[d - half] * s;
}
// Row `row` of the token at position pos, its K / V stored at cache row `slotRow` (pos itself in kv16.hip, pos % ringRows in
// kv_window.hip); xq, xk, xv and qOut are the token's vectors.
__device__ __forceinline__ void rope_kv_f16_row(const float* __restrict__ xq, const float* __restrict__ xk, const float* __restrict__ xv,
                                                float* __restrict__ qOut, _Float16* __restrict__ kCache, _Float16* __restrict__ vCache,
                                                uint32_t pos, uint32_t slotRow, uint32_t row, uint32_t numHeads, uint32_t numHeadsKV,
                                                float logBase) {
    const uint32_t d = threadIdx.x, headDim = blockDim.x;
    if (row < numHeads) {                              // (uniform)
        qOut[row * headDim + d] = rope_row(xq + row * headDim, pos, logBase);
        return;
    }
    const uint32_t g = row - numHeads;
    float kr = rope_row(xk + g * headDim, pos, logBase);
    asm volatile("" : "+v"(kr));                       // the f32 value first, then ONE conversion: no mixed-precision fold of the two
    const size_t slot = ((size_t)slotRow * numHeadsKV + g) * headDim + d;
    kCache[slot] = (_Float16)kr;                       // v_cvt_f16_f32: round to nearest even, overflow to +-inf
    vCache[slot] = (_Float16)xv[g * headDim + d];
}

// The ring rows of one key tile (kv_window.hip, attention_flash_window.hip): `first` is the tile's first live key, row0 its row (both
// uniform in the wave).
struct ring_tile {
    uint32_t first, last, row0, ringRows;
    // the row of `key` clamped into first .. last; last - first < ringRows
    __device__ __forceinline__ uint32_t row(uint32_t key) const {
        const uint32_t r = row0 + (min(max(key, first), last) - first);
        return r >= ringRows ? r - ringRows : r;
    }
};
__device__ __forceinline__ ring_tile ring_tile_at(uint32_t key0, uint32_t lo, uint32_t last, uint32_t ringRows) {
    const uint32_t first = max(key0, lo);
    return ring_tile{first, last, (uint32_t)__builtin_amdgcn_readfirstlane(first % ringRows), ringRows};   // the ONE division of a tile
}

typedef _Float16 kv_half2 __attribute__((ext_vector_type(2)));

// W 32-bit words (2 W halves) of a cache row in one load: 16 bytes (W = 4) or 8 (W = 2)
template <int W>
__device__ __forceinline__ void kv_load(const _Float16* __restrict__ p, uint32_t (&w)[W]) {
    if constexpr (W == 4) {
        const uint4 t = *reinterpret_cast<const uint4*>(p);
        w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
    } else {
        const uint2 t = *reinterpret_cast<const uint2*>(p);
        w[0] = t.x; w[1] = t.y;
    }
}
template <int W>
__device__ __forceinline__ void kv_widen(const uint32_t (&w)[W], float (&f)[2 * W]) {
#pragma unroll
    for (int i = 0; i < W; i++) {
        const kv_half2 h = __builtin_bit_cast(kv_half2, w[i]);
        f[2 * i] = (float)h[0]; f[2 * i + 1] = (float)h[1];
    }
}

}  // namespace effort
