// What the two prefill attentions on the f16 matrix instruction share on the device: attention_flash16.hip (the plain f16 cache) and
// attention_flash_window.hip (the ring with a window).  The tile geometry, the operand types, the split of an f32 operand into two
// halves and the transposed LDS read.
#pragma once
#include "effort_internal.h"

namespace effort {

constexpr int kFaWaves = 4;
constexpr int kFaTile = 32;                             // keys per tile
constexpr float kFaPScale = 16384.0f;                   // 2^14: the probabilities' pre-scale

typedef float fa_f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 fa_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 fa_f16x4 __attribute__((ext_vector_type(4)));
typedef __fp16 fa_fp16x4 __attribute__((ext_vector_type(4)));

// x ~ hi + lo: hi = f16(x) (round to nearest even), lo = f16(x - hi) (the difference is exact in f32)
__device__ __forceinline__ void fa_split(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}
// four halves [key 0 .. 3][d] of the 16 lanes' addresses, transposed (the lane map is in attention_flash16.hip's header)
__device__ __forceinline__ fa_f16x4 fa_read_tr(const _Float16* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __attribute__((address_space(3))) fa_fp16x4 lds_fp16x4;
    const fa_fp16x4 x = __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4*)(const_cast<_Float16*>(p)));
    return __builtin_bit_cast(fa_f16x4, x);
#else
    return fa_f16x4{};
#endif
}

}  // namespace effort
