// What the two block multiplies of prompt prefill share: prefill.hip (the f16 cores) and prefill_buckets.hip (the bucketed weights,
// un-bucketed on the fly).  Both walk K in stages of kPfStage under the SAME k split and reduce it with the same kernel, so that
// the bucket kernel's bits are the core kernel's on the un-bucketed matrix.
#pragma once
#include "effort_internal.h"

namespace effort {

constexpr int kPrefillMaxRows = 64;       // == EFFORT_PREFILL_MAX_ROWS (glue.hip asserts it)
constexpr uint32_t kPfStage = 256;        // k elements per stage: 8 16-byte weight loads per lane
constexpr size_t kPfKeepBytes = 64u << 20;   // == kGemvKeepBytes (gemv.hip): a larger matrix is streamed nt, for the reason given there
// the routed front ends: kPfMaxAssign = 2 * kPrefillMaxRows entries per expert: duplicates or clamping can give one expert all of them
constexpr uint32_t kPfMaxAssign = 2u * kPrefillMaxRows, kPfMaxExperts = 64;

typedef _Float16 pf_half8 __attribute__((ext_vector_type(8)));
typedef float pf_f32x4 __attribute__((ext_vector_type(4)));

// The k split of a shape: stages per split and the number of splits (a function of the shape alone -- never of rows).
struct PfSplit { uint32_t per, splits; };
PfSplit pf_split(uint32_t inDim, uint32_t outDim);

// The kernels around the multiply (prefill.hip), one launch each:
hipError_t launch_rows_to_f16(const float* x, uint16_t* xh, uint32_t n, hipStream_t st);                              // xh[i] = f16(x[i])
hipError_t launch_reduce_splits(const float* part, float* out, uint32_t n, uint32_t splits, hipStream_t st);        // out[i] = part[0][i] + part[1][i] + ...
// f16(x) and the assignments grouped by expert: cnt [kPfMaxExperts], list [kPfMaxExperts][kPfMaxAssign]
hipError_t launch_routed_prologue(const float* x, uint16_t* xh, uint32_t n, const uint32_t* idx2, uint32_t assigns, uint32_t numExperts, uint32_t* cnt,
                                  uint32_t* list, hipStream_t st);

// prefill_buckets.hip: the block multiply on the bucketed weights (FP16, percentLoad 16), un-bucketed on the fly; the scratch is the core
// launchers', same sizes.  B is ONE expert's buckets for the plain launcher and the whole stack's for the routed one.
bool bucket_gemm_rows_supported(uint32_t inDim, uint32_t outDim);
hipError_t launch_bucket_dense_check(const uint16_t* B, uint32_t pitch, uint32_t cols, uint32_t inDim, uint32_t numExperts, int* bad, hipStream_t st);
hipError_t launch_bucket_gemm_rows(const uint16_t* B, uint32_t pitch, const float* x, uint16_t* xh, float* part, float* out, uint32_t inDim,
                                   uint32_t outDim, uint32_t rows, hipStream_t st);
hipError_t launch_bucket_gemm_rows_routed(const uint16_t* B, uint32_t pitch, uint32_t numExperts, const uint32_t* idx2, const float* x, uint32_t xPerSlot,
                                          uint16_t* xh, float* part, uint32_t* groups, float* out, uint32_t inDim, uint32_t outDim, uint32_t rows,
                                          hipStream_t st);

}  // namespace effort
