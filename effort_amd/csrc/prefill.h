// What the block multiplies of prompt prefill share: prefill.hip (the f16 cores), prefill_buckets.hip (the FP16 bucketed weights,
// un-bucketed on the fly) and prefill_q4.hip (the Q4 buckets, de-quantised on the fly).  All walk K in stages of kPfStage under the
// SAME k split and reduce it with the same kernel, so that a bucket kernel's bits are the core kernel's on the un-bucketed matrix.
// The sequence of launches around the multiply is written here once (pf_block_call); a launcher hands it the launch of its own
// kernel.  Read by glue.hip and the three prefill units alone.
#pragma once
#include <type_traits>

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

// ---- a run-time choice as a compile-time value: f gets a std::integral_constant (with_geom's shape, bucket_mul.hip)
// the token tiles (of 16) that `rows` live columns need: NT = 1 .. 4
template <class F>
hipError_t pf_with_tiles(uint32_t rows, F&& f) {
    switch ((rows + 15u) / 16u) {
        case 1: return f(std::integral_constant<int, 1>{});
        case 2: return f(std::integral_constant<int, 2>{});
        case 3: return f(std::integral_constant<int, 3>{});
        default: return f(std::integral_constant<int, 4>{});
    }
}
// NO when `yes` is false, else YES: AUX (0, or 2 = nt) and VEC (1 dword per load, or 4)
template <int NO, int YES, class F>
hipError_t pf_with_either(bool yes, F&& f) {
    return yes ? f(std::integral_constant<int, YES>{}) : f(std::integral_constant<int, NO>{});
}

// ---- one block call, plain or routed, on cores or buckets
// x f32 [rows][inDim] (routed with xPerSlot: [rows][2][inDim]), out f32 [rows][outDim] (routed: [rows][2][outDim]).  Scratch: xh = halves
// for f16(x), part = dense_gemm_rows_partial_floats floats (routed: ..._routed_partial_floats); routed alone: groups =
// dense_gemm_rows_routed_group_words words (the counts, then the lists), idx2 = the 2 * rows expert numbers.
struct PfCall {
    const float* x;
    uint16_t* xh;
    float* part;
    float* out;
    uint32_t inDim, outDim, rows;
    bool routed = false;
    const uint32_t* idx2 = nullptr;
    uint32_t* groups = nullptr;
    uint32_t numExperts = 0, xPerSlot = 0;
};
// ... and what the multiply's launch is told: dst = out when there is one split, else the partial sums; the routed kernels' operands
struct PfMul {
    float* dst;
    PfSplit sp;
    uint32_t *cnt, *list;
    uint32_t assigns, xRows, xShift;
};
// The sequence of every block call: the prologue (f16(x); routed: and the grouping) -> the k split -> the multiply, mul(AUX, PfMul), into
// `out` or into the partial sums -> with more than one split, their reduction.  The split and the nt rule are judged by (inDim, outDim),
// ONE expert's matrix (what a workgroup's neighbours stream with it), never by rows.
template <class Mul>
hipError_t pf_block_call(const PfCall& c, hipStream_t st, Mul&& mul) {
    if (c.rows < 1u || c.rows > (uint32_t)kPrefillMaxRows) return hipErrorInvalidValue;
    if (c.routed && (c.numExperts < 1u || c.numExperts > kPfMaxExperts || c.xPerSlot > 1u)) return hipErrorInvalidValue;
    const uint32_t assigns = 2u * c.rows, xRows = c.routed && c.xPerSlot ? assigns : c.rows, outRows = c.routed ? assigns : c.rows;
    PfMul m{nullptr, pf_split(c.inDim, c.outDim), c.groups, c.routed ? c.groups + kPfMaxExperts : nullptr, assigns, xRows, c.xPerSlot ? 0u : 1u};
    hipError_t e = c.routed ? launch_routed_prologue(c.x, c.xh, xRows * c.inDim, c.idx2, assigns, c.numExperts, m.cnt, m.list, st)
                            : launch_rows_to_f16(c.x, c.xh, xRows * c.inDim, st);
    if (e != hipSuccess) return e;
    m.dst = m.sp.splits > 1u ? c.part : c.out;
    e = pf_with_either<0, 2>((size_t)c.inDim * c.outDim * 2u > kPfKeepBytes, [&](auto aux) { return mul(aux, m); });
    if (e != hipSuccess || m.sp.splits == 1u) return e;
    return launch_reduce_splits(c.part, c.out, outRows * c.outDim, m.sp.splits, st);
}

// prefill.hip: the block multiply on the f16 cores
bool dense_gemm_rows_supported(uint32_t inDim, uint32_t outDim);
size_t dense_gemm_rows_partial_floats(uint32_t inDim, uint32_t outDim, uint32_t rows);      // scratch for the k splits' partial sums (0: none)
hipError_t launch_dense_gemm_rows(const uint16_t* W_f16, const float* x, uint16_t* xhScratch /* rows * inDim halves */, float* partScratch, float* out,
                                  uint32_t inDim, uint32_t outDim, uint32_t rows, hipStream_t st);
// ... and its routed form: assignment 2 r + s multiplies expert idx2[2 r + s] of a stack (numExperts <= 64)
size_t dense_gemm_rows_routed_partial_floats(uint32_t inDim, uint32_t outDim, uint32_t rows);
size_t dense_gemm_rows_routed_group_words();                                              // scratch for the per-expert counts and assignment lists
hipError_t launch_dense_gemm_rows_routed(const uint16_t* W_f16, uint32_t numExperts, const uint32_t* idx2, const float* x, uint32_t xPerSlot,
                                         uint16_t* xhScratch /* (xPerSlot ? 2 : 1) * rows * inDim halves */, float* partScratch, uint32_t* groupScratch,
                                         float* out, uint32_t inDim, uint32_t outDim, uint32_t rows, hipStream_t st);

// prefill_buckets.hip: the block multiply on the bucketed weights (FP16, percentLoad 16), un-bucketed on the fly; the scratch is the core
// launchers', same sizes.  B is ONE expert's buckets for the plain launcher and the whole stack's for the routed one.
bool bucket_gemm_rows_supported(uint32_t inDim, uint32_t outDim);
hipError_t launch_bucket_dense_check(const uint16_t* B, uint32_t pitch, uint32_t cols, uint32_t inDim, uint32_t numExperts, int* bad, hipStream_t st);
hipError_t launch_bucket_gemm_rows(const uint16_t* B, uint32_t pitch, const float* x, uint16_t* xh, float* part, float* out, uint32_t inDim,
                                   uint32_t outDim, uint32_t rows, hipStream_t st);
hipError_t launch_bucket_gemm_rows_routed(const uint16_t* B, uint32_t pitch, uint32_t numExperts, const uint32_t* idx2, const float* x, uint32_t xPerSlot,
                                          uint16_t* xh, float* part, uint32_t* groups, float* out, uint32_t inDim, uint32_t outDim, uint32_t rows,
                                          hipStream_t st);

// prefill_q4.hip: the block multiply on the Q4 buckets, de-quantised on the fly, plus the handle's outliers; the scratch is the core
// launcher's, same sizes.  B and means16 (the f16 row means launch_q4_dense_check writes) are ONE expert's.
hipError_t launch_q4_dense_check(const uint16_t* B, uint32_t pitch, uint32_t words, const float* stats, uint32_t inDim, uint32_t numExperts,
                                 uint16_t* means16, int* bad, hipStream_t st);
hipError_t launch_q4_gemm_rows(const uint16_t* B, uint32_t pitch, const uint16_t* means16, const OutlierIndex& ol, const float* x, uint16_t* xh, float* part,
                               float* out, uint32_t inDim, uint32_t outDim, uint32_t rows, hipStream_t st);

}  // namespace effort
