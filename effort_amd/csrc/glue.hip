// Everything around the multiply that is one kernel per call on the context's stream: the dense baseline (the only unit that sees
// rocblas.h), both converters, cosine, the decode-loop glue, the prompt-prefill block calls, sampling and the two status words.
#include <rocblas/rocblas.h>

#include "host.h"
#include "prefill.h"
#include "sample_device.h"

using namespace effort;

// ---- dense baseline ------------------------------------------------------------------------------
extern "C" int effort_set_dense_backend(effort_ctx* c, int rocblas) {
    if (!c) return EFFORT_ERR_ARG;
    c->denseRocblas = rocblas != 0;
    return EFFORT_OK;
}
void dense_release(effort_ctx* c) { if (c->blas) rocblas_destroy_handle(c->blas); c->blas = nullptr; }
void dense_set_stream(effort_ctx* c) { if (c->blas) rocblas_set_stream(c->blas, c->stream); }
extern "C" int effort_dense_gemv(effort_ctx* c, const void* W, const float* v, float* out, int inDim, int outDim) {
    if (!c || !W || !v || !out || inDim <= 0 || outDim <= 0) return fail(c, EFFORT_ERR_ARG, "dense_gemv: bad argument");
    JOIN_TRY(c);
    if (inDim % 16) return fail(c, EFFORT_ERR_SHAPE, "dense_gemv: inDim % 16 != 0 (helpers/mps.swift:18)");
    if (!c->denseRocblas && dense_gemv_supported((uint32_t)inDim, (uint32_t)outDim)) {
        HIP_TRY(c, launch_dense_gemv(static_cast<const uint16_t*>(W), v, out, (uint32_t)inDim, (uint32_t)outDim, c->stream));
        return EFFORT_OK;
    }
    if (!c->blas) {
        if (rocblas_create_handle(&c->blas) != rocblas_status_success) return fail(c, EFFORT_ERR_BLAS, "rocblas_create_handle");
        rocblas_set_stream(c->blas, c->stream);
        rocblas_set_pointer_mode(c->blas, rocblas_pointer_mode_host);
    }
    OK_TRY(c->d_vhalf.grow(c, (size_t)inDim, (size_t)inDim));
    HIP_TRY(c, launch_f32_to_f16(v, c->d_vhalf.buf, inDim, c->stream));              // v.asFloat16(), mps.swift:19
    // W is [outDim][inDim] row-major == column-major inDim x outDim with lda = inDim: y = A^T x
    const float alpha = 1.0f, beta = 0.0f;
    rocblas_status s = rocblas_hssgemv_strided_batched(c->blas, rocblas_operation_transpose, inDim, outDim, &alpha,
                                                       static_cast<const rocblas_half*>(W), inDim, 0,
                                                       reinterpret_cast<const rocblas_half*>(c->d_vhalf.buf), 1, 0, &beta, out, 1, 0, 1);
    if (s != rocblas_status_success) return fail(c, EFFORT_ERR_BLAS, "rocblas_hssgemv_strided_batched");
    return EFFORT_OK;
}
// basicMul on expert *expNo of a stack of cores: always the in-tree kernel (rocBLAS takes its matrix from the host side)
extern "C" int effort_dense_gemv_expert(effort_ctx* c, const void* W, const uint32_t* expNo, const float* v, float* out, int inDim, int outDim,
                                        int numExperts) {
    if (!c || !W || !expNo || !v || !out || inDim <= 0 || outDim <= 0 || numExperts <= 0) return fail(c, EFFORT_ERR_ARG, "dense_gemv_expert: bad argument");
    JOIN_TRY(c);
    if (!dense_gemv_supported((uint32_t)inDim, (uint32_t)outDim) || (size_t)numExperts * outDim * inDim * 2 > 0xFFFFFFFFull)
        return fail(c, EFFORT_ERR_SHAPE, "dense_gemv_expert: inDim % 16 != 0, inDim > 65536, or a stack of 4 GiB or more");
    return HIP_RC(c, launch_dense_gemv_expert(static_cast<const uint16_t*>(W), expNo, v, out, (uint32_t)inDim, (uint32_t)outDim, (uint32_t)numExperts, c->stream));
}

// ---- converter -----------------------------------------------------------------------------------
extern "C" int effort_convert_fp16_pitched(effort_ctx* c, const void* W, int outDim, int inDim, void* buckets, int rowPitchBytes, void* stats, void* probes) {
    if (!c || !W || !buckets || !stats || !probes) return fail(c, EFFORT_ERR_ARG, "convert_fp16: null argument");
    JOIN_TRY(c);
    // convert.swift:210-215,239 + the 16384-wide limit of the multiply (bucketMul.swift:52)
    if (outDim <= 0 || inDim < kProbes || !(outDim >= kProbes || kProbes % outDim == 0) || outDim > 16384 || inDim > 32000 ||
        outDim % 16 || (outDim / 16) % 4)
        return fail(c, EFFORT_ERR_CONVERT, "convert_fp16: bucketize preconditions violated");
    const int pitch = rowPitchBytes ? rowPitchBytes : outDim / 16 * 2;
    if (pitch < outDim / 16 * 2 || pitch % 8) return fail(c, EFFORT_ERR_CONVERT, "convert_fp16: row pitch must be a multiple of 8 bytes >= 2*cols");   // (the stats pass loads 8 bytes at a time)
    const size_t elems = (size_t)outDim * inDim;
    OK_TRY(c->d_convVals.grow(c, elems, elems));
    return HIP_RC(c, launch_convert_fp16(static_cast<const uint16_t*>(W), outDim, inDim, static_cast<uint16_t*>(buckets), (uint32_t)pitch / 2u,
                                   static_cast<uint16_t*>(stats), static_cast<uint16_t*>(probes), c->d_convVals.buf, c->d_status, c->stream));
}
extern "C" int effort_convert_fp16(effort_ctx* c, const void* W, int outDim, int inDim, void* buckets, void* stats, void* probes) {
    return effort_convert_fp16_pitched(c, W, outDim, inDim, buckets, 0, stats, probes);
}

// q4_draft.convert (q4_draft.py:70-322) on the GPU: core2 = W.T, f16 [inDim][outDim].
extern "C" int64_t effort_q4_outlier_count(int inDim, int outDim, double perc) {
    if (inDim <= 0 || outDim <= 0 || !(perc >= 0.0 && perc <= 1.0)) return EFFORT_ERR_ARG;
    return (int64_t)((double)((int64_t)inDim * outDim) * perc);           // int(len(flat) * perc), q4_draft.py:76
}
extern "C" int effort_convert_q4(effort_ctx* c, const void* core2, int inDim, int outDim, double perc, void* buckets, void* stats, void* probes,
                                 void* outliers) {
    if (!c || !core2 || !buckets || !stats || !probes) return fail(c, EFFORT_ERR_ARG, "convert_q4: null argument");
    JOIN_TRY(c);
    if (inDim <= 0 || outDim <= 0 || outDim % 32 || (int64_t)inDim * outDim >= (1ll << 32) || !(perc >= 0.0 && perc <= 1.0))
        return fail(c, EFFORT_ERR_CONVERT, "convert_q4: outDim % 32 != 0 (q4_draft.py:299), or a matrix of 2^32 elements or more");
    const int64_t cnt = effort_q4_outlier_count(inDim, outDim, perc);
    if (cnt >= (1ll << 31)) return fail(c, EFFORT_ERR_CONVERT, "convert_q4: 2^31 outliers or more (the candidate sort counts in int)");
    if (cnt > 0 && !outliers) return fail(c, EFFORT_ERR_ARG, "convert_q4: outliers buffer missing");
    hipSetDevice(c->device);
    return HIP_RC(c, launch_convert_q4(static_cast<const uint16_t*>(core2), (uint32_t)inDim, (uint32_t)outDim, (uint32_t)cnt, static_cast<uint16_t*>(buckets),
                                 static_cast<float*>(stats), static_cast<uint16_t*>(probes), static_cast<float*>(outliers), c->env.numCU, c->stream));
}

extern "C" int effort_cosine(effort_ctx* c, const float* a, const float* b, int n, float* host_out) {
    if (!c || !a || !b || !host_out || n <= 0) return EFFORT_ERR_ARG;
    JOIN_TRY(c);
    HIP_TRY(c, launch_cosine(a, b, n, c->d_cos, c->stream));
    HIP_TRY(c, hipMemcpyAsync(host_out, c->d_cos, 4, hipMemcpyDeviceToHost, c->stream));
    return HIP_RC(c, hipStreamSynchronize(c->stream));
}

// ---- decode-loop glue (runNetwork.swift:68-316; kernels in decode.hip) ---------------------------------------
extern "C" int effort_add_rmsnorm_mul(effort_ctx* c, float* h, const float* delta, const void* w, float* out, int n) {
    if (!c || !h || !w || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "add_rmsnorm_mul: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_add_rmsnorm_mul(h, delta, static_cast<const uint16_t*>(w), out, (uint32_t)n, c->stream));
}
extern "C" int effort_rope_kv(effort_ctx* c, const float* xq, const float* xk, const float* xv, float* qOut, float* kCache,
                              float* vCache, const uint32_t* pos, int numHeads, int numHeadsKV, int headDim, int maxTokens, float ropeBase) {
    if (!c || !xq || !xk || !xv || !qOut || !kCache || !vCache || !pos) return fail(c, EFFORT_ERR_ARG, "rope_kv: null argument");
    JOIN_TRY(c);
    if (numHeads <= 0 || numHeadsKV <= 0 || numHeads % numHeadsKV || headDim < 2 || headDim > 1024 || headDim % 2 || !(ropeBase > 1.0f) || maxTokens <= 0)
        return fail(c, EFFORT_ERR_SHAPE, "rope_kv: bad head geometry");
    return HIP_RC(c, launch_rope_kv(xq, xk, xv, qOut, kCache, vCache, pos, numHeads, numHeadsKV, headDim, ropeBase, (uint32_t)maxTokens, c->d_status + 1, c->stream));
}
extern "C" int effort_attention(effort_ctx* c, const float* q, const float* kCache, const float* vCache, const uint32_t* pos,
                                float* out, int numHeads, int headDim, int maxTokens) {
    if (!c || !q || !kCache || !vCache || !pos || !out) return fail(c, EFFORT_ERR_ARG, "attention: null argument");
    JOIN_TRY(c);
    if (numHeads <= 0 || maxTokens <= 0 || maxTokens > 8192 || (headDim != 64 && headDim != 128 && headDim != 256))
        return fail(c, EFFORT_ERR_SHAPE, "attention: headDim 64/128/256, maxTokens <= 8192");
    return HIP_RC(c, launch_attention(q, kCache, vCache, pos, out, numHeads, headDim, maxTokens, c->stream));
}
extern "C" int effort_rope_attention(effort_ctx* c, const float* xq, const float* xk, const float* xv, float* kCache, float* vCache,
                                     const uint32_t* pos, float* out, int numHeads, int numHeadsKV, int headDim, int maxTokens, float ropeBase) {
    if (!c || !xq || !xk || !xv || !kCache || !vCache || !pos || !out) return fail(c, EFFORT_ERR_ARG, "rope_attention: null argument");
    JOIN_TRY(c);
    if (numHeads <= 0 || numHeadsKV <= 0 || numHeads % numHeadsKV || maxTokens <= 0 || maxTokens > 8192 || !(ropeBase > 1.0f) ||
        (headDim != 64 && headDim != 128 && headDim != 256))
        return fail(c, EFFORT_ERR_SHAPE, "rope_attention: headDim 64/128/256, maxTokens <= 8192");
    return HIP_RC(c, launch_rope_attention(xq, xk, xv, kCache, vCache, pos, out, numHeads, numHeadsKV, headDim, maxTokens, ropeBase, c->d_status + 1, c->stream));
}
extern "C" int effort_silu_mul(effort_ctx* c, const float* x1, const float* x3, float* out, int n) {
    if (!c || !x1 || !x3 || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "silu_mul: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_silu_mul(x1, x3, out, (uint32_t)n, c->stream));
}
extern "C" int effort_fetch_row(effort_ctx* c, const void* emb, const uint32_t* id, float* out, int n) {
    if (!c || !emb || !id || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "fetch_row: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_fetch_row(static_cast<const uint16_t*>(emb), id, out, (uint32_t)n, c->stream));
}
// ---- prompt prefill (the block multiply in prefill.hip, the block glue in decode.hip): a block of tokens per call.  pos0 and rows are
// HOST values (prefill is eager, never captured), so every refusal is a return code with nothing enqueued; the values are judged before
// the pointers, the lanes are joined before the launch.
static_assert(EFFORT_PREFILL_MAX_ROWS == 64, "prefill.hip: kPrefillMaxRows, four token tiles of 16");
static bool prefill_rows_ok(int rows) { return rows >= 1 && rows <= EFFORT_PREFILL_MAX_ROWS; }
// The scratch of a block multiply, on cores or buckets (both are eager on the context's stream, neither outlives its launches' reads),
// grown to a full block's worth whatever rows and xPerSlot are: the next, longer block and the w1, w3 and w2 calls of a layer do not
// allocate again.  A routed call has its OWN set (host.h: captured addresses).
static int grow_block_scratch(effort_ctx* c, uint32_t inDim, uint32_t outDim, int rows, bool routed, int xPerSlot = 0) {
    if (!routed) {
        OK_TRY(c->d_xhRows.grow(c, (size_t)rows * inDim, (size_t)EFFORT_PREFILL_MAX_ROWS * inDim));
        return c->d_gemmPart.grow(c, dense_gemm_rows_partial_floats(inDim, outDim, (uint32_t)rows),
                                  dense_gemm_rows_partial_floats(inDim, outDim, EFFORT_PREFILL_MAX_ROWS));
    }
    OK_TRY(c->d_xhRouted.grow(c, (size_t)(xPerSlot ? 2 : 1) * rows * inDim, (size_t)2 * EFFORT_PREFILL_MAX_ROWS * inDim));
    OK_TRY(c->d_routedPart.grow(c, dense_gemm_rows_routed_partial_floats(inDim, outDim, (uint32_t)rows),
                                dense_gemm_rows_routed_partial_floats(inDim, outDim, EFFORT_PREFILL_MAX_ROWS)));
    return c->d_routedGroups.grow(c, dense_gemm_rows_routed_group_words(), dense_gemm_rows_routed_group_words());
}
extern "C" int effort_dense_gemm_rows(effort_ctx* c, const void* W, const float* x, float* out, int inDim, int outDim, int rows) {
    if (inDim <= 0 || outDim <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows: inDim, outDim >= 1, 1 <= rows <= 64");
    if (!dense_gemm_rows_supported((uint32_t)inDim, (uint32_t)outDim))
        return fail(c, EFFORT_ERR_SHAPE, "dense_gemm_rows: inDim % 32 == 0, inDim <= 65536, outDim <= 2^24, W below 4 GiB");
    if (!c || !W || !x || !out) return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows: null argument");
    JOIN_TRY(c);
    OK_TRY(grow_block_scratch(c, (uint32_t)inDim, (uint32_t)outDim, rows, false));
    return HIP_RC(c, launch_dense_gemm_rows(static_cast<const uint16_t*>(W), x, c->d_xhRows.buf, c->d_gemmPart.buf, out, (uint32_t)inDim, (uint32_t)outDim,
                                      (uint32_t)rows, c->stream));
}
extern "C" int effort_dense_gemm_rows_routed(effort_ctx* c, const void* W, int numExperts, const uint32_t* idx2, const float* x, int xPerSlot, float* out,
                                             int inDim, int outDim, int rows) {
    if (inDim <= 0 || outDim <= 0 || numExperts <= 0 || !prefill_rows_ok(rows) || (xPerSlot != 0 && xPerSlot != 1))
        return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows_routed: inDim, outDim, numExperts >= 1, 1 <= rows <= 64, xPerSlot 0 / 1");
    if (!dense_gemm_rows_supported((uint32_t)inDim, (uint32_t)outDim) || numExperts > 64)
        return fail(c, EFFORT_ERR_SHAPE, "dense_gemm_rows_routed: inDim % 32 == 0, inDim <= 65536, outDim <= 2^24, one expert below 4 GiB, numExperts <= 64");
    if (!c || !W || !idx2 || !x || !out) return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows_routed: null argument");
    JOIN_TRY(c);
    OK_TRY(grow_block_scratch(c, (uint32_t)inDim, (uint32_t)outDim, rows, true, xPerSlot));
    return HIP_RC(c, launch_dense_gemm_rows_routed(static_cast<const uint16_t*>(W), (uint32_t)numExperts, idx2, x, (uint32_t)xPerSlot, c->d_xhRouted.buf,
                                             c->d_routedPart.buf, c->d_routedGroups.buf, out, (uint32_t)inDim, (uint32_t)outDim, (uint32_t)rows, c->stream));
}
// ---- the block multiplies on the bucketed weights (prefill_buckets.hip): no f16 core is read.
// What a handle must be before it is looked at: FP16 (else EFFORT_ERR_KIND), percentLoad 16, no column shard, inDim % 32 == 0.
static int bucket_handle_shape(const effort_w* w, const char* name) {
    char what[128];
    if (w->fmt != kFp16) { snprintf(what, sizeof(what), "%s: an FP16 bundle (Q4 buckets hold no whole matrix)", name); return fail(w->ctx, EFFORT_ERR_KIND, what); }
    if (w->rowsPerIn != 16u || w->view || w->inDim % 32u || !bucket_gemm_rows_supported(w->inDim, w->outDim)) {
        snprintf(what, sizeof(what), "%s: percentLoad 16, a full handle (no column shard), inDim %% 32 == 0", name);
        return fail(w->ctx, EFFORT_ERR_SHAPE, what);
    }
    return EFFORT_OK;
}
// The handle's answer to "un-bucketable?", computed on first use (one kernel over the buckets; synchronises) and kept until a refresh.
static int bucket_dense_state(const effort_w* w, int* ok) {
    effort_ctx* c = w->ctx;
    if (w->bucketDense < 0) {
        int bad = 0;
        hipSetDevice(c->device);
        JOIN_TRY(c);
        HIP_TRY(c, hipMemsetAsync(c->d_status + 2, 0, 4, c->stream));
        HIP_TRY(c, launch_bucket_dense_check(w->buckets, w->rowPitch, w->cols, w->inDim, w->numExperts, c->d_status + 2, c->stream));
        HIP_TRY(c, hipMemcpyAsync(&bad, c->d_status + 2, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        w->bucketDense = bad ? 0 : 1;
    }
    *ok = w->bucketDense;
    return EFFORT_OK;
}
extern "C" int effort_weights_bucket_dense_ok(effort_w* w, int* host_out) {
    if (!w || !w->ctx || w->dead || !host_out) return EFFORT_ERR_ARG;
    OK_TRY(bucket_handle_shape(w, "weights_bucket_dense_ok"));
    return bucket_dense_state(w, host_out);
}
static int bucket_refuse_collisions(effort_ctx* c, const effort_w* w, const char* name) {
    int ok = 0;
    OK_TRY(bucket_dense_state(w, &ok));
    if (ok) return EFFORT_OK;
    char what[160];
    snprintf(what, sizeof(what), "%s: the bundle is not un-bucketable (two entries of one bucket name the same output: effort_convert_status reported drops)", name);
    return fail(c, EFFORT_ERR_CONVERT, what);
}
extern "C" int effort_bucket_gemm_rows(effort_ctx* c, const effort_w* w, int expert, const float* x, float* out, int rows) {
    if (!w || w->dead) return fail(c, EFFORT_ERR_ARG, "bucket_gemm_rows: null handle");
    if (!prefill_rows_ok(rows) || expert < 0 || (uint32_t)expert >= w->numExperts) return fail(c, EFFORT_ERR_ARG, "bucket_gemm_rows: 1 <= rows <= 64, 0 <= expert < numExperts");
    OK_TRY(bucket_handle_shape(w, "bucket_gemm_rows"));
    if (!c || c != w->ctx || !x || !out) return fail(c, EFFORT_ERR_ARG, "bucket_gemm_rows: null argument (or a handle of another context)");
    JOIN_TRY(c);
    OK_TRY(bucket_refuse_collisions(c, w, "bucket_gemm_rows"));
    OK_TRY(grow_block_scratch(c, w->inDim, w->outDim, rows, false));
    const uint16_t* B = reinterpret_cast<const uint16_t*>(reinterpret_cast<const unsigned char*>(w->buckets) + (size_t)expert * 16u * w->inDim * w->rowPitch);
    return HIP_RC(c, launch_bucket_gemm_rows(B, w->rowPitch, x, c->d_xhRows.buf, c->d_gemmPart.buf, out, w->inDim, w->outDim, (uint32_t)rows, c->stream));
}
extern "C" int effort_bucket_gemm_rows_routed(effort_ctx* c, const effort_w* w, const uint32_t* idx2, const float* x, int xPerSlot, float* out, int rows) {
    if (!w || w->dead) return fail(c, EFFORT_ERR_ARG, "bucket_gemm_rows_routed: null handle");
    if (!prefill_rows_ok(rows) || (xPerSlot != 0 && xPerSlot != 1)) return fail(c, EFFORT_ERR_ARG, "bucket_gemm_rows_routed: 1 <= rows <= 64, xPerSlot 0 / 1");
    OK_TRY(bucket_handle_shape(w, "bucket_gemm_rows_routed"));
    if (w->numExperts > 64u) return fail(c, EFFORT_ERR_SHAPE, "bucket_gemm_rows_routed: numExperts <= 64");
    if (!c || c != w->ctx || !idx2 || !x || !out) return fail(c, EFFORT_ERR_ARG, "bucket_gemm_rows_routed: null argument (or a handle of another context)");
    JOIN_TRY(c);
    OK_TRY(bucket_refuse_collisions(c, w, "bucket_gemm_rows_routed"));
    OK_TRY(grow_block_scratch(c, w->inDim, w->outDim, rows, true, xPerSlot));
    return HIP_RC(c, launch_bucket_gemm_rows_routed(w->buckets, w->rowPitch, w->numExperts, idx2, x, (uint32_t)xPerSlot, c->d_xhRouted.buf, c->d_routedPart.buf,
                                              c->d_routedGroups.buf, out, w->inDim, w->outDim, (uint32_t)rows, c->stream));
}
// ---- the block multiply on the Q4 buckets (prefill_q4.hip): the twins of the two plain entry points above, same refusal order, same scratch.
// What a handle must be before it is looked at: Q4 (else EFFORT_ERR_KIND), no column shard, inDim % 32 == 0, a shape the core kernel serves.
static int q4_handle_shape(const effort_w* w, const char* name) {
    char what[128];
    if (w->fmt != kQ4) { snprintf(what, sizeof(what), "%s: a Q4 bundle (FP16 buckets go through effort_bucket_gemm_rows)", name); return fail(w->ctx, EFFORT_ERR_KIND, what); }
    if (w->view || w->inDim % 32u || !dense_gemm_rows_supported(w->inDim, w->outDim)) {
        snprintf(what, sizeof(what), "%s: a full handle (no column shard), inDim %% 32 == 0", name);
        return fail(w->ctx, EFFORT_ERR_SHAPE, what);
    }
    return EFFORT_OK;
}
// The handle's answer to "un-bucketable?", computed on first use (one kernel over the buckets and the stats, which also writes the
// compact f16 means the multiply reads; synchronises) and kept until a refresh.  The means are (re)written IN PLACE.
static int q4_dense_state(const effort_w* w, int* ok) {
    effort_ctx* c = w->ctx;
    if (w->q4Dense < 0) {
        int bad[2] = {0, 0};
        hipSetDevice(c->device);
        JOIN_TRY(c);
        if (!w->q4Means16) HIP_TRY(c, hipMalloc(&w->q4Means16, (size_t)w->numExperts * 8u * w->inDim * 2u));
        HIP_TRY(c, hipMemsetAsync(c->d_status + 2, 0, 8, c->stream));
        HIP_TRY(c, launch_q4_dense_check(w->buckets, w->rowPitch, w->cols, static_cast<const float*>(w->stats), w->inDim, w->numExperts, w->q4Means16,
                                         c->d_status + 2, c->stream));
        HIP_TRY(c, hipMemcpyAsync(bad, c->d_status + 2, 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        w->q4Dense = bad[0] || bad[1] ? 0 : 1;
    }
    *ok = w->q4Dense;
    return EFFORT_OK;
}
extern "C" int effort_weights_q4_dense_ok(effort_w* w, int* host_out) {
    if (!w || !w->ctx || w->dead || !host_out) return EFFORT_ERR_ARG;
    OK_TRY(q4_handle_shape(w, "weights_q4_dense_ok"));
    return q4_dense_state(w, host_out);
}
extern "C" int effort_q4_gemm_rows(effort_ctx* c, const effort_w* w, int expert, const float* x, float* out, int rows) {
    if (!w || w->dead) return fail(c, EFFORT_ERR_ARG, "q4_gemm_rows: null handle");
    if (!prefill_rows_ok(rows) || expert < 0 || (uint32_t)expert >= w->numExperts) return fail(c, EFFORT_ERR_ARG, "q4_gemm_rows: 1 <= rows <= 64, 0 <= expert < numExperts");
    OK_TRY(q4_handle_shape(w, "q4_gemm_rows"));
    if (!c || c != w->ctx || !x || !out) return fail(c, EFFORT_ERR_ARG, "q4_gemm_rows: null argument (or a handle of another context)");
    JOIN_TRY(c);
    int ok = 0;
    OK_TRY(q4_dense_state(w, &ok));
    if (!ok) return fail(c, EFFORT_ERR_CONVERT, "q4_gemm_rows: the bundle is not un-bucketable (the ranks of a bucket do not name eight different outputs, or a row mean is no finite f16 number)");
    OK_TRY(grow_block_scratch(c, w->inDim, w->outDim, rows, false));
    const size_t row0 = (size_t)expert * 8u * w->inDim;
    const uint16_t* B = reinterpret_cast<const uint16_t*>(reinterpret_cast<const unsigned char*>(w->buckets) + row0 * w->rowPitch);
    return HIP_RC(c, launch_q4_gemm_rows(B, w->rowPitch, w->q4Means16 + row0, OutlierIndex{w->olBlockPtr, w->olEntry, w->olMeta}, x, c->d_xhRows.buf,
                                         c->d_gemmPart.buf, out, w->inDim, w->outDim, (uint32_t)rows, c->stream));
}
extern "C" int effort_moe_route_rows(effort_ctx* c, const float* h, const void* normW, const void* gateW, int n, int numExperts, float* gateOut,
                                     uint32_t* idx2, float* val2, int rows) {
    if (n <= 0 || numExperts <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "moe_route_rows: n, numExperts >= 1, 1 <= rows <= 64");
    if (!moe_route_supported((uint32_t)n, (uint32_t)numExperts))
        return fail(c, EFFORT_ERR_SHAPE, "moe_route_rows: n % 16 == 0, 16 <= n <= 16384, 1 <= numExperts <= 64");
    if (!c || !h || !normW || !gateW || !idx2 || !val2) return fail(c, EFFORT_ERR_ARG, "moe_route_rows: null argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_moe_route_rows(h, static_cast<const uint16_t*>(normW), static_cast<const uint16_t*>(gateW), (uint32_t)n, (uint32_t)numExperts, gateOut,
                                     idx2, val2, (uint32_t)rows, c->stream));
}
extern "C" int effort_mix2_add_rows(effort_ctx* c, float* h, const float* f, const float* val2, int n, int rows) {
    if (n <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "mix2_add_rows: n >= 1, 1 <= rows <= 64");
    if (!c || !h || !f || !val2) return fail(c, EFFORT_ERR_ARG, "mix2_add_rows: null argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_mix2_add_rows(h, f, val2, (uint32_t)n, (uint32_t)rows, c->stream));
}
extern "C" int effort_fetch_rows(effort_ctx* c, const void* emb, const uint32_t* ids, float* out, int n, int rows) {
    if (n <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "fetch_rows: n >= 1, 1 <= rows <= 64");
    if (!c || !emb || !ids || !out) return fail(c, EFFORT_ERR_ARG, "fetch_rows: null argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_fetch_rows(static_cast<const uint16_t*>(emb), ids, out, (uint32_t)n, (uint32_t)rows, c->stream));
}
extern "C" int effort_add_rmsnorm_mul_rows(effort_ctx* c, float* h, const float* delta, const void* w, float* out, int n, int rows) {
    if (n <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "add_rmsnorm_mul_rows: n >= 1, 1 <= rows <= 64");
    if (!c || !h || !w || !out) return fail(c, EFFORT_ERR_ARG, "add_rmsnorm_mul_rows: null argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_add_rmsnorm_mul_rows(h, delta, static_cast<const uint16_t*>(w), out, (uint32_t)n, (uint32_t)rows, c->stream));
}
static bool prefill_range_ok(int pos0, int rows, int maxTokens) {
    return prefill_rows_ok(rows) && pos0 >= 0 && maxTokens > 0 && pos0 <= maxTokens - rows;
}
extern "C" int effort_rope_kv_rows(effort_ctx* c, const float* xq, const float* xk, const float* xv, float* qOut, float* kCache, float* vCache,
                                   int pos0, int rows, int numHeads, int numHeadsKV, int headDim, int maxTokens, float ropeBase) {
    if (!prefill_range_ok(pos0, rows, maxTokens)) return fail(c, EFFORT_ERR_ARG, "rope_kv_rows: 1 <= rows <= 64, 0 <= pos0, pos0 + rows <= maxTokens");
    if (numHeads <= 0 || numHeadsKV <= 0 || numHeads % numHeadsKV || headDim < 2 || headDim > 1024 || headDim % 2 || !(ropeBase > 1.0f))
        return fail(c, EFFORT_ERR_SHAPE, "rope_kv_rows: bad head geometry");
    if (!c || !xq || !xk || !xv || !qOut || !kCache || !vCache) return fail(c, EFFORT_ERR_ARG, "rope_kv_rows: null argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_rope_kv_rows(xq, xk, xv, qOut, kCache, vCache, (uint32_t)pos0, (uint32_t)rows, numHeads, numHeadsKV, headDim, ropeBase, c->stream));
}
// The two prefill attentions take the same arguments and refuse the same ones; `name` heads the messages.
static int prefill_attention(effort_ctx* c, const char* name, decltype(&launch_attention_rows) launch, const float* q, const float* kCache,
                             const float* vCache, int pos0, int rows, float* out, int numHeads, int headDim, int maxTokens) {
    char what[96];
    auto refuse = [&](int code, const char* why) { snprintf(what, sizeof(what), "%s: %s", name, why); return fail(c, code, what); };
    if (!prefill_range_ok(pos0, rows, maxTokens)) return refuse(EFFORT_ERR_ARG, "1 <= rows <= 64, 0 <= pos0, pos0 + rows <= maxTokens");
    if (numHeads <= 0 || maxTokens > 8192 || (headDim != 64 && headDim != 128 && headDim != 256))
        return refuse(EFFORT_ERR_SHAPE, "headDim 64/128/256, maxTokens <= 8192");
    if (!c || !q || !kCache || !vCache || !out) return refuse(EFFORT_ERR_ARG, "null argument");
    JOIN_TRY(c);
    return hip_rc(c, name, launch(q, kCache, vCache, (uint32_t)pos0, (uint32_t)rows, out, numHeads, headDim, c->stream));
}
extern "C" int effort_attention_rows(effort_ctx* c, const float* q, const float* kCache, const float* vCache, int pos0, int rows, float* out,
                                     int numHeads, int headDim, int maxTokens) {
    return prefill_attention(c, "attention_rows", launch_attention_rows, q, kCache, vCache, pos0, rows, out, numHeads, headDim, maxTokens);
}
extern "C" int effort_attention_block(effort_ctx* c, const float* q, const float* kCache, const float* vCache, int pos0, int rows, float* out,
                                      int numHeads, int headDim, int maxTokens) {
    return prefill_attention(c, "attention_block", launch_attention_block, q, kCache, vCache, pos0, rows, out, numHeads, headDim, maxTokens);
}
extern "C" int effort_top2_softmax(effort_ctx* c, const float* gate, int n, uint32_t* idx2, float* val2) {
    if (!c || !gate || !idx2 || !val2 || n < 1) return fail(c, EFFORT_ERR_ARG, "top2_softmax: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_top2_softmax(gate, (uint32_t)n, idx2, val2, c->stream));
}
extern "C" int effort_mix2(effort_ctx* c, const float* f0, const float* f1, const float* val2, float* out, int n) {
    if (!c || !f0 || !f1 || !val2 || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "mix2: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_mix2(f0, f1, val2, out, (uint32_t)n, c->stream));
}
extern "C" int effort_moe_route(effort_ctx* c, const float* h, const void* normW, const void* gateW, int n, int numExperts, float* gateOut,
                                uint32_t* idx2, float* val2) {
    if (!c || !h || !normW || !gateW || !idx2 || !val2) return fail(c, EFFORT_ERR_ARG, "moe_route: null argument");
    JOIN_TRY(c);
    if (n <= 0 || numExperts <= 0 || !moe_route_supported((uint32_t)n, (uint32_t)numExperts))
        return fail(c, EFFORT_ERR_SHAPE, "moe_route: n % 16 == 0, 16 <= n <= 16384, 1 <= numExperts <= 64");
    return HIP_RC(c, launch_moe_route(h, static_cast<const uint16_t*>(normW), static_cast<const uint16_t*>(gateW), (uint32_t)n, (uint32_t)numExperts, gateOut,
                                idx2, val2, c->stream));
}
extern "C" int effort_mix2_add(effort_ctx* c, float* h, const float* f0, const float* f1, const float* val2, int n) {
    if (!c || !h || !f0 || !f1 || !val2 || n <= 0) return fail(c, EFFORT_ERR_ARG, "mix2_add: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_mix2_add(h, f0, f1, val2, (uint32_t)n, c->stream));
}
extern "C" int effort_argmax(effort_ctx* c, const float* logits, int n, uint32_t* idOut, uint32_t* pos, uint32_t* history, int historyLen) {
    if (!c || !logits || !idOut || !pos || n <= 0 || (history && historyLen <= 0)) return fail(c, EFFORT_ERR_ARG, "argmax: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_argmax(logits, (uint32_t)n, idOut, pos, history, (uint32_t)(history ? historyLen : 0), c->d_status + 1, c->stream));
}
// The sampled pick (sample.hip).  The settings are read on the device: a captured step serves every seed, temperature, top-k and top-p.
extern "C" int effort_sample(effort_ctx* c, const float* logits, int n, const effort_sample_params* params, uint32_t* idOut, uint32_t* pos,
                             uint32_t* history, int historyLen, uint32_t* topkIdx, float* topkVal) {
    if (!c || !logits || !params || !idOut || !pos || n <= 0 || (history && historyLen <= 0)) return fail(c, EFFORT_ERR_ARG, "sample: bad argument");
    JOIN_TRY(c);
    return HIP_RC(c, launch_sample(logits, (uint32_t)n, params, idOut, pos, history, (uint32_t)(history ? historyLen : 0), c->d_status + 1, topkIdx, topkVal,
                             c->stream));
}
extern "C" int effort_topk(effort_ctx* c, const float* logits, int n, int k, uint32_t* idx, float* val) {
    if (!c || !logits || !idx || !val || n <= 0 || k < 1 || k > EFFORT_SAMPLE_MAX_K) return fail(c, EFFORT_ERR_ARG, "topk: bad argument (1 <= k <= 64)");
    JOIN_TRY(c);
    return HIP_RC(c, launch_topk(logits, (uint32_t)n, (uint32_t)k, idx, val, c->stream));
}
// The generation rules (rules.hip), between the LM head and the pick.  Their settings, too, are read on the device.
extern "C" int effort_logit_rules(effort_ctx* c, const float* logitsIn, int n, const effort_rules_params* params, const uint32_t* tok, const uint32_t* pos,
                                  uint32_t* seq, int seqLen, const uint32_t* biasIds, const float* biasVals, uint32_t* stopPos, float* logitsOut) {
    if (!c || n < 1 || seqLen < 0) return fail(c, EFFORT_ERR_ARG, "logit_rules: bad argument (n >= 1, seqLen >= 0)");
    if (!logitsIn || !logitsOut || !params || !pos) return fail(c, EFFORT_ERR_ARG, "logit_rules: null argument");
    if (!tok != !seq || !biasIds != !biasVals) return fail(c, EFFORT_ERR_ARG, "logit_rules: tok and seq, bias ids and values come in pairs");
    JOIN_TRY(c);
    return HIP_RC(c, launch_rules(logitsIn, (uint32_t)n, params, tok, pos, seq, (uint32_t)seqLen, biasIds, biasVals, stopPos, logitsOut, c->d_status + 1,
                                  c->stream));
}
extern "C" uint32_t effort_sample_bits(uint32_t seedLo, uint32_t seedHi, uint32_t stream, uint32_t pos) { return philox_x0(seedLo, seedHi, stream, pos); }

// ---- status words: conditions the device could not report through a return code.  Each is read and cleared. ----
static int read_and_clear(effort_ctx* c, int* word, int* host_out) {
    if (!c || !host_out) return EFFORT_ERR_ARG;
    JOIN_TRY(c);
    HIP_TRY(c, hipMemcpyAsync(host_out, word, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(word, 0, 4, c->stream));
    return HIP_RC(c, hipStreamSynchronize(c->stream));
}
// The decode glue (the position lives in device memory): bit 0 = a step ran past the key/value cache or the history buffer
// (nothing was written there), bit 1 = argmax over NaN logits (token 0 returned).
extern "C" int effort_decode_status(effort_ctx* c, int* host_out) { return read_and_clear(c, c ? c->d_status + 1 : nullptr, host_out); }
// Rows of the last effort_convert_fp16 calls whose bucket 0 overflowed in the literal preBucketize path (zero padding
// tying with real zeros, convert.metal:40-61: the reference drops those elements silently).
extern "C" int effort_convert_status(effort_ctx* c, int* host_out) { return read_and_clear(c, c ? c->d_status : nullptr, host_out); }
