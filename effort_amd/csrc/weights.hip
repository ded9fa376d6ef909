// Weight handles (host.h: effort_w): what registration accepts, the fixed-point bound, refresh, line-aligned rows, column shards, free.
#include <mutex>

#include "host.h"

using namespace effort;

int check_shape(uint32_t inDim, uint32_t outDim) {
    // bucketMul.swift:73 (outDim % 16), :52 tmpMulVec 16384 wide; probes need 4096 inputs (:36).  The reference also asserts
    // (outDim/16) % 4 == 0 (:76: its kernel loads four columns per thread); this kernel masks a ragged last tile, so a
    // handle -- in particular a column shard of a multi-GPU split, 11008/16/8 = 86 columns -- may have any column count.
    // (an EVEN count: the row pieces are dword / dwordx2 loads, so rows must stay 4-byte aligned -- outDim % 32 == 0)
    if (inDim < (uint32_t)kProbes || outDim == 0 || outDim % 32 || outDim > 16384) return EFFORT_ERR_SHAPE;
    return EFFORT_OK;
}
// What a bundle's sizes must satisfy beyond check_shape, for both formats (Q4: percentLoad 8, rows 2 * outDim/32 bytes apart).  The multiply
// addresses EVERY per-row array through 32-bit buffer descriptors and 32-bit byte offsets, so each array of the whole stack must end below
// 4 GiB: with rows = numExperts * percentLoad * inDim,
//   the buckets      rows * pitch   (mul_item: boff = (vRow0 + rowIdx) * vRowPitch, the descriptor's vRecords; effort_weights_align_rows asks again for its pitch),
//   the stats        rows * 8       (stage_issue: make_rsrc(a.stats, ...), voff = (rowBase + ...) * 8 + 4; Q4: ((rowBase + ...) * 2 + 1) * 4) -- the
//                                   larger of the two where a bucket row is shorter than 8 bytes (FP16 outDim 32; Q4 outDim 32, 64, 96),
//   the compact means rows * 2      (FP16: a quarter of the stats, covered by them).
// Every other 32-bit product over rows is a ROW NUMBER or an element count and smaller than these: rowBase = e * expertRows and
// vRow0 = e * expertRows + j0 (* 8) are below rows <= 2^29; launch_rank_bound / launch_compact_means take rows itself; calc_dispatch's
// i * g.cols (dispatch.hip) is below rows * cols = half the buckets' bytes at most.  (All for e < numExperts: the caller's contract.)
// Returns the row pitch through *pitchOut.
int check_bundle(Format fmt, int inDim, int outDim, int percentLoad, int numExperts, int rowPitchBytes, uint32_t* pitchOut) {
    if (inDim <= 0 || outDim <= 0 || numExperts < 1 || inDim > 65535 || check_shape((uint32_t)inDim, (uint32_t)outDim) != EFFORT_OK) return EFFORT_ERR_SHAPE;
    int pitch;
    if (fmt == kFp16) {
        if (percentLoad < 1 || percentLoad > 16) return EFFORT_ERR_SHAPE;
        pitch = rowPitchBytes ? rowPitchBytes : outDim / 16 * 2;
        if (pitch < outDim / 16 * 2 || pitch % 4) return EFFORT_ERR_SHAPE;
    } else {
        if (rowPitchBytes) return EFFORT_ERR_SHAPE;
        percentLoad = 8; pitch = outDim / 32 * 2;
    }
    const size_t rows = (size_t)numExperts * (size_t)percentLoad * (size_t)inDim;
    if (rows * (size_t)pitch > 0xFFFFFFFFull || rows * 8u > 0xFFFFFFFFull) return EFFORT_ERR_SHAPE;
    if (pitchOut) *pitchOut = (uint32_t)pitch;
    return EFFORT_OK;
}
// check_bundle without a context or a device (include/effort_hip_debug.h).
extern "C" int effort_debug_check_bundle(int q4, int inDim, int outDim, int percentLoad, int numExperts, int rowPitchBytes) {
    return check_bundle(q4 ? kQ4 : kFp16, inDim, outDim, percentLoad, numExperts, rowPitchBytes, nullptr);
}

// The multiply accumulates in fixed point; its scale needs a bound on the weights: per expert, the sum over ranks
// of the largest |w| of that rank (Q4: of the largest row mean).  One pass over the buckets at registration.
static int register_bound(effort_ctx* c, effort_w* w) {
    // (Re)computed IN PLACE: launches copy these pointers by value, and a captured hipGraph bakes them in, so a refresh must
    // never move them.
    hipSetDevice(c->device);
    const size_t rows = (size_t)w->numExperts * w->rowsPerIn * w->inDim;
    float* scratch = nullptr;
    bool ok = (w->rankBound || hipMalloc(&w->rankBound, (size_t)w->numExperts * 4) == hipSuccess) && hipMalloc(&scratch, rows * 4) == hipSuccess;
    if (ok) ok = launch_rank_bound(w->fmt, w->bucketsSrc, w->srcPitch / 2u, w->stats, w->numExperts, w->rowsPerIn, w->inDim, w->cols, scratch, w->rankBound, c->stream) == hipSuccess;
    if (ok && w->fmt == kFp16) {
        ok = w->means16 || hipMalloc(&w->means16, rows * 2) == hipSuccess;
        if (ok) ok = launch_compact_means(w->stats, w->means16, (uint32_t)rows, c->stream) == hipSuccess;
    }
    if (ok) ok = hipStreamSynchronize(c->stream) == hipSuccess;
    hipFree(scratch);
    return ok ? EFFORT_OK : fail(c, EFFORT_ERR_HIP, "weight registration: rank bound");
}

extern "C" int effort_aligned_row_pitch(int outDim) {
    if (outDim <= 0 || outDim % 32 || outDim > 16384) return EFFORT_ERR_SHAPE;      // (what registration accepts: check_shape)
    return (outDim / 16 * 2 + 127) / 128 * 128;
}

// A registered handle of format `fmt` over the caller's buffers, its sizes already judged (check_bundle; `pitch` is what it returned):
// the shared fields and the fixed-point bound.  Null when the handle could not be allocated or the bound not computed (freed again).
static effort_w* new_handle(effort_ctx* c, Format fmt, const void* buckets, const void* stats, const void* probes, int inDim, int outDim,
                            int rowsPerIn, int numExperts, uint32_t pitch) {
    effort_w* w = new (std::nothrow) effort_w();
    if (!w) return nullptr;
    w->ctx = c; w->fmt = fmt;
    w->buckets = static_cast<const uint16_t*>(buckets); w->stats = stats; w->probes = static_cast<const uint16_t*>(probes);
    w->inDim = inDim; w->outDim = outDim; w->rowsPerIn = rowsPerIn; w->numExperts = numExperts; w->cols = outDim / (fmt == kFp16 ? 16 : 32);
    w->bucketsSrc = w->buckets; w->rowPitch = w->srcPitch = pitch;
    if (register_bound(c, w) != EFFORT_OK) { effort_weights_free(w); return nullptr; }
    return w;
}
extern "C" effort_w* effort_weights_fp16_pitched(effort_ctx* c, const void* buckets, int rowPitchBytes, const void* stats, const void* probes,
                                                 int inDim, int outDim, int percentLoad, int numExperts) {
    if (!c || !buckets || !stats || !probes) { fail(c, EFFORT_ERR_ARG, "effort_weights_fp16: null argument"); return nullptr; }
    uint32_t pitch = 0;
    if (check_bundle(kFp16, inDim, outDim, percentLoad, numExperts, rowPitchBytes, &pitch) != EFFORT_OK) {     // (before anything is read or allocated)
        fail(c, EFFORT_ERR_SHAPE, "effort_weights_fp16: unsupported shape or row pitch (a multiple of 4 bytes >= 2*cols; buckets < 4 GiB; stats, 8 bytes a bucket row, < 4 GiB)"); return nullptr; }
    return new_handle(c, kFp16, buckets, stats, probes, inDim, outDim, percentLoad, numExperts, pitch);
}
extern "C" effort_w* effort_weights_fp16(effort_ctx* c, const void* buckets, const void* stats, const void* probes,
                                         int inDim, int outDim, int percentLoad, int numExperts) {
    return effort_weights_fp16_pitched(c, buckets, 0, stats, probes, inDim, outDim, percentLoad, numExperts);
}

extern "C" effort_w* effort_weights_q4(effort_ctx* c, const void* buckets, const void* stats, const void* probes,
                                       const void* outliers, int64_t nOutliers, int inDim, int outDim, int numExperts) {
    if (!c || !buckets || !stats || !probes) { fail(c, EFFORT_ERR_ARG, "effort_weights_q4: null argument"); return nullptr; }
    uint32_t pitch = 0;
    if (nOutliers < 0 || check_bundle(kQ4, inDim, outDim, 8, numExperts, 0, &pitch) != EFFORT_OK) {            // (before anything is read or allocated)
        fail(c, EFFORT_ERR_SHAPE, "effort_weights_q4: unsupported shape (or buckets >= 4 GiB, or stats, 8 bytes a bucket row, >= 4 GiB)"); return nullptr; }
    effort_w* w = new_handle(c, kQ4, buckets, stats, probes, inDim, outDim, 8, numExperts, pitch);
    if (!w) return nullptr;
    if (outliers && nOutliers > 0) {
        if (outDim > 65536) { fail(c, EFFORT_ERR_SHAPE, "effort_weights_q4: outliers need outDim <= 65536"); effort_weights_free(w); return nullptr; }
        hipSetDevice(c->device);
        {   // every entry must name an element of THIS matrix (the index is built with unchecked scatters) and carry an f16 value
            int bad[2] = {0, 0};
            bool okv = hipMemsetAsync(c->d_status + 2, 0, 8, c->stream) == hipSuccess &&
                       launch_validate_outliers(static_cast<const float*>(outliers), (uint64_t)nOutliers, (uint32_t)inDim, (uint32_t)outDim, c->d_status + 2, c->stream) == hipSuccess &&
                       hipMemcpyAsync(bad, c->d_status + 2, 8, hipMemcpyDeviceToHost, c->stream) == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
            if (!okv || bad[0] || bad[1]) {
                fail(c, okv ? EFFORT_ERR_ARG : EFFORT_ERR_HIP, !okv ? "effort_weights_q4: outlier validation" :
                     bad[0] ? "effort_weights_q4: outlier entries outside the matrix (inIdx >= inDim or outIdx >= outDim)"
                            : "effort_weights_q4: outlier values that are not f16 numbers (the table comes from an f16 matrix, q4_draft.py:58-67)");
                effort_weights_free(w); return nullptr;
            }
        }
        uint32_t *tmp = nullptr, *rowPtr = nullptr;
        w->nOutliers = (uint64_t)nOutliers;
        const uint32_t olBlocks = ((uint32_t)outDim + 63u) / 64u;
        bool ok = hipMalloc(&rowPtr, ((size_t)outDim + 2) * 4) == hipSuccess && hipMalloc(&w->olBlockPtr, ((size_t)olBlocks + 1) * 4) == hipSuccess &&
                  hipMalloc(&w->olMeta, (size_t)olBlocks * 64 * 4) == hipSuccess &&
                  hipMalloc(&w->olEntry, ((size_t)nOutliers + 64) * 4) == hipSuccess && hipMalloc(&tmp, 4 * (size_t)nOutliers * 4) == hipSuccess;
        if (ok) ok = hipMemsetAsync(w->olEntry + (size_t)nOutliers, 0, 64 * 4, c->stream) == hipSuccess;     // padding: a step's load takes 64 entries from its cursor
        if (ok) ok = launch_build_outlier_index(static_cast<const float*>(outliers), w->nOutliers, (uint32_t)inDim, (uint32_t)outDim, rowPtr, w->olBlockPtr,
                                                w->olEntry, w->olMeta, tmp, c->stream) == hipSuccess;
        if (ok) ok = hipStreamSynchronize(c->stream) == hipSuccess;
        hipFree(tmp);
        uint32_t longest = 0;
        if (ok) ok = hipMemcpy(&longest, rowPtr + (size_t)outDim + 1, 4, hipMemcpyDeviceToHost) == hipSuccess;
        hipFree(rowPtr);
        if (!ok) { fail(c, EFFORT_ERR_HIP, "effort_weights_q4: outlier index"); effort_weights_free(w); return nullptr; }
        if (longest >= (1u << 24)) { fail(c, EFFORT_ERR_SHAPE, "effort_weights_q4: more than 2^24 outliers on one output"); effort_weights_free(w); return nullptr; }
    }
    return w;
}

// The fixed-point scale of the multiply comes from rankBound, a snapshot of the weights taken at registration: weights
// rewritten in place afterwards need effort_weights_refresh (the reference's loader.swift buffers are mutable).
static int copy_aligned(effort_w* w) {
    const size_t rows = (size_t)w->numExperts * w->rowsPerIn * w->inDim;
    HIP_TRY(w->ctx, hipMemcpy2DAsync(w->aligned, w->rowPitch, w->bucketsSrc, w->srcPitch, (size_t)w->cols * 2, rows, hipMemcpyDeviceToDevice, w->ctx->stream));
    return HIP_RC(w->ctx, hipStreamSynchronize(w->ctx->stream));
}
extern "C" int effort_weights_refresh(effort_w* w) {
    if (!w || !w->ctx || w->dead) return EFFORT_ERR_ARG;
    if (w->view) return fail(w->ctx, EFFORT_ERR_ARG, "effort_weights_refresh: a column shard takes its bound from the full handle -- refresh that one and shard again");
    hipSetDevice(w->ctx->device);
    w->bucketDense = w->q4Dense = -1;            // (effort_weights_bucket_dense_ok / effort_weights_q4_dense_ok look again)
    int rc = join_lanes(w->ctx);                 // multiplies still in flight on the lanes read what is recomputed here
    if (rc == EFFORT_OK) rc = register_bound(w->ctx, w);          // in place: graphs captured earlier keep valid pointers
    if (rc == EFFORT_OK && w->aligned) rc = copy_aligned(w);
    return rc;
}
// The converter's rows are 2*cols bytes apart (1376 for 11008 outputs): a 512-byte piece of a row then straddles 128-byte
// lines, the three column tiles of a row fetch 14 lines where 11 would do, and the stream runs at 5.4-5.6 TB/s instead of
// the 6.1-6.9 TB/s it reaches on line-aligned rows (measured: 4096x11264 / 12288 / 8192).  This call gives the handle its
// OWN copy of the buckets with every row starting on a 128-byte line (pitch = 2*cols rounded up to 128); the multiply
// streams the copy, and the caller's buffer is no longer read (it may be freed; effort_weights_refresh reads it again, so
// keep it if the weights are going to change).  No-op when the pitch is line-aligned already.  Results are bit-identical.
extern "C" int effort_weights_align_rows(effort_w* w) {
    if (!w || !w->ctx || w->dead) return EFFORT_ERR_ARG;
    if (w->aligned || w->rowPitch % 128u == 0u) return EFFORT_OK;        // (already on whole lines: as converted with effort_convert_fp16_pitched, or 2*cols % 128 == 0)
    hipSetDevice(w->ctx->device);
    const uint32_t pitch = (w->cols * 2u + 127u) / 128u * 128u;
    const size_t rows = (size_t)w->numExperts * w->rowsPerIn * w->inDim;
    if (rows * pitch > 0xFFFFFFFFull) return fail(w->ctx, EFFORT_ERR_SHAPE, "effort_weights_align_rows: the padded buckets would reach 4 GiB");
    if (hipMalloc(&w->aligned, rows * pitch) != hipSuccess) return fail(w->ctx, EFFORT_ERR_HIP, "effort_weights_align_rows: out of device memory");
    HIP_TRY(w->ctx, hipMemsetAsync(w->aligned, 0, rows * pitch, w->ctx->stream));
    w->rowPitch = pitch;
    const int rc = copy_aligned(w);
    if (rc != EFFORT_OK) { hipFree(w->aligned); w->aligned = nullptr; w->rowPitch = w->srcPitch; return rc; }
    w->buckets = w->aligned;
    return EFFORT_OK;
}
extern "C" int effort_weights_row_pitch(const effort_w* w) { return w ? (int)w->rowPitch : EFFORT_ERR_ARG; }
extern "C" int effort_weights_get_bound(effort_w* w, float* host_out) {
    if (!w || !w->ctx || !host_out || !w->rankBound) return EFFORT_ERR_ARG;
    return HIP_RC(w->ctx, hipMemcpy(host_out, w->rankBound, (size_t)w->numExperts * 4, hipMemcpyDeviceToHost));
}
extern "C" int effort_weights_set_bound(effort_w* w, const float* host_in) {
    if (!w || !w->ctx || !host_in || !w->rankBound || w->dead) return EFFORT_ERR_ARG;
    for (uint32_t e = 0; e < w->numExperts; e++) if (!(host_in[e] >= 0.0f)) return EFFORT_ERR_ARG;
    JOIN_TRY(w->ctx);
    HIP_TRY(w->ctx, hipStreamSynchronize(w->ctx->stream));
    return HIP_RC(w->ctx, hipMemcpy(w->rankBound, host_in, (size_t)w->numExperts * 4, hipMemcpyHostToDevice));
}

// A full handle's `views` / `dead` are touched from whichever threads shard and free (one context per rank-thread is a pattern the
// multi-GPU path invites): one process-wide mutex orders those few words.
static std::mutex g_viewMutex;
// One view of `par` is gone: the last view of a freed parent takes the parent along.
static void release_view(effort_w* par) {
    bool last = false;
    if (par) { std::lock_guard<std::mutex> lk(g_viewMutex); last = --par->views == 0 && par->dead; if (last) par->dead = false; }
    if (last) effort_weights_free(par);
}
extern "C" void effort_weights_free(effort_w* w) {
    if (!w) return;
    if (w->view) {                               // a column shard owns its bound only
        effort_w* const par = w->parent;
        hipFree(w->rankBound);
        delete w;
        release_view(par);
        return;
    }
    {   // views still read these buffers (the header says: free the shards first -- but do not dangle if not)
        std::lock_guard<std::mutex> lk(g_viewMutex);
        if (w->views > 0) { w->dead = true; return; }
    }
    hipFree(w->olBlockPtr); hipFree(w->olEntry); hipFree(w->olMeta);
    hipFree(w->aligned); hipFree(w->rankBound); hipFree(w->means16); hipFree(w->q4Means16);
    delete w;
}

// Column shard of a registered bundle for rank `rank` of `world`: bucket columns [rank*C/world, (rank+1)*C/world) of every bucket
// row -- outputs [rank*outDim/world, ...) -- as a VIEW of the full handle's buffers (rows stay rowPitch bytes apart: no copy),
// stats and probes shared (they are row-global, convert.metal:105-119: every rank computes the same cutoff and selects the same
// rows), the full matrix's fixed-point bound (every rank rounds on the same grid), and for Q4 the slice of the outlier index that
// falls on these outputs (the index is grouped by blocks of outputs: a view too).
extern "C" effort_w* effort_weights_column_shard(const effort_w* full, int rank, int world) {
    if (!full || !full->ctx) return nullptr;
    effort_ctx* c = full->ctx;
    const uint32_t unit = full->fmt == kFp16 ? 16u : 32u;
    if (world < 1 || rank < 0 || rank >= world || full->cols % (uint32_t)world || (full->cols / (uint32_t)world) % 2u) {
        fail(c, EFFORT_ERR_SHAPE, "effort_weights_column_shard: the bucket columns must split evenly into an even number per rank"); return nullptr; }
    const uint32_t per = full->cols / (uint32_t)world, outDim = per * unit;
    if (check_shape(full->inDim, outDim) != EFFORT_OK) { fail(c, EFFORT_ERR_SHAPE, "effort_weights_column_shard: shard shape"); return nullptr; }
    if (full->nOutliers && outDim % 64u) {
        fail(c, EFFORT_ERR_SHAPE, "effort_weights_column_shard: the shard must hold whole blocks of the outlier index"); return nullptr; }
    effort_w* w = new (std::nothrow) effort_w();
    if (!w) return nullptr;
    {   // (`dead` and `views` under the mutex: a concurrent effort_weights_free(full) either sees this view or is seen here)
        std::lock_guard<std::mutex> lk(g_viewMutex);
        if (full->view || full->dead) { fail(c, EFFORT_ERR_ARG, "effort_weights_column_shard: shard a full, live handle"); delete w; return nullptr; }
        const_cast<effort_w*>(full)->views++;
    }
    *w = *full;
    w->view = true; w->parent = const_cast<effort_w*>(full); w->views = 0; w->dead = false;
    w->aligned = nullptr; w->rankBound = nullptr;
    w->buckets = full->buckets + (size_t)rank * per;            // what the multiply streams (the full handle's own line-aligned copy, if it made one)
    w->viewTrim = (uint32_t)((size_t)rank * per * 2u);          // < rowPitch <= 2048: the descriptor stops where the full buffer does
    w->bucketsSrc = w->buckets; w->srcPitch = full->rowPitch;
    w->cols = per; w->outDim = outDim;
    // the row means are row-global: the view uses the full handle's compact copy (means16 stays the parent's); the fixed-point bound is
    // the FULL matrix's -- every rank rounds on the same grid -- in a word of the view's own (effort_weights_set_bound may change it)
    hipSetDevice(c->device);
    if (hipMalloc(&w->rankBound, (size_t)w->numExperts * 4) != hipSuccess ||
        hipMemcpy(w->rankBound, full->rankBound, (size_t)w->numExperts * 4, hipMemcpyDeviceToDevice) != hipSuccess) {
        fail(c, EFFORT_ERR_HIP, "effort_weights_column_shard: bound"); hipFree(w->rankBound);
        effort_w* const par = w->parent;
        delete w;
        release_view(par);
        return nullptr; }
    if (full->nOutliers) {
        w->olBlockPtr = full->olBlockPtr + (size_t)rank * outDim / 64u;                       // block bounds index the SHARED entry array
        w->olMeta = full->olMeta + (size_t)rank * outDim;                                     // (64 meta words per block of 64 outputs)
    }
    return w;
}
