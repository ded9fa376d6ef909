// The host layer behind include/effort_hip.h, shared by its units: the context, the weight handle and the helpers every entry point uses.
// ctx.hip: contexts, pools, lane executor, setters; weights.hip: handles; comm.hip: RCCL; mul.hip: the group launch; glue.hip: the rest.
// Host-side equivalent of class BucketMul / BucketMulQ4 (bucketMul.swift:18-90, bucketMulQ4.swift:18-87)
// and of the slice of class Gpu they use (helpers/gpu.swift:109-196).
#pragma once
#include <cstdio>
#include <cstring>
#include <new>

#include "../../include/effort_hip.h"
#include "../../include/effort_hip_debug.h"
#include "effort_internal.h"
#include "lanes.h"
#include "plan.h"

struct ncclComm;              // rccl.h is comm.hip's alone, rocblas.h glue.hip's: the context keeps their handles as opaque pointers
struct _rocblas_handle;

// What ONE multiply launch in flight owns: the reference's singleton scratch (BucketMul.shared: cutoff, dispatch counter,
// partial tiles) plus the launch machinery's (arrival tickets, per-slice counts, item queues).  A context has one such lane,
// or -- effort_set_overlap -- up to kMaxLanes of them, each with an internal stream: independent launches then overlap.
struct Lane {
    hipStream_t own = nullptr;        // internal stream (overlap mode); with one lane the launches go to the context's stream
    hipEvent_t done = nullptr;        // "everything enqueued on the lane so far": recorded LAZILY, when somebody is about to wait for the lane (lane_mark)
    bool dirty = false;               // launches were enqueued on `own` since `done` was last recorded
    float* d_cutoff = nullptr;        // BucketMul.cutoff
    uint32_t* d_count = nullptr;      // dispatch.size
    float* d_slabs = nullptr;         // partial tiles (replaces tmpMulVec)
    uint32_t* d_counters = nullptr;   // per-tile arrival tickets (zero between calls)
    uint32_t* d_sliceCounts = nullptr;
    uint32_t* d_queue = nullptr;      // item queues of persistent launches
    // where each call of the lane's last (group) launch keeps its per-slice counts; slices == 0: dispatch.size is d_count
    uint32_t lastCalls = 1, lastSliceOff[effort::kMaxGroup] = {0}, lastSlices[effort::kMaxGroup] = {0};
    // what each launch of the lane's last group ran (launch_mul_t fills it; effort_debug_last_variant)
    uint32_t lastLaunches = 0;
    effort::LaunchedVariant lastVariant[effort::kMaxLaunches] = {};
};

// Context scratch that only grows: `have` elements at `buf`.  grow(): an adequate buffer is left untouched (its address may sit in a captured
// graph); otherwise the stream is synchronised (nothing in flight reads the old one), the old one freed and `want` >= need elements
// allocated.  A failed allocation leaves buf null and have 0.
template <typename T>
struct Scratch {
    T* buf = nullptr;
    size_t have = 0;
    int grow(effort_ctx* c, size_t need, size_t want);
    void release() { hipFree(buf); buf = nullptr; have = 0; }
};
// The context's scratch buffers, declared and released (effort_destroy) through this one list.  Each is its OWN allocation.
#define EFFORT_CTX_SCRATCH(X)                                                                                                              \
    X(uint16_t, d_vhalf)        /* v.asFloat16() for the dense baseline */                                                                 \
    X(uint16_t, d_xhRows)       /* effort_dense_gemm_rows: f16(x) of a block.  Not d_vhalf: its address sits in captured token steps (rocBLAS backend) */ \
    X(float, d_gemmPart)        /* effort_dense_gemm_rows: the k splits' partial sums */                                                   \
    X(uint16_t, d_xhRouted)     /* effort_dense_gemm_rows_routed: its OWN three (a captured effort_dense_gemm_rows keeps the block multiply's addresses) */ \
    X(float, d_routedPart) X(uint32_t, d_routedGroups)      /* ... the groups: per-expert counts and assignment lists (a fixed size) */    \
    X(uint16_t, d_convVals)     /* converter scratch (transposed matrix) */

struct effort_ctx {
    static constexpr uint32_t kMaxTiles = 1024, kMaxSlices = 4096;
    static constexpr size_t kSlabBytes = (size_t)64 << 20;   // a lane's partial-tile scratch
    int device = 0;
    hipStream_t stream = nullptr;
    // The planner's persistent settings (plan.h), written by effort_create and the setters: CU count, lanes, persistent, tuning overrides,
    // split cutoff, clock mode and the lanes' scratch sizes.  A launch copies it and fills in what belongs to the call (mul.hip: call_env).
    effort::PlanEnv env = scratch_env();
    static effort::PlanEnv scratch_env() { effort::PlanEnv e; e.slabBytes = kSlabBytes; e.maxTiles = kMaxTiles; e.maxSlices = kMaxSlices; return e; }
    Lane lane[effort::kMaxLanes];
    effort::LaneBook book;            // overlap mode: which lanes hold launches nobody waited for yet, and the ranges they touch (lanes.h)
    int lastLane = 0;
    hipEvent_t forkEv = nullptr;      // overlap mode: "everything enqueued on the context's stream so far"
    uint32_t* d_blockScratch = nullptr;
#define EFFORT_X(T, name) Scratch<T> name;
    EFFORT_CTX_SCRATCH(EFFORT_X)
#undef EFFORT_X
    float* d_cos = nullptr;
    int* d_status = nullptr;          // [0] converter overflow count, [1] decode status bits, [2..3] outlier validation
    unsigned long long* d_tstamp = nullptr;   // device-clock stamps of the multiply kernel (timing mode)
    double wallClockKHz = 100000.0;
    _rocblas_handle* blas = nullptr;  // the dense baseline's rocBLAS handle, created at first use (glue.hip)
    ncclComm* comm = nullptr;         // effort_comm_create: this rank's RCCL communicator (one process per GPU; comm.hip)
    int commRank = 0, commWorld = 1;
    bool denseRocblas = false;        // effort_set_dense_backend: basicMul through rocBLAS instead of dense_gemv_kernel
    bool rowReuse = false;            // effort_set_row_reuse: the bucket-row stream with the ordinary cache policy instead of nt (GroupKArgs::split bit 3)
    // optional per-kernel timing (env.clock: device wall-clock stamps inside the multiply kernel)
    bool timing = false;              // HIP events around each group launch
    bool trace = false;               // clock mode plus one record per work item (effort_debug_trace)
    static constexpr int kMaxSamples = 4096;
    hipEvent_t* ev = nullptr;         // 2 events per sample: before and after the group's launches
    int nSamples = 0;
    char err[256] = {0};
};

struct effort_w {
    effort_ctx* ctx = nullptr;
    effort::Format fmt = effort::kFp16;
    const uint16_t* buckets = nullptr;    // what the multiply streams: the caller's buffer, or `aligned`
    const uint16_t* bucketsSrc = nullptr; // the caller's buffer (borrowed)
    uint16_t* aligned = nullptr;          // own copy with rows padded to whole 128-byte lines (effort_weights_align_rows)
    uint32_t rowPitch = 0;                // bytes between rows of `buckets`
    uint32_t srcPitch = 0;                // ... of `bucketsSrc` (2*cols as the reference lays them out, or what effort_weights_fp16_pitched was given)
    const void* stats = nullptr;
    const uint16_t* probes = nullptr;
    uint32_t inDim = 0, outDim = 0, rowsPerIn = 0, numExperts = 1, cols = 0;
    bool view = false;                // a column shard (effort_weights_column_shard): buckets, row means and the outlier index point INTO the full handle's
    effort_w* parent = nullptr;       // ... that handle; it stays alive (its buffers, that is) until its last view is freed
    uint32_t viewTrim = 0;            // ... bytes `buckets` lies behind the full handle's: the multiply's buffer descriptor ends at the END of the full allocation
    int views = 0;                    // live views of this (full) handle
    bool dead = false;                // effort_weights_free was called while views were alive: freed with the last of them
    float* rankBound = nullptr;       // [numExperts] fixed-point bound of the multiply (see launch_rank_bound)
    uint16_t* means16 = nullptr;      // FP16: the row means alone (stats lane .w), one u16 per bucket row (launch_compact_means)
    mutable int bucketDense = -1;     // effort_weights_bucket_dense_ok: -1 not checked yet, 0 two entries collide, 1 un-bucketable (effort_weights_refresh: -1 again)
    mutable uint16_t* q4Means16 = nullptr;   // Q4: the row means as f16 (stats lane .y), one u16 per bucket row; written by effort_weights_q4_dense_ok's check, read by effort_q4_gemm_rows alone
    mutable int q4Dense = -1;         // effort_weights_q4_dense_ok: -1 not checked yet, 0 not un-bucketable, 1 un-bucketable (effort_weights_refresh: -1 again)
    // Q4 outliers
    uint64_t nOutliers = 0;
    uint32_t* olBlockPtr = nullptr;   // entry bounds per block of 64 outputs (a column shard's: a slice of the full handle's)
    uint32_t* olEntry = nullptr;      // 4 bytes per outlier, jagged-diagonal order inside a block (dispatch.hip)
    uint32_t* olMeta = nullptr;       // per (block, rank): entry count << 8 | output in block
};

static inline int fail(effort_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    if (c) {
        if (e != hipSuccess) snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(c->err, sizeof(c->err), "%s", what);
    }
    return code;
}
// A HIP call's status as a return code (the message: the call's text and HIP's), and the three ways an entry point goes on only after
// EFFORT_OK: from any step, from a HIP call, and from the join -- the context's stream waits for every lane's launches (join_lanes).
static inline int hip_rc(effort_ctx* c, const char* what, hipError_t e) { return e == hipSuccess ? EFFORT_OK : fail(c, EFFORT_ERR_HIP, what, e); }
#define HIP_RC(ctx, call) hip_rc((ctx), #call, (call))
#define OK_TRY(step) do { const int rc_ = (step); if (rc_ != EFFORT_OK) return rc_; } while (0)
#define HIP_TRY(ctx, call) OK_TRY(HIP_RC(ctx, call))
#define JOIN_TRY(ctx) OK_TRY(join_lanes(ctx))

template <typename T>
int Scratch<T>::grow(effort_ctx* c, size_t need, size_t want) {
    if (need <= have) return EFFORT_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    release();
    HIP_TRY(c, hipMalloc(&buf, want * sizeof(T)));
    have = want;
    return EFFORT_OK;
}

// ---- ctx.hip: the lane executor ----
int join_lanes(effort_ctx* c);
// A group launch on a lane (overlap mode).  The lane is CHOSEN first (choose_lane) and forked (made to wait, fork_lane) only when the first
// kernel of the group is about to be launched: a group that fails validation or finds no launch geometry has then touched no stream.  From
// the fork on the lane is pending, so a later join -- in particular the join a caller owes the capturing stream before it ends a hipGraph
// capture -- always rejoins a lane that was forked.
struct LaneChoice {
    bool laned = false;               // the launch goes to a lane's own stream (lanes > 1 and no timing / clock mode)
    effort::LanePick pick;
    effort::LaunchRanges ranges;
    unsigned long long capNow = 0;
    bool forked = false;
};
int choose_lane(effort_ctx* c, LaneChoice& lc, int n, const effort_w* const* ws, const float* const* vs, const uint32_t* const* expNos,
                float* const* outs, const void* const* vAux, const float* const* resids);
int fork_lane(effort_ctx* c, LaneChoice& lc);       // before the group's first launch
// ---- weights.hip ----
int check_shape(uint32_t inDim, uint32_t outDim);
int check_bundle(effort::Format fmt, int inDim, int outDim, int percentLoad, int numExperts, int rowPitchBytes, uint32_t* pitchOut);
// ---- what effort_destroy / effort_set_stream owe the libraries that only comm.hip and glue.hip see ----
void comm_release(effort_ctx* c);
void dense_release(effort_ctx* c);
void dense_set_stream(effort_ctx* c);
