// C ABI of libeffort_hip.so (include/effort_hip.h): contexts, weight handles, launch orchestration.
// Host-side equivalent of class BucketMul / BucketMulQ4 (bucketMul.swift:18-90, bucketMulQ4.swift:18-87)
// and of the slice of class Gpu they use (helpers/gpu.swift:109-196).
#include <dlfcn.h>
#include <rccl/rccl.h>          // types only: the library is opened when the first communicator is asked for (rccl(), below)
#include <rocblas/rocblas.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/effort_hip.h"
#include "../../include/effort_hip_debug.h"
#include "effort_internal.h"
#include "lanes.h"
#include "plan.h"
#include "sample_device.h"

using namespace effort;

static constexpr size_t kStampBytes = (size_t)(kTraceOff + kTraceItems * 12) * 8;   // phase stamps + per-item trace records

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

struct effort_ctx {
    static constexpr int kMaxLanes = effort::kMaxLanes;
    int device = 0;
    hipStream_t stream = nullptr;
    int numCU = 256;
    Lane lane[kMaxLanes];
    LaneBook book;                    // overlap mode: which lanes hold launches nobody waited for yet, and the ranges they touch (lanes.h)
    int lastLane = 0;
    hipEvent_t forkEv = nullptr;      // overlap mode: "everything enqueued on the context's stream so far"
    size_t slabBytes = 0;
    uint32_t* d_blockScratch = nullptr;
    uint16_t* d_vhalf = nullptr;      // v.asFloat16() for the dense baseline
    size_t vhalfElems = 0;
    uint16_t* d_xhRows = nullptr;     // effort_dense_gemm_rows: f16(x) of a block.  Its OWN scratch: d_vhalf's address sits in captured token steps (rocBLAS backend)
    size_t xhRowsElems = 0;
    float* d_gemmPart = nullptr;      // effort_dense_gemm_rows: the k splits' partial sums
    size_t gemmPartFloats = 0;
    uint16_t* d_xhRouted = nullptr;   // effort_dense_gemm_rows_routed: its OWN three (a captured effort_dense_gemm_rows keeps the block multiply's addresses)
    size_t xhRoutedElems = 0;
    float* d_routedPart = nullptr;
    size_t routedPartFloats = 0;
    uint32_t* d_routedGroups = nullptr;   // per-expert counts and assignment lists (a fixed size)
    size_t routedGroupWords = 0;
    float* d_cos = nullptr;
    uint16_t* d_convVals = nullptr;   // converter scratch (transposed matrix)
    size_t convElems = 0;
    int* d_status = nullptr;
    int persistent = -1;              // workgroups per CU of group launches: -1 heuristic, 0 plain grid, R > 0 persistent
    static constexpr uint32_t kMaxTiles = 1024, kMaxSlices = 4096;
    static constexpr size_t kSlabBytes = (size_t)64 << 20;   // a lane's partial-tile scratch
    unsigned long long* d_tstamp = nullptr;   // device-clock stamps of the multiply kernel (timing mode)
    double wallClockKHz = 100000.0;
    rocblas_handle blas = nullptr;
    ncclComm_t comm = nullptr;        // effort_comm_create: this rank's RCCL communicator (one process per GPU)
    int commRank = 0, commWorld = 1;
    bool denseRocblas = false;        // effort_set_dense_backend: basicMul through rocBLAS instead of dense_gemv_kernel
    // tuning overrides (0 = heuristic)
    int tuneW = 0, tuneE = 0, tuneS = 0;
    bool splitCutoff = false;     // run findCutoff32 as its own 1-workgroup kernel instead of inside every workgroup
    bool rowReuse = false;        // effort_set_row_reuse: the bucket-row stream with the ordinary cache policy instead of nt (GroupKArgs::split bit 3)
    // optional per-kernel timing
    bool timing = false;          // HIP events around each kernel
    bool clock = false;           // device wall-clock stamps inside the multiply kernel
    bool trace = false;           // ... plus one record per work item (effort_debug_trace)
    static constexpr int kMaxSamples = 4096;
    hipEvent_t* ev = nullptr;         // 4 events per sample
    int nSamples = 0;
    char err[256] = {0};
};

struct effort_w {
    effort_ctx* ctx = nullptr;
    Format fmt = kFp16;
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
    // Q4 outliers
    uint64_t nOutliers = 0;
    uint32_t* olBlockPtr = nullptr;   // entry bounds per block of 64 outputs (a column shard's: a slice of the full handle's)
    uint32_t* olEntry = nullptr;      // 4 bytes per outlier, jagged-diagonal order inside a block (dispatch.hip)
    uint32_t* olMeta = nullptr;       // per (block, rank): entry count << 8 | output in block
};

static int fail(effort_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    if (c) {
        if (e != hipSuccess) snprintf(c->err, sizeof(c->err), "%s: %s", what, hipGetErrorString(e));
        else snprintf(c->err, sizeof(c->err), "%s", what);
    }
    return code;
}
#define HIP_TRY(ctx, call)                                                   \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return fail((ctx), EFFORT_ERR_HIP, #call, e_); \
    } while (0)

// Context scratch that only grows: `have` elements at `buf`.  An adequate buffer is left untouched (its address may sit in a captured
// graph); otherwise the stream is synchronised (nothing in flight reads the old one), the old one freed and `want` >= need elements
// allocated.  A failed allocation leaves buf null and have 0.
template <typename T>
static int grow_scratch(effort_ctx* c, T*& buf, size_t& have, size_t need, size_t want) {
    if (need <= have) return EFFORT_OK;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    hipFree(buf); buf = nullptr; have = 0;
    HIP_TRY(c, hipMalloc(&buf, want * sizeof(T)));
    have = want;
    return EFFORT_OK;
}

// RCCL is bound at RUN time, when the first communicator is asked for: a single-GPU host needs no librccl to load this library,
// and a process that has one mapped already (PyTorch-ROCm brings its own copy) gets THAT one -- dlopen by soname returns the copy
// already in the process -- so two RCCLs never meet in one address space; a plain C / Swift host gets the system ROCm's.
struct RcclApi {
    void* lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
};
static const RcclApi& rccl() {
    static RcclApi api = [] {
        RcclApi a;
        for (const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            a.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (a.lib) break;
        }
        if (!a.lib) return a;
        a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(a.lib, "ncclGetUniqueId"));
        a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(a.lib, "ncclCommInitRank"));
        a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(a.lib, "ncclCommDestroy"));
        a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(a.lib, "ncclAllGather"));
        a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(a.lib, "ncclGetErrorString"));
        a.ok = a.GetUniqueId && a.CommInitRank && a.CommDestroy && a.AllGather && a.GetErrorString;
        return a;
    }();
    return api;
}

extern "C" const char* effort_version(void) { return "effort-hip 0.1 (gfx950)"; }
static char g_createErr[256] = "null context";       // effort_last_error(NULL): why the last effort_create failed, if one did
extern "C" const char* effort_last_error(effort_ctx* c) { return c ? c->err : g_createErr; }

static bool lane_alloc(effort_ctx* c, Lane& L) {
    bool ok = hipMalloc(&L.d_cutoff, 512) == hipSuccess && hipMalloc(&L.d_count, 16) == hipSuccess &&
              hipMalloc(&L.d_slabs, c->slabBytes) == hipSuccess && hipMalloc(&L.d_counters, effort_ctx::kMaxTiles * 4) == hipSuccess &&
              hipMalloc(&L.d_sliceCounts, effort_ctx::kMaxSlices * 4) == hipSuccess && hipMalloc(&L.d_queue, kQueueWords * 4) == hipSuccess;
    if (!ok) return false;
    hipMemset(L.d_counters, 0, effort_ctx::kMaxTiles * 4);
    hipMemset(L.d_sliceCounts, 0, effort_ctx::kMaxSlices * 4);
    hipMemset(L.d_queue, 0, kQueueWords * 4);
    hipMemset(L.d_cutoff, 0, 512);
    hipMemset(L.d_count, 0, 16);
    return true;
}
// The lanes' streams and events are POOLED per process and never destroyed: a stream or event that took part in a hipGraph
// capture and is destroyed while other captured graphs are alive crashes a later hipGraphLaunch inside the runtime (ROCm 7.2:
// segfault in hipGraphLaunch after a multi-lane context was destroyed; tools/lab/lane_crash.py reproduces it).  A context returns
// them to the pool; the next one takes them from there.
// The pools are keyed by DEVICE: a stream or event belongs to the device that was current when it was created, and a context
// of another device must never be handed one (its launches would go to the wrong GPU).  The caller has made `device` current.
static std::mutex g_poolMutex;
static std::map<int, std::vector<hipStream_t>> g_streamPool;
static std::map<int, std::vector<hipEvent_t>> g_eventPool;
static hipStream_t pool_stream(int device) {
    std::lock_guard<std::mutex> lk(g_poolMutex);
    auto& pool = g_streamPool[device];
    if (!pool.empty()) { hipStream_t s = pool.back(); pool.pop_back(); return s; }
    hipStream_t s = nullptr;
    return hipStreamCreateWithFlags(&s, hipStreamNonBlocking) == hipSuccess ? s : nullptr;
}
static hipEvent_t pool_event(int device) {
    std::lock_guard<std::mutex> lk(g_poolMutex);
    auto& pool = g_eventPool[device];
    if (!pool.empty()) { hipEvent_t e = pool.back(); pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    return hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess ? e : nullptr;
}
static void pool_put(int device, hipStream_t s) { if (s) { std::lock_guard<std::mutex> lk(g_poolMutex); g_streamPool[device].push_back(s); } }
static void pool_put(int device, hipEvent_t e) { if (e) { std::lock_guard<std::mutex> lk(g_poolMutex); g_eventPool[device].push_back(e); } }

static void lane_free(int device, Lane& L) {
    pool_put(device, L.own);
    pool_put(device, L.done);
    hipFree(L.d_cutoff); hipFree(L.d_count); hipFree(L.d_slabs); hipFree(L.d_counters); hipFree(L.d_sliceCounts); hipFree(L.d_queue);
    L = Lane();
}

extern "C" effort_ctx* effort_create(int device, void* stream) {
    if (hipSetDevice(device) != hipSuccess) return nullptr;
    effort_ctx* c = new (std::nothrow) effort_ctx();
    if (!c) return nullptr;
    c->device = device;
    c->stream = reinterpret_cast<hipStream_t>(stream);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->numCU = prop.multiProcessorCount;
    c->slabBytes = effort_ctx::kSlabBytes;
    {   // function attributes belong to a device: set them when the device's first context is created
        static std::mutex m; static std::map<int, bool> prepared;
        std::lock_guard<std::mutex> lk(m);
        if (!prepared[device]) {
            const hipError_t pe = bucket_mul_prepare_device();
            if (pe != hipSuccess) { snprintf(g_createErr, sizeof(g_createErr), "effort_create: kernel attributes: %s", hipGetErrorString(pe)); delete c; return nullptr; }
            prepared[device] = true;
        }
    }
    bool ok = lane_alloc(c, c->lane[0]) && hipMalloc(&c->d_blockScratch, 4096 * 4) == hipSuccess &&
              hipMalloc(&c->d_cos, 16) == hipSuccess && hipMalloc(&c->d_status, 16) == hipSuccess &&
              hipMalloc(&c->d_tstamp, kStampBytes) == hipSuccess;
    if (!ok) { snprintf(g_createErr, sizeof(g_createErr), "effort_create: out of device memory for the context scratch"); effort_destroy(c); return nullptr; }
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device) == hipSuccess && khz > 0) c->wallClockKHz = khz;
    hipMemset(c->d_tstamp, 0, kStampBytes);
    { unsigned long long init[2] = {~0ull, 0ull}; hipMemcpy(c->d_tstamp, init, 16, hipMemcpyHostToDevice); }
    hipMemset(c->d_status, 0, 16);
    return c;
}

// ---- lanes: independent launches of one context in flight together (effort_set_overlap) -------------------------
// The scheduler (lanes.h: c->book) decides; what follows issues the HIP calls its answers call for.
// The lane's `done` event, brought up to date.  An event per launch made a chain of dependent lone calls -- which the scheduler
// keeps on ONE lane, in order -- pay an event packet between every two kernels (the reference's own timing loop,
// benchmarks/benchmark.swift:245-257: 30.1 us per call with lanes against 22.8 without, after the fork was already skipped on an
// idle stream); recorded only where something waits for the lane -- a join, or a launch on another lane that depends on it -- the
// chain is back-to-back kernels on the lane's stream and nothing else.
static hipError_t lane_mark(Lane& L) {
    if (!L.dirty) return hipSuccess;
    const hipError_t e = hipEventRecord(L.done, L.own);
    if (e == hipSuccess) L.dirty = false;
    return e;
}
// `st` waits for everything enqueued on the lanes of `set` so far.
static hipError_t wait_for_lanes(effort_ctx* c, hipStream_t st, uint32_t set) {
    for (int i = 0; i < effort_ctx::kMaxLanes; i++) if (set >> i & 1u) {
        hipError_t e = lane_mark(c->lane[i]);
        if (e == hipSuccess) e = hipStreamWaitEvent(st, c->lane[i].done, 0);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
// The capture the context's stream is in (0: none).
static unsigned long long capture_of(hipStream_t st) {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    unsigned long long id = 0;
    if (hipStreamGetCaptureInfo(st, &cap, &id) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return cap == hipStreamCaptureStatusActive ? (id ? id : ~0ull) : 0ull;
}
// The capture rule (LaneBook::match_capture): refused with a message instead of surfacing as a HIP error in the middle of a launch.
static bool lanes_match_capture(effort_ctx* c, unsigned long long now) {
    uint32_t dropped = 0;
    if (!c->book.match_capture(now, &dropped)) { snprintf(c->err, sizeof(c->err), "%s", kLanesPendingBeforeCapture); return false; }
    for (int i = 0; i < effort_ctx::kMaxLanes; i++) if (dropped >> i & 1u) c->lane[i].dirty = false;
    return true;
}
// The context's stream waits for every lane's launches; from here on the context's stream order covers them.
static int join_lanes(effort_ctx* c) {
    if (c->book.pending_lanes()) {
        if (!lanes_match_capture(c, capture_of(c->stream))) return EFFORT_ERR_ARG;
        const hipError_t e = wait_for_lanes(c, c->stream, c->book.pending_lanes());
        if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "join: %s", hipGetErrorString(e)); return EFFORT_ERR_HIP; }    // (the lanes stay pending)
    }
    c->book.join();
    return EFFORT_OK;
}
// ---- a group launch on a lane (overlap mode) ----
// The lane is CHOSEN first (choose_lane) and forked (made to wait, fork_lane) only when the first kernel of the group is about to be
// launched: a group that fails validation or finds no launch geometry has then touched no stream.  From the fork on the lane is
// pending, so a later join -- in particular the join a caller owes the capturing stream before it ends a hipGraph capture -- always
// rejoins a lane that was forked.
struct LaneChoice {
    bool laned = false;               // the launch goes to a lane's own stream (lanes > 1 and no timing / clock mode)
    LanePick pick;
    LaunchRanges ranges;
    unsigned long long capNow = 0;
    bool forked = false;
};
static int choose_lane(effort_ctx* c, LaneChoice& lc, int n, const effort_w* const* ws, const float* const* vs, const uint32_t* const* expNos,
                       float* const* outs, const void* const* vAux, const float* const* resids) {
    if (lc.laned) {
        lc.capNow = capture_of(c->stream);
        if (!lanes_match_capture(c, lc.capNow)) return EFFORT_ERR_ARG;
        if (c->book.full()) { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
        for (int i = 0; i < n; i++)
            lc.ranges.call(vs[i], expNos ? expNos[i] : nullptr, vAux ? vAux[i] : nullptr, resids ? resids[i] : nullptr, outs[i], ws[i]->inDim, ws[i]->outDim);
        lc.pick = c->book.pick(lc.ranges);
    } else if (c->book.nLanes > 1) {
        { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }        // timing modes: one launch at a time, on lane 0
    }
    return EFFORT_OK;
}
// Before the group's first launch.
static int fork_lane(effort_ctx* c, LaneChoice& lc) {
    if (!lc.laned || lc.forked) return EFFORT_OK;
    Lane& L = c->lane[lc.pick.lane];
    // "after everything enqueued on the context's stream before this call": an event recorded there, the lane waits -- UNLESS the
    // stream is idle: then everything enqueued on it has completed and there is nothing to wait for.  That is the state of a
    // caller who enqueues multiply after multiply and evaluates once (helpers/gpu.swift:109-119; the reference's own timing
    // loop, benchmarks/benchmark.swift:245-257): all its work sits on the lanes, and the two HIP calls plus the cross-stream
    // edge per call made that loop 45 % SLOWER with lanes than without (round 4: 32.5 against 22.5 us per call).  A capturing
    // stream cannot be queried (and "idle" means nothing inside a capture): there the fork is a graph edge, as before.
    bool wait = true;
    if (lc.capNow == 0) {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) wait = false;
        else {
            (void)hipGetLastError();                    // ("not ready" must not linger as the thread's last error: the launchers read it after their kernels)
            if (q != hipErrorNotReady) return fail(c, EFFORT_ERR_HIP, "hipStreamQuery", q);
        }
    }
    if (wait) {
        HIP_TRY(c, hipEventRecord(c->forkEv, c->stream));
        HIP_TRY(c, hipStreamWaitEvent(L.own, c->forkEv, 0));
    }
    lc.forked = true;
    L.dirty = true;                                     // (the event itself: lane_mark, when somebody waits for the lane)
    const uint32_t waits = c->book.commit(lc.pick, lc.ranges, lc.capNow, wait);
    const hipError_t e = wait_for_lanes(c, L.own, waits);
    if (e != hipSuccess) { c->book.keep_pending(waits, lc.capNow); return fail(c, EFFORT_ERR_HIP, "lane wait", e); }
    return EFFORT_OK;
}

extern "C" int effort_set_overlap(effort_ctx* c, int lanes) {
    if (!c || lanes < 1 || lanes > effort_ctx::kMaxLanes) return EFFORT_ERR_ARG;
    hipSetDevice(c->device);
    int rc = join_lanes(c);
    if (rc != EFFORT_OK) return rc;
    if (lanes > 1) {
        if (!c->forkEv && !(c->forkEv = pool_event(c->device))) return fail(c, EFFORT_ERR_HIP, "set_overlap: event");
        for (int i = 0; i < lanes; i++) {
            Lane& L = c->lane[i];
            if (!L.d_slabs && !lane_alloc(c, L)) return fail(c, EFFORT_ERR_HIP, "set_overlap: out of device memory for a lane's scratch");
            if (!L.own && !(L.own = pool_stream(c->device))) return fail(c, EFFORT_ERR_HIP, "set_overlap: stream");
            if (!L.done && !(L.done = pool_event(c->device))) return fail(c, EFFORT_ERR_HIP, "set_overlap: event");
        }
    }
    c->book.reset(lanes); c->lastLane = 0;
    return EFFORT_OK;
}
extern "C" int effort_join(effort_ctx* c) {
    if (!c) return EFFORT_ERR_ARG;
    return join_lanes(c);
}

extern "C" void effort_destroy(effort_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    for (int i = 0; i < effort_ctx::kMaxLanes; i++) if (c->lane[i].own) hipStreamSynchronize(c->lane[i].own);
    hipStreamSynchronize(c->stream);
    if (c->comm) rccl().CommDestroy(c->comm);
    if (c->blas) rocblas_destroy_handle(c->blas);
    if (c->ev) { for (int i = 0; i < effort_ctx::kMaxSamples * 4; i++) if (c->ev[i]) hipEventDestroy(c->ev[i]); delete[] c->ev; }
    for (int i = 0; i < effort_ctx::kMaxLanes; i++) lane_free(c->device, c->lane[i]);
    pool_put(c->device, c->forkEv);
    hipFree(c->d_blockScratch); hipFree(c->d_vhalf); hipFree(c->d_xhRows); hipFree(c->d_gemmPart); hipFree(c->d_xhRouted); hipFree(c->d_routedPart); hipFree(c->d_routedGroups); hipFree(c->d_cos); hipFree(c->d_convVals); hipFree(c->d_status); hipFree(c->d_tstamp);
    delete c;
}

extern "C" int effort_set_stream(effort_ctx* c, void* stream) {
    if (!c) return EFFORT_ERR_ARG;
    if (reinterpret_cast<hipStream_t>(stream) != c->stream && join_lanes(c) != EFFORT_OK) return EFFORT_ERR_HIP;   // (the old stream carries the join)
    c->stream = reinterpret_cast<hipStream_t>(stream);
    if (c->blas) rocblas_set_stream(c->blas, c->stream);
    return EFFORT_OK;
}

extern "C" int effort_sync(effort_ctx* c) {
    if (!c) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EFFORT_OK;
}

// ---- weights ------------------------------------------------------------------------------------
static int check_shape(uint32_t inDim, uint32_t outDim) {
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
static int check_bundle(Format fmt, int inDim, int outDim, int percentLoad, int numExperts, int rowPitchBytes, uint32_t* pitchOut) {
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

extern "C" effort_w* effort_weights_fp16_pitched(effort_ctx* c, const void* buckets, int rowPitchBytes, const void* stats, const void* probes,
                                                 int inDim, int outDim, int percentLoad, int numExperts) {
    if (!c || !buckets || !stats || !probes) { fail(c, EFFORT_ERR_ARG, "effort_weights_fp16: null argument"); return nullptr; }
    uint32_t pitch = 0;
    if (check_bundle(kFp16, inDim, outDim, percentLoad, numExperts, rowPitchBytes, &pitch) != EFFORT_OK) {     // (before anything is read or allocated)
        fail(c, EFFORT_ERR_SHAPE, "effort_weights_fp16: unsupported shape or row pitch (a multiple of 4 bytes >= 2*cols; buckets < 4 GiB; stats, 8 bytes a bucket row, < 4 GiB)"); return nullptr; }
    effort_w* w = new (std::nothrow) effort_w();
    if (!w) return nullptr;
    w->ctx = c; w->fmt = kFp16;
    w->buckets = static_cast<const uint16_t*>(buckets); w->stats = stats; w->probes = static_cast<const uint16_t*>(probes);
    w->inDim = inDim; w->outDim = outDim; w->rowsPerIn = percentLoad; w->numExperts = numExperts; w->cols = outDim / 16;
    w->bucketsSrc = w->buckets; w->rowPitch = w->srcPitch = pitch;
    if (register_bound(c, w) != EFFORT_OK) { effort_weights_free(w); return nullptr; }
    return w;
}
extern "C" effort_w* effort_weights_fp16(effort_ctx* c, const void* buckets, const void* stats, const void* probes,
                                         int inDim, int outDim, int percentLoad, int numExperts) {
    return effort_weights_fp16_pitched(c, buckets, 0, stats, probes, inDim, outDim, percentLoad, numExperts);
}

extern "C" effort_w* effort_weights_q4(effort_ctx* c, const void* buckets, const void* stats, const void* probes,
                                       const void* outliers, int64_t nOutliers, int inDim, int outDim, int numExperts) {
    if (!c || !buckets || !stats || !probes) { fail(c, EFFORT_ERR_ARG, "effort_weights_q4: null argument"); return nullptr; }
    if (nOutliers < 0 || check_bundle(kQ4, inDim, outDim, 8, numExperts, 0, nullptr) != EFFORT_OK) {           // (before anything is read or allocated)
        fail(c, EFFORT_ERR_SHAPE, "effort_weights_q4: unsupported shape (or buckets >= 4 GiB, or stats, 8 bytes a bucket row, >= 4 GiB)"); return nullptr; }
    effort_w* w = new (std::nothrow) effort_w();
    if (!w) return nullptr;
    w->ctx = c; w->fmt = kQ4;
    w->buckets = static_cast<const uint16_t*>(buckets); w->stats = stats; w->probes = static_cast<const uint16_t*>(probes);
    w->inDim = inDim; w->outDim = outDim; w->rowsPerIn = 8; w->numExperts = numExperts; w->cols = outDim / 32;
    w->bucketsSrc = w->buckets; w->rowPitch = w->srcPitch = w->cols * 2u;
    if (register_bound(c, w) != EFFORT_OK) { effort_weights_free(w); return nullptr; }
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
    HIP_TRY(w->ctx, hipStreamSynchronize(w->ctx->stream));
    return EFFORT_OK;
}
extern "C" int effort_weights_refresh(effort_w* w) {
    if (!w || !w->ctx || w->dead) return EFFORT_ERR_ARG;
    if (w->view) return fail(w->ctx, EFFORT_ERR_ARG, "effort_weights_refresh: a column shard takes its bound from the full handle -- refresh that one and shard again");
    hipSetDevice(w->ctx->device);
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
    HIP_TRY(w->ctx, hipMemcpy(host_out, w->rankBound, (size_t)w->numExperts * 4, hipMemcpyDeviceToHost));
    return EFFORT_OK;
}
extern "C" int effort_weights_set_bound(effort_w* w, const float* host_in) {
    if (!w || !w->ctx || !host_in || !w->rankBound || w->dead) return EFFORT_ERR_ARG;
    for (uint32_t e = 0; e < w->numExperts; e++) if (!(host_in[e] >= 0.0f)) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(w->ctx); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(w->ctx, hipStreamSynchronize(w->ctx->stream));
    HIP_TRY(w->ctx, hipMemcpy(w->rankBound, host_in, (size_t)w->numExperts * 4, hipMemcpyHostToDevice));
    return EFFORT_OK;
}

// A full handle's `views` / `dead` are touched from whichever threads shard and free (one context per rank-thread is a pattern the
// multi-GPU path invites): one process-wide mutex orders those few words.
static std::mutex g_viewMutex;
extern "C" void effort_weights_free(effort_w* w) {
    if (!w) return;
    if (w->view) {                               // a column shard owns its bound only; the last view of a freed parent takes the parent along
        effort_w* const par = w->parent;
        hipFree(w->rankBound);
        delete w;
        bool last = false;
        if (par) { std::lock_guard<std::mutex> lk(g_viewMutex); last = --par->views == 0 && par->dead; if (last) par->dead = false; }
        if (last) effort_weights_free(par);
        return;
    }
    {   // views still read these buffers (the header says: free the shards first -- but do not dangle if not)
        std::lock_guard<std::mutex> lk(g_viewMutex);
        if (w->views > 0) { w->dead = true; return; }
    }
    hipFree(w->olBlockPtr); hipFree(w->olEntry); hipFree(w->olMeta);
    hipFree(w->aligned); hipFree(w->rankBound); hipFree(w->means16);
    delete w;
}

// ---- multi-GPU: one process per GPU, RCCL over xGMI (the reference is single-device, helpers/gpu.swift:36-38) --------------
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
        bool last;
        { std::lock_guard<std::mutex> lk(g_viewMutex); last = --par->views == 0 && par->dead; if (last) par->dead = false; }
        if (last) effort_weights_free(par);
        return nullptr; }
    if (full->nOutliers) {
        w->olBlockPtr = full->olBlockPtr + (size_t)rank * outDim / 64u;                       // block bounds index the SHARED entry array
        w->olMeta = full->olMeta + (size_t)rank * outDim;                                     // (64 meta words per block of 64 outputs)
    }
    return w;
}
extern "C" int effort_comm_unique_id(void* id_out) {
    if (!id_out) return EFFORT_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == EFFORT_COMM_ID_BYTES, "effort_hip.h: EFFORT_COMM_ID_BYTES");
    if (!rccl().ok) return EFFORT_ERR_COMM;
    return rccl().GetUniqueId(static_cast<ncclUniqueId*>(id_out)) == ncclSuccess ? EFFORT_OK : EFFORT_ERR_COMM;
}
extern "C" int effort_comm_create(effort_ctx* c, int rank, int world, const void* id) {
    if (!c || !id || world < 1 || rank < 0 || rank >= world) return fail(c, EFFORT_ERR_ARG, "comm_create: bad argument");
    if (c->comm) return fail(c, EFFORT_ERR_ARG, "comm_create: the context has a communicator already");
    hipSetDevice(c->device);
    ncclUniqueId uid;
    memcpy(&uid, id, sizeof(uid));
    if (!rccl().ok) return fail(c, EFFORT_ERR_COMM, "comm_create: librccl.so could not be opened (dlopen) -- multi-GPU needs RCCL");
    const ncclResult_t r = rccl().CommInitRank(&c->comm, world, uid, rank);
    if (r != ncclSuccess) { c->comm = nullptr; snprintf(c->err, sizeof(c->err), "ncclCommInitRank: %s", rccl().GetErrorString(r)); return EFFORT_ERR_COMM; }
    c->commRank = rank; c->commWorld = world;
    return EFFORT_OK;
}
extern "C" int effort_comm_destroy(effort_ctx* c) {
    if (!c) return EFFORT_ERR_ARG;
    if (c->comm) { hipSetDevice(c->device); effort_sync(c); rccl().CommDestroy(c->comm); c->comm = nullptr; c->commRank = 0; c->commWorld = 1; }
    return EFFORT_OK;
}
extern "C" int effort_comm_rank(effort_ctx* c) { return c ? c->commRank : EFFORT_ERR_ARG; }
extern "C" int effort_comm_world(effort_ctx* c) { return c ? c->commWorld : EFFORT_ERR_ARG; }
// All-gather of the ranks' output slices on the context's stream, after the multiplies that wrote them (the lanes are joined):
// recv = [world][count] f32.  send may be recv + rank*count (in place).
extern "C" int effort_allgather_outputs(effort_ctx* c, const float* send, float* recv, int count) {
    if (!c || !send || !recv || count < 1) return fail(c, EFFORT_ERR_ARG, "allgather_outputs: bad argument");
    if (!c->comm) return fail(c, EFFORT_ERR_ARG, "allgather_outputs: no communicator (effort_comm_create)");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    const ncclResult_t r = rccl().AllGather(send, recv, (size_t)count, ncclFloat, c->comm, c->stream);
    if (r != ncclSuccess) { snprintf(c->err, sizeof(c->err), "ncclAllGather: %s", rccl().GetErrorString(r)); return EFFORT_ERR_COMM; }
    return EFFORT_OK;
}

static int ensure_timing(effort_ctx* c) {
    if (c->ev) return EFFORT_OK;
    c->ev = new (std::nothrow) hipEvent_t[effort_ctx::kMaxSamples * 4]();       // (value-initialised: effort_destroy walks the whole array)
    if (!c->ev) return EFFORT_ERR_HIP;
    for (int i = 0; i < effort_ctx::kMaxSamples * 4; i++) HIP_TRY(c, hipEventCreate(&c->ev[i]));
    return EFFORT_OK;
}

// ---- launch planning: the inputs of plan_group (plan.hip) ------------------------------------------
static PlanEnv plan_env(const effort_ctx* c, bool laned, bool thinEffort) {
    PlanEnv env;
    env.numCU = c->numCU; env.nLanes = c->book.nLanes; env.laned = laned;
    env.persistent = c->persistent; env.tuneW = c->tuneW; env.tuneE = c->tuneE; env.tuneS = c->tuneS;
    env.splitCutoff = c->splitCutoff; env.clock = c->clock;
    env.slabBytes = c->slabBytes; env.maxTiles = effort_ctx::kMaxTiles; env.maxSlices = effort_ctx::kMaxSlices;
    env.thinEffort = thinEffort;
    // The A/B switches below read the environment in LAB builds only (-DEFFORT_LAB: tools/build_variant*.sh); the shipped
    // library has no getenv on this path.
#ifdef EFFORT_LAB
    static const uint32_t ablate = getenv("EFFORT_ABLATE") ? (uint32_t)atoi(getenv("EFFORT_ABLATE")) : 0u;   // profiling only
    static const bool noJobs = getenv("EFFORT_NO_CUTJOBS") != nullptr, noCompact = getenv("EFFORT_NO_COMPACT_MEANS") != nullptr;
    env.ablate = ablate; env.noJobs = noJobs; env.noCompact = noCompact;
    if (getenv("EFFORT_TAIL_CALLS")) {       // profiling knobs (read at every call: tools/qbench.py --tails sweeps them in one process)
        env.tailCalls = atoi(getenv("EFFORT_TAIL_CALLS"));
        env.tailMult = getenv("EFFORT_TAIL_MULT") ? atoi(getenv("EFFORT_TAIL_MULT")) : 2;
    }
#endif
    return env;
}
static PlanCall plan_call(const effort_w* w, int pre, bool resid) {
    return PlanCall{w->inDim, w->outDim, w->cols, w->rowsPerIn, w->rowPitch, w->numExperts, w->means16 != nullptr, (uint16_t)pre, resid};
}
// The launch's mean effort is under 8 %: PlanEnv::thinEffort.
static bool thin_effort(int n, const double* efforts) {
    double sum = 0.0;
    for (int i = 0; i < n; i++) sum += efforts[i];
    return sum < 0.08 * n;
}

// One launch for a group of independent calls (a lone call is a group of one): validate, plan, choose the lane, then per launch of the
// plan copy it and the pointers into the kernel arguments and launch.
static int do_group(effort_ctx* c, Format fmt, int n, const effort_w* const* ws, const float* const* vs,
                    const uint32_t* const* expNos, float* const* outs, const double* efforts,
                    const int* prologues = nullptr, const void* const* vAux = nullptr, const float* const* resids = nullptr) {
    if (!c || !ws || !vs || !outs || !efforts) return fail(c, EFFORT_ERR_ARG, "bucketmul: null argument");
    if (n < 1 || n > kMaxGroup) return fail(c, EFFORT_ERR_ARG, "bucketmul: group size outside 1..32");
    PlanCall pc[kMaxGroup];
    for (int i = 0; i < n; i++) {                      // every argument first: nothing is launched for a group with a bad call
        if (!ws[i] || !vs[i] || !outs[i]) return fail(c, EFFORT_ERR_ARG, "bucketmul: null argument");
        if (ws[i]->dead) return fail(c, EFFORT_ERR_ARG, "bucketmul: the handle was freed (its buffers live on only for its column shards)");
        if (ws[i]->fmt != fmt) return fail(c, EFFORT_ERR_KIND, "bucketmul: weight handle of the wrong kind");
        if (!(efforts[i] >= 0.0 && efforts[i] <= 1.0)) return fail(c, EFFORT_ERR_EFFORT, "bucketmul: effort outside [0,1]");
        const int pre = prologues ? prologues[i] : 0;
        if (pre < 0 || pre > 2 || (pre && (!vAux || !vAux[i]))) return fail(c, EFFORT_ERR_ARG, "bucketmul: bad input prologue");
        if (pre && c->splitCutoff) return fail(c, EFFORT_ERR_KIND, "bucketmul: input prologues need the fused cutoff");
        // Q4: the outlier phase needs the whole TRANSFORMED input and keeps it in LDS; beyond that copy's size it gathers v from memory, where a prologue's
        // input does not exist (bucket_mul.hip, phase O).  A residual alone, or a handle without outliers, works at any size.
        if (pre && fmt == kQ4 && ws[i]->olBlockPtr && (uint32_t)ws[i]->inDim > bucket_mul_ol_lds_floats())
            return fail(c, EFFORT_ERR_SHAPE, "bucketmul: an input prologue on a Q4 handle with outliers needs inDim <= 16384 (materialise the input, or register without outliers)");
        pc[i] = plan_call(ws[i], pre, resids && resids[i]);
    }
    LaneChoice lc;
    lc.laned = c->book.nLanes > 1 && !c->timing && !c->clock;
    const PlanEnv env = plan_env(c, lc.laned, thin_effort(n, efforts));
    GroupPlan plan;
    if (plan_group(fmt, env, n, pc, &plan) != EFFORT_OK) return fail(c, plan.err, plan.msg);
    const bool tm = c->timing && c->nSamples < effort_ctx::kMaxSamples;
    hipEvent_t* ev = tm ? c->ev + 4 * c->nSamples : nullptr;
    { const int lrc = choose_lane(c, lc, n, ws, vs, expNos, outs, vAux, resids); if (lrc != EFFORT_OK) return lrc; }
    Lane& L = c->lane[lc.pick.lane];
    const hipStream_t st = lc.laned ? L.own : c->stream;
    c->lastLane = lc.pick.lane;
    if (tm) HIP_TRY(c, hipEventRecord(ev[0], st));
    L.lastLaunches = 0;
    for (uint32_t l = 0; l < plan.nLaunches; l++) {    // (more than one: a group of more than kMaxGeoms shapes)
        const LaunchPlan& lp = plan.launch[l];
        GroupKArgs ga;
        memset(&ga, 0, sizeof(ga));
        ga.groupDone = L.d_counters + effort_ctx::kMaxTiles - 1;
        ga.slabs = L.d_slabs; ga.counters = L.d_counters; ga.sliceCounts = L.d_sliceCounts; ga.cutoff = L.d_cutoff + lp.first;
        ga.tstamp = c->clock ? c->d_tstamp : nullptr;
        ga.ablate = env.ablate; ga.trace = (c->clock && c->trace) ? 1u : 0u;
        ga.split = (c->splitCutoff ? 1u : 0u) | (lp.compact ? 4u : 0u) | (c->rowReuse ? 8u : 0u);
        ga.numCU = (uint32_t)c->numCU; ga.queue = L.d_queue;
        ga.count = lp.count; ga.totalTiles = lp.totalTiles; ga.totalItems = lp.totalItems;
        ga.persistent = lp.persistent; ga.cutJobs = lp.cutJobs; ga.staggerSleeps = lp.staggerSleeps;
        for (uint32_t k = 0; k < lp.count; k++) {
            const int i = (int)(lp.first + k);
            const effort_w* w = ws[i];
            const CallPlan& p = plan.call[i];
            CallDesc& a = ga.call[k];
            a.buckets = w->buckets; a.stats = lp.compact ? (const void*)w->means16 : w->stats; a.rankBound = w->rankBound; a.probes = w->probes; a.v = vs[i];
            a.expNo = expNos ? expNos[i] : nullptr; a.out = outs[i];
            a.ol = OutlierIndex{fmt == kQ4 ? w->olBlockPtr : nullptr, w->olEntry, w->olMeta};
            a.q = (uint16_t)(int)((double)(kProbes - 1) * (1.0 - efforts[i]));            // bucketMul.swift:39
            a.bucketsTrim = (uint16_t)w->viewTrim;
            a.pre = pc[i].pre; a.vAux = a.pre ? vAux[i] : nullptr; a.resid = resids ? resids[i] : nullptr;
            a.slabOff = p.slabOff; a.tileOff = (uint16_t)p.tileOff; a.sliceOff = (uint16_t)p.sliceOff; a.geom = (uint16_t)p.geom;
            ga.geom[p.geom] = p.g;
            ga.wgEnd8[k] = (uint16_t)p.itemEnd8;
            L.lastSliceOff[i] = p.sliceOff; L.lastSlices[i] = p.g.slices;             // dispatch.size = sum of the per-slice counts
        }
        { const int frc = fork_lane(c, lc); if (frc != EFFORT_OK) return frc; }
        if (c->splitCutoff && !(env.ablate & 1u)) HIP_TRY(c, launch_find_cutoff_group(ga, st));
        HIP_TRY(c, launch_bucket_mul(fmt, plan.W, plan.E, ga, st, &L.lastVariant[l]));
        L.lastLaunches = l + 1u;
    }
    L.lastCalls = (uint32_t)n;
    if (tm) { HIP_TRY(c, hipEventRecord(ev[1], st)); c->nSamples++; }
    return EFFORT_OK;
}

extern "C" int effort_bucketmul(effort_ctx* c, const effort_w* w, const float* v, const uint32_t* expNo, float* out, double effort) {
    return do_group(c, kFp16, 1, &w, &v, &expNo, &out, &effort);
}
extern "C" int effort_bucketmul_q4(effort_ctx* c, const effort_w* w, const float* v, const uint32_t* expNo, float* out, double effort) {
    return do_group(c, kQ4, 1, &w, &v, &expNo, &out, &effort);
}
extern "C" int effort_bucketmul_group(effort_ctx* c, int n, const effort_w* const* ws, const float* const* vs,
                                      const uint32_t* const* expNos, float* const* outs, const double* efforts) {
    return do_group(c, kFp16, n, ws, vs, expNos, outs, efforts);
}
extern "C" int effort_bucketmul_group_fused(effort_ctx* c, int n, const effort_w* const* ws, const float* const* vs,
                                            const uint32_t* const* expNos, float* const* outs, const double* efforts,
                                            const int* prologues, const void* const* vAux, const float* const* resids) {
    return do_group(c, kFp16, n, ws, vs, expNos, outs, efforts, prologues, vAux, resids);
}
extern "C" int effort_bucketmul_q4_group_fused(effort_ctx* c, int n, const effort_w* const* ws, const float* const* vs,
                                               const uint32_t* const* expNos, float* const* outs, const double* efforts,
                                               const int* prologues, const void* const* vAux, const float* const* resids) {
    return do_group(c, kQ4, n, ws, vs, expNos, outs, efforts, prologues, vAux, resids);
}
extern "C" int effort_bucketmul_q4_group(effort_ctx* c, int n, const effort_w* const* ws, const float* const* vs,
                                         const uint32_t* const* expNos, float* const* outs, const double* efforts) {
    return do_group(c, kQ4, n, ws, vs, expNos, outs, efforts);
}

extern "C" int effort_calc_dispatch(effort_ctx* c, const effort_w* w, const float* v, const uint32_t* expNo, double effort,
                                    float* dispatch, uint32_t* count) {
    if (!c || !w || !v || !dispatch || w->dead) return fail(c, EFFORT_ERR_ARG, "calc_dispatch: null argument (or a freed handle)");
    if (!(effort >= 0.0 && effort <= 1.0)) return fail(c, EFFORT_ERR_EFFORT, "calc_dispatch: effort outside [0,1]");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    Lane& L = c->lane[0];
    c->lastLane = 0;
    const PlanCall pc = plan_call(w, 0, false);
    GroupPlan plan;
    if (plan_group(w->fmt, plan_env(c, false, false), 1, &pc, &plan) != EFFORT_OK) return fail(c, plan.err, "calc_dispatch: geometry");
    const MulGeom& g = plan.call[0].g;
    const uint32_t q = (uint32_t)(int)((double)(kProbes - 1) * (1.0 - effort));
    HIP_TRY(c, launch_find_cutoff(v, w->probes, expNo, q, L.d_cutoff, L.d_count, nullptr, c->stream));
    HIP_TRY(c, launch_calc_dispatch(w->fmt, w->stats, v, expNo, L.d_cutoff, g, dispatch, count, L.d_count, c->d_blockScratch, c->stream));
    L.lastCalls = 1; L.lastSlices[0] = 0;        // dispatch.size is the scalar written by the scan kernel
    L.lastLaunches = 0;                          // (no multiply kernel ran)
    return EFFORT_OK;
}

extern "C" int effort_group_dispatch_count(effort_ctx* c, int idx, uint32_t* host_out) {
    if (!c || !host_out || idx < 0 || (uint32_t)idx >= c->lane[c->lastLane].lastCalls) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    Lane& L = c->lane[c->lastLane];
    if (L.lastSlices[idx] == 0) {
        HIP_TRY(c, hipMemcpyAsync(host_out, L.d_count, 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        return EFFORT_OK;
    }
    static thread_local uint32_t h[effort_ctx::kMaxSlices];
    HIP_TRY(c, hipMemcpyAsync(h, L.d_sliceCounts + L.lastSliceOff[idx], (size_t)L.lastSlices[idx] * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    uint32_t n = 0;
    for (uint32_t i = 0; i < L.lastSlices[idx]; i++) n += h[i];
    *host_out = n;
    return EFFORT_OK;
}
extern "C" int effort_debug_slice_counts(effort_ctx* c, int idx, uint32_t* host, int maxSlices) {
    if (!c || !host || idx < 0 || (uint32_t)idx >= c->lane[c->lastLane].lastCalls || maxSlices < 1) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    Lane& L = c->lane[c->lastLane];
    const uint32_t n = L.lastSlices[idx] < (uint32_t)maxSlices ? L.lastSlices[idx] : (uint32_t)maxSlices;
    if (n) HIP_TRY(c, hipMemcpyAsync(host, L.d_sliceCounts + L.lastSliceOff[idx], (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return (int)n;
}
// The planner without a context: no device, no HIP call (include/effort_hip_debug.h).
extern "C" int effort_debug_plan(int q4, int numCU, int lanes, int n, const int* inDim, const int* outDim, const int* percentLoad,
                                 const int* prologue, const int* hasResid, const double* effort, int persistent, int tuneW, int tuneE, int tuneS,
                                 int* we, int* slices, int* tiles, int* sliceRows, int* launchOf,
                                 int* launchPersistent, int* launchCutJobs, int* launchCompact, int* launchStagger) {
    if (numCU < 1 || lanes < 1 || lanes > effort_ctx::kMaxLanes || n < 1 || n > kMaxGroup || !inDim || !outDim || !effort || !we || !slices || !tiles ||
        !sliceRows || !launchOf || !launchPersistent || !launchCutJobs || !launchCompact || !launchStagger) return EFFORT_ERR_ARG;
    const Format fmt = q4 ? kQ4 : kFp16;
    effort_ctx c0;                                     // (a context's defaults; never created: no device behind it)
    c0.numCU = numCU; c0.book.nLanes = lanes; c0.persistent = persistent; c0.tuneW = tuneW; c0.tuneE = tuneE; c0.tuneS = tuneS;
    c0.slabBytes = effort_ctx::kSlabBytes;
    PlanCall pc[kMaxGroup];
    for (int i = 0; i < n; i++) {
        const int load = q4 ? 8 : (percentLoad ? percentLoad[i] : 16);
        if (inDim[i] <= 0 || outDim[i] <= 0 || check_shape((uint32_t)inDim[i], (uint32_t)outDim[i]) != EFFORT_OK || load < 1 || load > 16) return EFFORT_ERR_SHAPE;
        if (!(effort[i] >= 0.0 && effort[i] <= 1.0)) return EFFORT_ERR_EFFORT;
        const uint32_t cols = (uint32_t)outDim[i] / (q4 ? 32u : 16u);
        pc[i] = PlanCall{(uint32_t)inDim[i], (uint32_t)outDim[i], cols, (uint32_t)load, cols * 2u, 1u, !q4, (uint16_t)(prologue ? prologue[i] : 0), hasResid && hasResid[i]};
    }
    GroupPlan plan;
    const int rc = plan_group(fmt, plan_env(&c0, lanes > 1, thin_effort(n, effort)), n, pc, &plan);
    if (rc != EFFORT_OK) return rc;
    we[0] = plan.W; we[1] = plan.E;
    for (int i = 0; i < n; i++) {
        const CallPlan& p = plan.call[i];
        slices[i] = (int)p.g.slices; tiles[i] = (int)p.g.tiles; sliceRows[i] = (int)p.g.sliceRows; launchOf[i] = (int)p.launch;
    }
    for (uint32_t l = 0; l < plan.nLaunches; l++) {
        const LaunchPlan& lp = plan.launch[l];
        launchPersistent[l] = (int)lp.persistent; launchCutJobs[l] = (int)lp.cutJobs; launchCompact[l] = lp.compact ? 1 : 0; launchStagger[l] = (int)lp.staggerSleeps;
    }
    return (int)plan.nLaunches;
}
// The instantiations that exist, without a context or a device (include/effort_hip_debug.h).
extern "C" int effort_debug_variants(int q4, int* rows, int maxRows) {
    if (maxRows < 0 || (maxRows > 0 && !rows)) return EFFORT_ERR_ARG;
    return bucket_mul_variants(q4 ? kQ4 : kFp16, rows, maxRows);
}
// What launch `launch` of the most recent group ran: host-side record, nothing is read from the device.
extern "C" int effort_debug_last_variant(effort_ctx* c, int launch, int* out8) {
    if (!c || !out8 || launch < 0) return EFFORT_ERR_ARG;
    const Lane& L = c->lane[c->lastLane];
    if ((uint32_t)launch >= L.lastLaunches) return EFFORT_ERR_ARG;
    const LaunchedVariant& v = L.lastVariant[launch];
    const uint32_t w[8] = {v.W, v.E, v.fused, v.compact, v.lean, v.persistent, v.grid, v.totalItems};
    for (int i = 0; i < 8; i++) out8[i] = (int)w[i];
    return EFFORT_OK;
}
extern "C" int effort_group_cutoff(effort_ctx* c, int idx, float* host_out) {
    if (!c || !host_out || idx < 0 || (uint32_t)idx >= c->lane[c->lastLane].lastCalls) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    Lane& L = c->lane[c->lastLane];
    HIP_TRY(c, hipMemcpyAsync(host_out, L.d_cutoff + idx, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EFFORT_OK;
}
extern "C" int effort_last_dispatch_count(effort_ctx* c, uint32_t* host_out) { return effort_group_dispatch_count(c, 0, host_out); }
extern "C" int effort_last_cutoff(effort_ctx* c, float* host_out) { return effort_group_cutoff(c, 0, host_out); }

// ---- dense baseline ------------------------------------------------------------------------------
extern "C" int effort_set_dense_backend(effort_ctx* c, int rocblas) {
    if (!c) return EFFORT_ERR_ARG;
    c->denseRocblas = rocblas != 0;
    return EFFORT_OK;
}
extern "C" int effort_dense_gemv(effort_ctx* c, const void* W, const float* v, float* out, int inDim, int outDim) {
    if (!c || !W || !v || !out || inDim <= 0 || outDim <= 0) return fail(c, EFFORT_ERR_ARG, "dense_gemv: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
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
    { const int grc = grow_scratch(c, c->d_vhalf, c->vhalfElems, (size_t)inDim, (size_t)inDim); if (grc != EFFORT_OK) return grc; }
    HIP_TRY(c, launch_f32_to_f16(v, c->d_vhalf, inDim, c->stream));                  // v.asFloat16(), mps.swift:19
    // W is [outDim][inDim] row-major == column-major inDim x outDim with lda = inDim: y = A^T x
    const float alpha = 1.0f, beta = 0.0f;
    rocblas_status s = rocblas_hssgemv_strided_batched(c->blas, rocblas_operation_transpose, inDim, outDim, &alpha,
                                                       static_cast<const rocblas_half*>(W), inDim, 0,
                                                       reinterpret_cast<const rocblas_half*>(c->d_vhalf), 1, 0, &beta, out, 1, 0, 1);
    if (s != rocblas_status_success) return fail(c, EFFORT_ERR_BLAS, "rocblas_hssgemv_strided_batched");
    return EFFORT_OK;
}
// basicMul on expert *expNo of a stack of cores: always the in-tree kernel (rocBLAS takes its matrix from the host side)
extern "C" int effort_dense_gemv_expert(effort_ctx* c, const void* W, const uint32_t* expNo, const float* v, float* out, int inDim, int outDim,
                                        int numExperts) {
    if (!c || !W || !expNo || !v || !out || inDim <= 0 || outDim <= 0 || numExperts <= 0) return fail(c, EFFORT_ERR_ARG, "dense_gemv_expert: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    if (!dense_gemv_supported((uint32_t)inDim, (uint32_t)outDim) || (size_t)numExperts * outDim * inDim * 2 > 0xFFFFFFFFull)
        return fail(c, EFFORT_ERR_SHAPE, "dense_gemv_expert: inDim % 16 != 0, inDim > 65536, or a stack of 4 GiB or more");
    HIP_TRY(c, launch_dense_gemv_expert(static_cast<const uint16_t*>(W), expNo, v, out, (uint32_t)inDim, (uint32_t)outDim, (uint32_t)numExperts, c->stream));
    return EFFORT_OK;
}

// ---- converter -----------------------------------------------------------------------------------
extern "C" int effort_convert_fp16_pitched(effort_ctx* c, const void* W, int outDim, int inDim, void* buckets, int rowPitchBytes, void* stats, void* probes) {
    if (!c || !W || !buckets || !stats || !probes) return fail(c, EFFORT_ERR_ARG, "convert_fp16: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    // convert.swift:210-215,239 + the 16384-wide limit of the multiply (bucketMul.swift:52)
    if (outDim <= 0 || inDim < kProbes || !(outDim >= kProbes || kProbes % outDim == 0) || outDim > 16384 || inDim > 32000 ||
        outDim % 16 || (outDim / 16) % 4)
        return fail(c, EFFORT_ERR_CONVERT, "convert_fp16: bucketize preconditions violated");
    const int pitch = rowPitchBytes ? rowPitchBytes : outDim / 16 * 2;
    if (pitch < outDim / 16 * 2 || pitch % 8) return fail(c, EFFORT_ERR_CONVERT, "convert_fp16: row pitch must be a multiple of 8 bytes >= 2*cols");   // (the stats pass loads 8 bytes at a time)
    const size_t elems = (size_t)outDim * inDim;
    { const int grc = grow_scratch(c, c->d_convVals, c->convElems, elems, elems); if (grc != EFFORT_OK) return grc; }
    HIP_TRY(c, launch_convert_fp16(static_cast<const uint16_t*>(W), outDim, inDim, static_cast<uint16_t*>(buckets), (uint32_t)pitch / 2u,
                                   static_cast<uint16_t*>(stats), static_cast<uint16_t*>(probes), c->d_convVals, c->d_status, c->stream));
    return EFFORT_OK;
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
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    if (inDim <= 0 || outDim <= 0 || outDim % 32 || (int64_t)inDim * outDim >= (1ll << 32) || !(perc >= 0.0 && perc <= 1.0))
        return fail(c, EFFORT_ERR_CONVERT, "convert_q4: outDim % 32 != 0 (q4_draft.py:299), or a matrix of 2^32 elements or more");
    const int64_t cnt = effort_q4_outlier_count(inDim, outDim, perc);
    if (cnt >= (1ll << 31)) return fail(c, EFFORT_ERR_CONVERT, "convert_q4: 2^31 outliers or more (the candidate sort counts in int)");
    if (cnt > 0 && !outliers) return fail(c, EFFORT_ERR_ARG, "convert_q4: outliers buffer missing");
    hipSetDevice(c->device);
    HIP_TRY(c, launch_convert_q4(static_cast<const uint16_t*>(core2), (uint32_t)inDim, (uint32_t)outDim, (uint32_t)cnt, static_cast<uint16_t*>(buckets),
                                 static_cast<float*>(stats), static_cast<uint16_t*>(probes), static_cast<float*>(outliers), c->numCU, c->stream));
    return EFFORT_OK;
}

extern "C" int effort_cosine(effort_ctx* c, const float* a, const float* b, int n, float* host_out) {
    if (!c || !a || !b || !host_out || n <= 0) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_cosine(a, b, n, c->d_cos, c->stream));
    HIP_TRY(c, hipMemcpyAsync(host_out, c->d_cos, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EFFORT_OK;
}

// ---- decode-loop glue (runNetwork.swift:68-316; kernels in decode.hip) ---------------------------------------
extern "C" int effort_add_rmsnorm_mul(effort_ctx* c, float* h, const float* delta, const void* w, float* out, int n) {
    if (!c || !h || !w || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "add_rmsnorm_mul: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_add_rmsnorm_mul(h, delta, static_cast<const uint16_t*>(w), out, (uint32_t)n, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_rope_kv(effort_ctx* c, const float* xq, const float* xk, const float* xv, float* qOut, float* kCache,
                              float* vCache, const uint32_t* pos, int numHeads, int numHeadsKV, int headDim, int maxTokens, float ropeBase) {
    if (!c || !xq || !xk || !xv || !qOut || !kCache || !vCache || !pos) return fail(c, EFFORT_ERR_ARG, "rope_kv: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    if (numHeads <= 0 || numHeadsKV <= 0 || numHeads % numHeadsKV || headDim < 2 || headDim > 1024 || headDim % 2 || !(ropeBase > 1.0f) || maxTokens <= 0)
        return fail(c, EFFORT_ERR_SHAPE, "rope_kv: bad head geometry");
    HIP_TRY(c, launch_rope_kv(xq, xk, xv, qOut, kCache, vCache, pos, numHeads, numHeadsKV, headDim, ropeBase, (uint32_t)maxTokens, c->d_status + 1, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_attention(effort_ctx* c, const float* q, const float* kCache, const float* vCache, const uint32_t* pos,
                                float* out, int numHeads, int headDim, int maxTokens) {
    if (!c || !q || !kCache || !vCache || !pos || !out) return fail(c, EFFORT_ERR_ARG, "attention: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    if (numHeads <= 0 || maxTokens <= 0 || maxTokens > 8192 || (headDim != 64 && headDim != 128 && headDim != 256))
        return fail(c, EFFORT_ERR_SHAPE, "attention: headDim 64/128/256, maxTokens <= 8192");
    HIP_TRY(c, launch_attention(q, kCache, vCache, pos, out, numHeads, headDim, maxTokens, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_rope_attention(effort_ctx* c, const float* xq, const float* xk, const float* xv, float* kCache, float* vCache,
                                     const uint32_t* pos, float* out, int numHeads, int numHeadsKV, int headDim, int maxTokens, float ropeBase) {
    if (!c || !xq || !xk || !xv || !kCache || !vCache || !pos || !out) return fail(c, EFFORT_ERR_ARG, "rope_attention: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    if (numHeads <= 0 || numHeadsKV <= 0 || numHeads % numHeadsKV || maxTokens <= 0 || maxTokens > 8192 || !(ropeBase > 1.0f) ||
        (headDim != 64 && headDim != 128 && headDim != 256))
        return fail(c, EFFORT_ERR_SHAPE, "rope_attention: headDim 64/128/256, maxTokens <= 8192");
    HIP_TRY(c, launch_rope_attention(xq, xk, xv, kCache, vCache, pos, out, numHeads, numHeadsKV, headDim, maxTokens, ropeBase, c->d_status + 1, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_silu_mul(effort_ctx* c, const float* x1, const float* x3, float* out, int n) {
    if (!c || !x1 || !x3 || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "silu_mul: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_silu_mul(x1, x3, out, (uint32_t)n, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_fetch_row(effort_ctx* c, const void* emb, const uint32_t* id, float* out, int n) {
    if (!c || !emb || !id || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "fetch_row: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_fetch_row(static_cast<const uint16_t*>(emb), id, out, (uint32_t)n, c->stream));
    return EFFORT_OK;
}
// ---- prompt prefill (the block multiply in prefill.hip, the block glue in decode.hip): a block of tokens per call.  pos0 and rows are
// HOST values (prefill is eager, never captured), so every refusal is a return code with nothing enqueued; the values are judged before
// the pointers, the lanes are joined before the launch.
static_assert(EFFORT_PREFILL_MAX_ROWS == 64, "prefill.hip: kPrefillMaxRows, four token tiles of 16");
static bool prefill_rows_ok(int rows) { return rows >= 1 && rows <= EFFORT_PREFILL_MAX_ROWS; }
extern "C" int effort_dense_gemm_rows(effort_ctx* c, const void* W, const float* x, float* out, int inDim, int outDim, int rows) {
    if (inDim <= 0 || outDim <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows: inDim, outDim >= 1, 1 <= rows <= 64");
    if (!dense_gemm_rows_supported((uint32_t)inDim, (uint32_t)outDim))
        return fail(c, EFFORT_ERR_SHAPE, "dense_gemm_rows: inDim % 32 == 0, inDim <= 65536, outDim <= 2^24, W below 4 GiB");
    if (!c || !W || !x || !out) return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    // (a block's worth of both: the next, longer block does not allocate again)
    int grc = grow_scratch(c, c->d_xhRows, c->xhRowsElems, (size_t)rows * inDim, (size_t)EFFORT_PREFILL_MAX_ROWS * inDim);
    if (grc == EFFORT_OK)
        grc = grow_scratch(c, c->d_gemmPart, c->gemmPartFloats, dense_gemm_rows_partial_floats((uint32_t)inDim, (uint32_t)outDim, (uint32_t)rows),
                           dense_gemm_rows_partial_floats((uint32_t)inDim, (uint32_t)outDim, EFFORT_PREFILL_MAX_ROWS));
    if (grc != EFFORT_OK) return grc;
    HIP_TRY(c, launch_dense_gemm_rows(static_cast<const uint16_t*>(W), x, c->d_xhRows, c->d_gemmPart, out, (uint32_t)inDim, (uint32_t)outDim, (uint32_t)rows,
                                      c->stream));
    return EFFORT_OK;
}
extern "C" int effort_dense_gemm_rows_routed(effort_ctx* c, const void* W, int numExperts, const uint32_t* idx2, const float* x, int xPerSlot, float* out,
                                             int inDim, int outDim, int rows) {
    if (inDim <= 0 || outDim <= 0 || numExperts <= 0 || !prefill_rows_ok(rows) || (xPerSlot != 0 && xPerSlot != 1))
        return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows_routed: inDim, outDim, numExperts >= 1, 1 <= rows <= 64, xPerSlot 0 / 1");
    if (!dense_gemm_rows_supported((uint32_t)inDim, (uint32_t)outDim) || numExperts > 64)
        return fail(c, EFFORT_ERR_SHAPE, "dense_gemm_rows_routed: inDim % 32 == 0, inDim <= 65536, outDim <= 2^24, one expert below 4 GiB, numExperts <= 64");
    if (!c || !W || !idx2 || !x || !out) return fail(c, EFFORT_ERR_ARG, "dense_gemm_rows_routed: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    // (grown to a full block's worth whatever xPerSlot and rows are: the w1, w3 and w2 calls of a layer allocate once)
    const size_t xRows = (size_t)(xPerSlot ? 2 : 1) * rows;
    int grc = grow_scratch(c, c->d_xhRouted, c->xhRoutedElems, xRows * inDim, (size_t)2 * EFFORT_PREFILL_MAX_ROWS * inDim);
    if (grc == EFFORT_OK)
        grc = grow_scratch(c, c->d_routedPart, c->routedPartFloats, dense_gemm_rows_routed_partial_floats((uint32_t)inDim, (uint32_t)outDim, (uint32_t)rows),
                           dense_gemm_rows_routed_partial_floats((uint32_t)inDim, (uint32_t)outDim, EFFORT_PREFILL_MAX_ROWS));
    if (grc == EFFORT_OK)
        grc = grow_scratch(c, c->d_routedGroups, c->routedGroupWords, dense_gemm_rows_routed_group_words(), dense_gemm_rows_routed_group_words());
    if (grc != EFFORT_OK) return grc;
    HIP_TRY(c, launch_dense_gemm_rows_routed(static_cast<const uint16_t*>(W), (uint32_t)numExperts, idx2, x, (uint32_t)xPerSlot, c->d_xhRouted, c->d_routedPart,
                                             c->d_routedGroups, out, (uint32_t)inDim, (uint32_t)outDim, (uint32_t)rows, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_moe_route_rows(effort_ctx* c, const float* h, const void* normW, const void* gateW, int n, int numExperts, float* gateOut,
                                     uint32_t* idx2, float* val2, int rows) {
    if (n <= 0 || numExperts <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "moe_route_rows: n, numExperts >= 1, 1 <= rows <= 64");
    if (!moe_route_supported((uint32_t)n, (uint32_t)numExperts))
        return fail(c, EFFORT_ERR_SHAPE, "moe_route_rows: n % 16 == 0, 16 <= n <= 16384, 1 <= numExperts <= 64");
    if (!c || !h || !normW || !gateW || !idx2 || !val2) return fail(c, EFFORT_ERR_ARG, "moe_route_rows: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_moe_route_rows(h, static_cast<const uint16_t*>(normW), static_cast<const uint16_t*>(gateW), (uint32_t)n, (uint32_t)numExperts, gateOut,
                                     idx2, val2, (uint32_t)rows, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_mix2_add_rows(effort_ctx* c, float* h, const float* f, const float* val2, int n, int rows) {
    if (n <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "mix2_add_rows: n >= 1, 1 <= rows <= 64");
    if (!c || !h || !f || !val2) return fail(c, EFFORT_ERR_ARG, "mix2_add_rows: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_mix2_add_rows(h, f, val2, (uint32_t)n, (uint32_t)rows, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_fetch_rows(effort_ctx* c, const void* emb, const uint32_t* ids, float* out, int n, int rows) {
    if (n <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "fetch_rows: n >= 1, 1 <= rows <= 64");
    if (!c || !emb || !ids || !out) return fail(c, EFFORT_ERR_ARG, "fetch_rows: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_fetch_rows(static_cast<const uint16_t*>(emb), ids, out, (uint32_t)n, (uint32_t)rows, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_add_rmsnorm_mul_rows(effort_ctx* c, float* h, const float* delta, const void* w, float* out, int n, int rows) {
    if (n <= 0 || !prefill_rows_ok(rows)) return fail(c, EFFORT_ERR_ARG, "add_rmsnorm_mul_rows: n >= 1, 1 <= rows <= 64");
    if (!c || !h || !w || !out) return fail(c, EFFORT_ERR_ARG, "add_rmsnorm_mul_rows: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_add_rmsnorm_mul_rows(h, delta, static_cast<const uint16_t*>(w), out, (uint32_t)n, (uint32_t)rows, c->stream));
    return EFFORT_OK;
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
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_rope_kv_rows(xq, xk, xv, qOut, kCache, vCache, (uint32_t)pos0, (uint32_t)rows, numHeads, numHeadsKV, headDim, ropeBase, c->stream));
    return EFFORT_OK;
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
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    const hipError_t e = launch(q, kCache, vCache, (uint32_t)pos0, (uint32_t)rows, out, numHeads, headDim, c->stream);
    if (e != hipSuccess) return fail(c, EFFORT_ERR_HIP, name, e);
    return EFFORT_OK;
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
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_top2_softmax(gate, (uint32_t)n, idx2, val2, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_mix2(effort_ctx* c, const float* f0, const float* f1, const float* val2, float* out, int n) {
    if (!c || !f0 || !f1 || !val2 || !out || n <= 0) return fail(c, EFFORT_ERR_ARG, "mix2: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_mix2(f0, f1, val2, out, (uint32_t)n, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_moe_route(effort_ctx* c, const float* h, const void* normW, const void* gateW, int n, int numExperts, float* gateOut,
                                uint32_t* idx2, float* val2) {
    if (!c || !h || !normW || !gateW || !idx2 || !val2) return fail(c, EFFORT_ERR_ARG, "moe_route: null argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    if (n <= 0 || numExperts <= 0 || !moe_route_supported((uint32_t)n, (uint32_t)numExperts))
        return fail(c, EFFORT_ERR_SHAPE, "moe_route: n % 16 == 0, 16 <= n <= 16384, 1 <= numExperts <= 64");
    HIP_TRY(c, launch_moe_route(h, static_cast<const uint16_t*>(normW), static_cast<const uint16_t*>(gateW), (uint32_t)n, (uint32_t)numExperts, gateOut,
                                idx2, val2, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_mix2_add(effort_ctx* c, float* h, const float* f0, const float* f1, const float* val2, int n) {
    if (!c || !h || !f0 || !f1 || !val2 || n <= 0) return fail(c, EFFORT_ERR_ARG, "mix2_add: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_mix2_add(h, f0, f1, val2, (uint32_t)n, c->stream));
    return EFFORT_OK;
}
extern "C" int effort_argmax(effort_ctx* c, const float* logits, int n, uint32_t* idOut, uint32_t* pos, uint32_t* history, int historyLen) {
    if (!c || !logits || !idOut || !pos || n <= 0 || (history && historyLen <= 0)) return fail(c, EFFORT_ERR_ARG, "argmax: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_argmax(logits, (uint32_t)n, idOut, pos, history, (uint32_t)(history ? historyLen : 0), c->d_status + 1, c->stream));
    return EFFORT_OK;
}
// The sampled pick (sample.hip).  The settings are read on the device: a captured step serves every seed, temperature, top-k and top-p.
extern "C" int effort_sample(effort_ctx* c, const float* logits, int n, const effort_sample_params* params, uint32_t* idOut, uint32_t* pos,
                             uint32_t* history, int historyLen, uint32_t* topkIdx, float* topkVal) {
    if (!c || !logits || !params || !idOut || !pos || n <= 0 || (history && historyLen <= 0)) return fail(c, EFFORT_ERR_ARG, "sample: bad argument");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_sample(logits, (uint32_t)n, params, idOut, pos, history, (uint32_t)(history ? historyLen : 0), c->d_status + 1, topkIdx, topkVal,
                             c->stream));
    return EFFORT_OK;
}
extern "C" int effort_topk(effort_ctx* c, const float* logits, int n, int k, uint32_t* idx, float* val) {
    if (!c || !logits || !idx || !val || n <= 0 || k < 1 || k > EFFORT_SAMPLE_MAX_K) return fail(c, EFFORT_ERR_ARG, "topk: bad argument (1 <= k <= 64)");
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, launch_topk(logits, (uint32_t)n, (uint32_t)k, idx, val, c->stream));
    return EFFORT_OK;
}
extern "C" uint32_t effort_sample_bits(uint32_t seedLo, uint32_t seedHi, uint32_t stream, uint32_t pos) { return philox_x0(seedLo, seedHi, stream, pos); }
// Device-side conditions the decode glue could not report through a return code (the position lives in device memory):
// bit 0 = a step ran past the key/value cache or the history buffer (nothing was written there), bit 1 = argmax over NaN
// logits (token 0 returned).  Reads and clears the word.
extern "C" int effort_decode_status(effort_ctx* c, int* host_out) {
    if (!c || !host_out) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, hipMemcpyAsync(host_out, c->d_status + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_status + 1, 0, 4, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EFFORT_OK;
}
// Rows of the last effort_convert_fp16 calls whose bucket 0 overflowed in the literal preBucketize path (zero padding
// tying with real zeros, convert.metal:40-61: the reference drops those elements silently).  Reads and clears the count.
extern "C" int effort_convert_status(effort_ctx* c, int* host_out) {
    if (!c || !host_out) return EFFORT_ERR_ARG;
    { const int jrc = join_lanes(c); if (jrc != EFFORT_OK) return jrc; }
    HIP_TRY(c, hipMemcpyAsync(host_out, c->d_status, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_status, 0, 4, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EFFORT_OK;
}

// ---- tuning / timing -----------------------------------------------------------------------------
extern "C" int effort_set_tuning(effort_ctx* c, int W, int E, int S) {
    if (!c) return EFFORT_ERR_ARG;
    if ((W || E) && !supported(W ? W : 16, E ? E : 1)) return fail(c, EFFORT_ERR_ARG, "set_tuning: unsupported (waves, elems)");
    if (S < 0) return EFFORT_ERR_ARG;
    c->tuneW = W; c->tuneE = E; c->tuneS = S;
    return EFFORT_OK;
}

extern "C" int effort_debug_occupancy(effort_ctx* c, int q4, int W, int E, int ldsBytes) {
    if (!c || !supported(W, E)) return EFFORT_ERR_ARG;
    return bucket_mul_occupancy(q4 ? kQ4 : kFp16, W, E, (size_t)ldsBytes);
}

extern "C" int effort_set_persistent(effort_ctx* c, int wgPerCU) {
    if (!c || wgPerCU < -1 || wgPerCU > 8) return EFFORT_ERR_ARG;
    c->persistent = wgPerCU;
    return EFFORT_OK;
}

extern "C" int effort_debug_hook_lane(effort_ctx* c, int lane) {
    if (!c || lane < 0 || lane >= c->book.nLanes) return EFFORT_ERR_ARG;
    c->lastLane = lane;
    return EFFORT_OK;
}

extern "C" int effort_set_row_reuse(effort_ctx* c, int reuse) {
    if (!c) return EFFORT_ERR_ARG;
    c->rowReuse = reuse != 0;
    return EFFORT_OK;
}

extern "C" int effort_set_split_cutoff(effort_ctx* c, int split) {
    if (!c) return EFFORT_ERR_ARG;
    c->splitCutoff = split != 0;
    return EFFORT_OK;
}

// The device-clock stamps and the per-item trace live in the LAB library only (libeffort_hip_lab.so, -DEFFORT_LAB; csrc/Makefile): the
// shipped kernels carry no stamp code at all.  In the shipped library mode 1 times launches with HIP events alone and modes 2 / 3 are refused.
#ifdef EFFORT_LAB
static constexpr bool kLabBuild = true;
#else
static constexpr bool kLabBuild = false;
#endif
static int lab_only(effort_ctx* c) { return fail(c, EFFORT_ERR_KIND, "device-clock stamps / traces are compiled into libeffort_hip_lab.so only (EFFORT_HIP_LIB=lab)"); }
extern "C" int effort_is_lab_build(void) { return kLabBuild ? 1 : 0; }

extern "C" int effort_enable_kernel_timing(effort_ctx* c, int enable) {
    if (!c) return EFFORT_ERR_ARG;
    if (!kLabBuild && enable >= 2) return lab_only(c);
    if (enable == 1) { int rc = ensure_timing(c); if (rc != EFFORT_OK) return rc; }
    c->timing = enable == 1;      // 1: events + device clock, 2: device clock only (graph-capture safe), 3: 2 + per-item trace
    c->clock = kLabBuild && enable != 0;
    c->trace = kLabBuild && enable == 3;
    if (c->trace) HIP_TRY(c, hipMemsetAsync(c->d_tstamp + kTraceOff, 0, (size_t)kTraceItems * 96, c->stream));
    c->nSamples = 0;
    HIP_TRY(c, hipMemsetAsync(c->d_tstamp, 0, 4096, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_tstamp, 0xFF, 8, c->stream));
    return EFFORT_OK;
}

extern "C" int effort_debug_stamps(effort_ctx* c, unsigned long long* host32) {
    if (!c || !host32) return EFFORT_ERR_ARG;
    if (!kLabBuild) return lab_only(c);
    HIP_TRY(c, hipMemcpyAsync(host32, c->d_tstamp + 8, 192, hipMemcpyDeviceToHost, c->stream));
    unsigned long long lines[32 * 8];
    HIP_TRY(c, hipMemcpyAsync(lines, c->d_tstamp + 64, sizeof(lines), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < 8; i++) { host32[24 + i] = 0; for (int l = 0; l < 32; l++) host32[24 + i] += lines[l * 8 + i]; }   // all-workgroup phase sums
    return EFFORT_OK;
}

extern "C" int effort_debug_trace(effort_ctx* c, unsigned long long* host, int maxRecords) {
    if (!c || !host || maxRecords < 1 || maxRecords > kTraceItems) return EFFORT_ERR_ARG;
    if (!kLabBuild) return lab_only(c);
    HIP_TRY(c, hipMemcpyAsync(host, c->d_tstamp + kTraceOff, (size_t)maxRecords * 64, hipMemcpyDeviceToHost, c->stream));
    // (then, per item, four progress stamps of its streaming phase: wave 0 a quarter / half / three quarters through its rows)
    HIP_TRY(c, hipMemcpyAsync(host + (size_t)maxRecords * 8, c->d_tstamp + kTraceOff + (size_t)kTraceItems * 8, (size_t)maxRecords * 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return EFFORT_OK;
}

extern "C" int effort_kernel_clock(effort_ctx* c, double* mul_us_avg, int* n_launches) {
    if (!c) return EFFORT_ERR_ARG;
    if (!kLabBuild) return lab_only(c);
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(h, c->d_tstamp, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (mul_us_avg) *mul_us_avg = h[3] ? (double)h[2] / (double)h[3] * 1000.0 / c->wallClockKHz : 0.0;
    if (n_launches) *n_launches = (int)h[3];
    HIP_TRY(c, hipMemsetAsync(c->d_tstamp + 2, 0, 16, c->stream));
    return EFFORT_OK;
}

extern "C" int effort_kernel_timing(effort_ctx* c, double* mul_us, double* cutoff_us, double* integrate_us, int* n) {
    if (!c) return EFFORT_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double a = 0, b = 0, d = 0;
    for (int i = 0; i < c->nSamples; i++) {
        float ms;
        HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[4 * i + 0], c->ev[4 * i + 1])); b += ms;   // the one fused kernel
    }
    const int ns = c->nSamples ? c->nSamples : 1;
    if (cutoff_us) *cutoff_us = a * 1000.0 / ns;
    if (mul_us) *mul_us = b * 1000.0 / ns;
    if (integrate_us) *integrate_us = d * 1000.0 / ns;
    if (n) *n = c->nSamples;
    c->nSamples = 0;
    return EFFORT_OK;
}
