// Contexts (host.h): create / destroy / stream / sync, the per-device stream and event pools, the lane executor and the setters.
#include <map>
#include <mutex>
#include <vector>

#include "host.h"

using namespace effort;

static constexpr size_t kStampBytes = (size_t)(kTraceOff + kTraceItems * 12) * 8;   // phase stamps + per-item trace records

extern "C" const char* effort_version(void) { return "effort-hip 0.1 (gfx950)"; }
static char g_createErr[256] = "null context";       // effort_last_error(NULL): why the last effort_create failed, if one did
extern "C" const char* effort_last_error(effort_ctx* c) { return c ? c->err : g_createErr; }

static bool lane_alloc(effort_ctx* c, Lane& L) {
    bool ok = hipMalloc(&L.d_cutoff, 512) == hipSuccess && hipMalloc(&L.d_count, 16) == hipSuccess &&
              hipMalloc(&L.d_slabs, c->env.slabBytes) == hipSuccess && hipMalloc(&L.d_counters, effort_ctx::kMaxTiles * 4) == hipSuccess &&
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
    if (hipGetDeviceProperties(&prop, device) == hipSuccess) c->env.numCU = prop.multiProcessorCount;
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
    for (int i = 0; i < kMaxLanes; i++) if (set >> i & 1u) {
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
    for (int i = 0; i < kMaxLanes; i++) if (dropped >> i & 1u) c->lane[i].dirty = false;
    return true;
}
// The context's stream waits for every lane's launches; from here on the context's stream order covers them.
int join_lanes(effort_ctx* c) {
    if (c->book.pending_lanes()) {
        if (!lanes_match_capture(c, capture_of(c->stream))) return EFFORT_ERR_ARG;
        const hipError_t e = wait_for_lanes(c, c->stream, c->book.pending_lanes());
        if (e != hipSuccess) { snprintf(c->err, sizeof(c->err), "join: %s", hipGetErrorString(e)); return EFFORT_ERR_HIP; }    // (the lanes stay pending)
    }
    c->book.join();
    return EFFORT_OK;
}
int choose_lane(effort_ctx* c, LaneChoice& lc, int n, const effort_w* const* ws, const float* const* vs, const uint32_t* const* expNos,
                float* const* outs, const void* const* vAux, const float* const* resids) {
    if (lc.laned) {
        lc.capNow = capture_of(c->stream);
        if (!lanes_match_capture(c, lc.capNow)) return EFFORT_ERR_ARG;
        if (c->book.full()) JOIN_TRY(c);
        for (int i = 0; i < n; i++)
            lc.ranges.call(vs[i], expNos ? expNos[i] : nullptr, vAux ? vAux[i] : nullptr, resids ? resids[i] : nullptr, outs[i], ws[i]->inDim, ws[i]->outDim);
        lc.pick = c->book.pick(lc.ranges);
    } else if (c->book.nLanes > 1) {
        JOIN_TRY(c);                                        // timing modes: one launch at a time, on lane 0
    }
    return EFFORT_OK;
}
int fork_lane(effort_ctx* c, LaneChoice& lc) {
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
    if (!c || lanes < 1 || lanes > kMaxLanes) return EFFORT_ERR_ARG;
    hipSetDevice(c->device);
    JOIN_TRY(c);
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
    c->env.nLanes = c->book.nLanes;                     // (the one place the planner's lane count is written: it follows the book's)
    return EFFORT_OK;
}
extern "C" int effort_join(effort_ctx* c) { return c ? join_lanes(c) : EFFORT_ERR_ARG; }

extern "C" void effort_destroy(effort_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    for (int i = 0; i < kMaxLanes; i++) if (c->lane[i].own) hipStreamSynchronize(c->lane[i].own);
    hipStreamSynchronize(c->stream);
    comm_release(c);
    dense_release(c);
    if (c->ev) { for (int i = 0; i < effort_ctx::kMaxSamples * 2; i++) if (c->ev[i]) hipEventDestroy(c->ev[i]); delete[] c->ev; }
    for (int i = 0; i < kMaxLanes; i++) lane_free(c->device, c->lane[i]);
    pool_put(c->device, c->forkEv);
#define EFFORT_X(T, name) c->name.release();
    EFFORT_CTX_SCRATCH(EFFORT_X)
#undef EFFORT_X
    hipFree(c->d_blockScratch); hipFree(c->d_cos); hipFree(c->d_status); hipFree(c->d_tstamp);
    delete c;
}

extern "C" int effort_set_stream(effort_ctx* c, void* stream) {
    if (!c) return EFFORT_ERR_ARG;
    if (reinterpret_cast<hipStream_t>(stream) != c->stream && join_lanes(c) != EFFORT_OK) return EFFORT_ERR_HIP;   // (the old stream carries the join)
    c->stream = reinterpret_cast<hipStream_t>(stream);
    dense_set_stream(c);
    return EFFORT_OK;
}

extern "C" int effort_sync(effort_ctx* c) {
    if (!c) return EFFORT_ERR_ARG;
    JOIN_TRY(c);
    return HIP_RC(c, hipStreamSynchronize(c->stream));
}

// ---- the setters ---------------------------------------------------------------------------------
extern "C" int effort_set_tuning(effort_ctx* c, int W, int E, int S) {
    if (!c) return EFFORT_ERR_ARG;
    if ((W || E) && !supported(W ? W : 16, E ? E : 1)) return fail(c, EFFORT_ERR_ARG, "set_tuning: unsupported (waves, elems)");
    if (S < 0) return EFFORT_ERR_ARG;
    c->env.tuneW = W; c->env.tuneE = E; c->env.tuneS = S;
    return EFFORT_OK;
}
extern "C" int effort_set_persistent(effort_ctx* c, int wgPerCU) {
    if (!c || wgPerCU < -1 || wgPerCU > 8) return EFFORT_ERR_ARG;
    c->env.persistent = wgPerCU;
    return EFFORT_OK;
}
extern "C" int effort_set_row_reuse(effort_ctx* c, int reuse) {
    if (!c) return EFFORT_ERR_ARG;
    c->rowReuse = reuse != 0;
    return EFFORT_OK;
}
extern "C" int effort_set_split_cutoff(effort_ctx* c, int split) {
    if (!c) return EFFORT_ERR_ARG;
    c->env.splitCutoff = split != 0;
    return EFFORT_OK;
}
extern "C" int effort_debug_hook_lane(effort_ctx* c, int lane) {
    if (!c || lane < 0 || lane >= c->book.nLanes) return EFFORT_ERR_ARG;
    c->lastLane = lane;
    return EFFORT_OK;
}
