// The multiply's executor: a group's launches as the planner cut them (plan.hip) on the lane the scheduler chose (ctx.hip), its entry points,
// the queries about the last launch and about the planner, and the timing hooks.  The one host unit that reads EFFORT_LAB.
#include <cstdlib>

#include "host.h"

using namespace effort;

// ---- launch planning: the inputs of plan_group (plan.hip) ------------------------------------------
// `env`: the persistent settings (a context's, or effort_debug_plan's); what belongs to the call is filled in here.
static PlanEnv call_env(PlanEnv env, bool laned, bool thinEffort) {
    env.laned = laned; env.thinEffort = thinEffort;
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
        if (pre && c->env.splitCutoff) return fail(c, EFFORT_ERR_KIND, "bucketmul: input prologues need the fused cutoff");
        // Q4: the outlier phase needs the whole TRANSFORMED input and keeps it in LDS; beyond that copy's size it gathers v from memory, where a prologue's
        // input does not exist (bucket_mul.hip, phase O).  A residual alone, or a handle without outliers, works at any size.
        if (pre && fmt == kQ4 && ws[i]->olBlockPtr && (uint32_t)ws[i]->inDim > bucket_mul_ol_lds_floats())
            return fail(c, EFFORT_ERR_SHAPE, "bucketmul: an input prologue on a Q4 handle with outliers needs inDim <= 16384 (materialise the input, or register without outliers)");
        pc[i] = plan_call(ws[i], pre, resids && resids[i]);
    }
    LaneChoice lc;
    lc.laned = c->book.nLanes > 1 && !c->timing && !c->env.clock;
    const PlanEnv env = call_env(c->env, lc.laned, thin_effort(n, efforts));
    GroupPlan plan;
    if (plan_group(fmt, env, n, pc, &plan) != EFFORT_OK) return fail(c, plan.err, plan.msg);
    const bool tm = c->timing && c->nSamples < effort_ctx::kMaxSamples;
    hipEvent_t* ev = tm ? c->ev + 2 * c->nSamples : nullptr;
    OK_TRY(choose_lane(c, lc, n, ws, vs, expNos, outs, vAux, resids));
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
        ga.tstamp = env.clock ? c->d_tstamp : nullptr;
        ga.ablate = env.ablate; ga.trace = (env.clock && c->trace) ? 1u : 0u;
        ga.split = (env.splitCutoff ? 1u : 0u) | (lp.compact ? 4u : 0u) | (c->rowReuse ? 8u : 0u);
        ga.numCU = (uint32_t)env.numCU; ga.queue = L.d_queue;
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
        OK_TRY(fork_lane(c, lc));
        if (env.splitCutoff && !(env.ablate & 1u)) HIP_TRY(c, launch_find_cutoff_group(ga, st));
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
    JOIN_TRY(c);
    Lane& L = c->lane[0];
    c->lastLane = 0;
    const PlanCall pc = plan_call(w, 0, false);
    GroupPlan plan;
    if (plan_group(w->fmt, call_env(c->env, false, false), 1, &pc, &plan) != EFFORT_OK) return fail(c, plan.err, "calc_dispatch: geometry");
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
    JOIN_TRY(c);
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
    JOIN_TRY(c);
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
    if (numCU < 1 || lanes < 1 || lanes > kMaxLanes || n < 1 || n > kMaxGroup || !inDim || !outDim || !effort || !we || !slices || !tiles ||
        !sliceRows || !launchOf || !launchPersistent || !launchCutJobs || !launchCompact || !launchStagger) return EFFORT_ERR_ARG;
    const Format fmt = q4 ? kQ4 : kFp16;
    PlanEnv env = effort_ctx::scratch_env();           // (a context's defaults)
    env.numCU = numCU; env.nLanes = lanes; env.persistent = persistent; env.tuneW = tuneW; env.tuneE = tuneE; env.tuneS = tuneS;
    PlanCall pc[kMaxGroup];
    for (int i = 0; i < n; i++) {
        const int load = q4 ? 8 : (percentLoad ? percentLoad[i] : 16);
        if (inDim[i] <= 0 || outDim[i] <= 0 || check_shape((uint32_t)inDim[i], (uint32_t)outDim[i]) != EFFORT_OK || load < 1 || load > 16) return EFFORT_ERR_SHAPE;
        if (!(effort[i] >= 0.0 && effort[i] <= 1.0)) return EFFORT_ERR_EFFORT;
        const uint32_t cols = (uint32_t)outDim[i] / (q4 ? 32u : 16u);
        pc[i] = PlanCall{(uint32_t)inDim[i], (uint32_t)outDim[i], cols, (uint32_t)load, cols * 2u, 1u, !q4, (uint16_t)(prologue ? prologue[i] : 0), hasResid && hasResid[i]};
    }
    GroupPlan plan;
    const int rc = plan_group(fmt, call_env(env, lanes > 1, thin_effort(n, effort)), n, pc, &plan);
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
extern "C" int effort_debug_occupancy(effort_ctx* c, int q4, int W, int E, int ldsBytes) {
    if (!c || !supported(W, E)) return EFFORT_ERR_ARG;
    return bucket_mul_occupancy(q4 ? kQ4 : kFp16, W, E, (size_t)ldsBytes);
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
    JOIN_TRY(c);
    Lane& L = c->lane[c->lastLane];
    HIP_TRY(c, hipMemcpyAsync(host_out, L.d_cutoff + idx, 4, hipMemcpyDeviceToHost, c->stream));
    return HIP_RC(c, hipStreamSynchronize(c->stream));
}
extern "C" int effort_last_dispatch_count(effort_ctx* c, uint32_t* host_out) { return effort_group_dispatch_count(c, 0, host_out); }
extern "C" int effort_last_cutoff(effort_ctx* c, float* host_out) { return effort_group_cutoff(c, 0, host_out); }

// ---- timing --------------------------------------------------------------------------------------
// The device-clock stamps and the per-item trace live in the LAB library only (libeffort_hip_lab.so, -DEFFORT_LAB; csrc/Makefile): the
// shipped kernels carry no stamp code at all.  In the shipped library mode 1 times launches with HIP events alone and modes 2 / 3 are refused.
#ifdef EFFORT_LAB
static constexpr bool kLabBuild = true;
#else
static constexpr bool kLabBuild = false;
#endif
static int lab_only(effort_ctx* c) { return fail(c, EFFORT_ERR_KIND, "device-clock stamps / traces are compiled into libeffort_hip_lab.so only (EFFORT_HIP_LIB=lab)"); }
extern "C" int effort_is_lab_build(void) { return kLabBuild ? 1 : 0; }

static int ensure_timing(effort_ctx* c) {
    if (c->ev) return EFFORT_OK;
    c->ev = new (std::nothrow) hipEvent_t[effort_ctx::kMaxSamples * 2]();       // (value-initialised: effort_destroy walks the whole array)
    if (!c->ev) return EFFORT_ERR_HIP;
    for (int i = 0; i < effort_ctx::kMaxSamples * 2; i++) HIP_TRY(c, hipEventCreate(&c->ev[i]));
    return EFFORT_OK;
}
extern "C" int effort_enable_kernel_timing(effort_ctx* c, int enable) {
    if (!c) return EFFORT_ERR_ARG;
    if (!kLabBuild && enable >= 2) return lab_only(c);
    if (enable == 1) OK_TRY(ensure_timing(c));
    c->timing = enable == 1;      // 1: events + device clock, 2: device clock only (graph-capture safe), 3: 2 + per-item trace
    c->env.clock = kLabBuild && enable != 0;
    c->trace = kLabBuild && enable == 3;
    if (c->trace) HIP_TRY(c, hipMemsetAsync(c->d_tstamp + kTraceOff, 0, (size_t)kTraceItems * 96, c->stream));
    c->nSamples = 0;
    HIP_TRY(c, hipMemsetAsync(c->d_tstamp, 0, 4096, c->stream));
    return HIP_RC(c, hipMemsetAsync(c->d_tstamp, 0xFF, 8, c->stream));
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
    return HIP_RC(c, hipStreamSynchronize(c->stream));
}

extern "C" int effort_kernel_clock(effort_ctx* c, double* mul_us_avg, int* n_launches) {
    if (!c) return EFFORT_ERR_ARG;
    if (!kLabBuild) return lab_only(c);
    unsigned long long h[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpyAsync(h, c->d_tstamp, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (mul_us_avg) *mul_us_avg = h[3] ? (double)h[2] / (double)h[3] * 1000.0 / c->wallClockKHz : 0.0;
    if (n_launches) *n_launches = (int)h[3];
    return HIP_RC(c, hipMemsetAsync(c->d_tstamp + 2, 0, 16, c->stream));
}

// The one fused kernel is all a sample times: the separate cutoff and integrate kernels are gone, and their figures are reported as 0.
extern "C" int effort_kernel_timing(effort_ctx* c, double* mul_us, double* cutoff_us, double* integrate_us, int* n) {
    if (!c) return EFFORT_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double b = 0;
    float ms;
    for (int i = 0; i < c->nSamples; i++) { HIP_TRY(c, hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1])); b += ms; }
    const int ns = c->nSamples ? c->nSamples : 1;
    if (cutoff_us) *cutoff_us = 0.0;
    if (mul_us) *mul_us = b * 1000.0 / ns;
    if (integrate_us) *integrate_us = 0.0;
    if (n) *n = c->nSamples;
    c->nSamples = 0;
    return EFFORT_OK;
}
