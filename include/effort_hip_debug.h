/*
 * effort_hip_debug.h -- profiling, tracing and A/B hooks of libeffort_hip.so.  NOT part of the drop-in boundary
 * (include/effort_hip.h): nothing in the reference corresponds to these; the bench, the tools/ scripts and a few tests
 * use them.  They may change between builds.
 */
#ifndef EFFORT_HIP_DEBUG_H
#define EFFORT_HIP_DEBUG_H

#include "effort_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Tuning knobs (nothing in the reference corresponds to them; the tests pin launch geometries with them). */
/* Override the launch geometry heuristics of the multiply kernel: waves per workgroup (4, 8 or 16),
 * elements per lane (1, 2 or 4) and number of row slices (0 = heuristic).  Returns EFFORT_ERR_ARG
 * for unsupported combinations. */
EFFORT_API int effort_set_tuning(effort_ctx* ctx, int wavesPerGroup, int elemsPerLane, int rowSlices);
/* split = 1: evaluate findCutoff32 in its own one-workgroup launch ahead of the multiply kernel instead of
 * inside it.  Costs a kernel boundary per call.  Results are bit-identical.  Default 0 (fused). */
EFFORT_API int effort_set_split_cutoff(effort_ctx* ctx, int split);

/* Group launches with more work items than wgPerCU workgroups per CU run as that many PERSISTENT workgroups pulling
 * items from per-XCD queues.  -1 = heuristic (default), 0 = always one workgroup per item. */
EFFORT_API int effort_set_persistent(effort_ctx* ctx, int wgPerCU);

/* Overlap mode (effort_set_overlap): the hooks effort_group_dispatch_count / effort_group_cutoff / effort_debug_slice_counts
 * read the lane the most recent launch went to; this points them at another lane's last launch (0 .. lanes-1). */
EFFORT_API int effort_debug_hook_lane(effort_ctx* ctx, int lane);

/* 1 in libeffort_hip_lab.so (built with -DEFFORT_LAB: device-clock stamps, per-item trace, ablation switches, environment knobs), 0 in the
 * shipped libeffort_hip.so, whose kernels carry none of that: there enable = 2 / 3 below, effort_kernel_clock, effort_debug_stamps and
 * effort_debug_trace return EFFORT_ERR_KIND, and enable = 1 records HIP events only. */
EFFORT_API int effort_is_lab_build(void);
/* Timing hooks.  enable = 1: HIP events are recorded on the context's stream around each launch (not capturable into a
 * graph) AND the multiply kernel stamps the device wall clock at its first workgroup's start / last workgroup's end;
 * enable = 2: device clock only (works inside hipGraph replays); 3: 2 plus a per-item trace (effort_debug_trace); 0: off.
 * effort_kernel_timing returns event-to-event averages in microseconds (they include the launch gap in front of each
 * kernel); effort_kernel_clock returns the multiply kernel's own average duration (first start -> last end).  Both
 * reset their accumulators. */
EFFORT_API int effort_enable_kernel_timing(effort_ctx* ctx, int enable);
EFFORT_API int effort_kernel_clock(effort_ctx* ctx, double* mul_us_avg, int* n_launches);
EFFORT_API int effort_kernel_timing(effort_ctx* ctx, double* mul_us_avg, double* cutoff_us_avg,
                         double* integrate_us_avg, int* n_samples);
/* resident workgroups per CU the runtime grants the (q4, waves, elems) multiply kernel at ldsBytes of LDS */
EFFORT_API int effort_debug_occupancy(effort_ctx* ctx, int q4, int waves, int elems, int ldsBytes);
/* 24 raw u64 phase stamps written by the most recent cutoff / multiply kernels in timing mode. */
EFFORT_API int effort_debug_stamps(effort_ctx* ctx, unsigned long long* host32);
/* Kept rows per row slice of call idx of the most recent (group) launch (their sum is dispatch.size); returns the
 * number of slices copied (<= maxSlices), or a negative error code. */
EFFORT_API int effort_debug_slice_counts(effort_ctx* ctx, int idx, uint32_t* host, int maxSlices);
/* The launch planner on its own (csrc/plan.hip: plan_group), for the n calls of one group on a device of numCU compute units and a context of
 * `lanes` lanes: no context, no device, no HIP call -- it runs on a machine without a GPU.  Per call: inDim, outDim, percentLoad (FP16; NULL = 16,
 * ignored for q4), prologue (EFFORT_PRE_*; NULL = none), hasResid (NULL = none), effort (the launch is "thin" when their mean is under 8 %, as in
 * the multiply calls).  persistent / tuneW / tuneE / tuneS: effort_set_persistent / effort_set_tuning (-1, 0, 0, 0 = the heuristics).
 * Fills we[2] = {waves per workgroup, columns per lane}; per call [n]: slices, tiles, sliceRows, launchOf (the launch the call went to: a group
 * splits when it holds more than four shapes); per launch [n]: persistent workgroups per CU (0: plain grid), cutoff jobs, compact-means bit,
 * stagger sleeps.  Returns the number of launches, or the negative error code the multiply call would return. */
EFFORT_API int effort_debug_plan(int q4, int numCU, int lanes, int n, const int* inDim, const int* outDim, const int* percentLoad,
                      const int* prologue, const int* hasResid, const double* effort, int persistent, int tuneW, int tuneE, int tuneS,
                      int* we, int* slices, int* tiles, int* sliceRows, int* launchOf,
                      int* launchPersistent, int* launchCutJobs, int* launchCompact, int* launchStagger);
/* What registration answers for a bundle's SIZES alone -- effort_weights_fp16_pitched (q4 = 0) / effort_weights_q4 (q4 = 1: percentLoad is
 * ignored, rowPitchBytes must be 0) -- before it reads or allocates anything: EFFORT_OK or EFFORT_ERR_SHAPE.  The limits of effort_hip.h
 * ("weights"): the shape rule, and every per-row array of the stack below 4 GiB.  No context, no device, no HIP call. */
EFFORT_API int effort_debug_check_bundle(int q4, int inDim, int outDim, int percentLoad, int numExperts, int rowPitchBytes);
/* The instantiations of the multiply kernel that exist for a format (q4 = 0: FP16), as rows of five ints {waves per workgroup, columns per
 * lane, fused (prologue / residual), compact (FP16: compact row means), lean (the plain-grid instantiation)}: the list the device preparation
 * and the launch selection walk (bucket_mul.hip: EFFORT_GEOMS x each_variant).  No context, no device, no HIP call.  Fills at most maxRows rows
 * (rows may be NULL with maxRows = 0) and returns the number that exist. */
EFFORT_API int effort_debug_variants(int q4, int* rows, int maxRows);
/* What launch `launch` (0 .. launches - 1; a group splits when it holds more than four shapes) of the most recent multiply group of the hooked
 * lane ran, as the launcher recorded it on the host: out8 = {waves, columns per lane, fused, compact, lean, persistent workgroups per CU (0: a
 * plain grid), grid size in workgroups, items of the launch (without cutoff jobs)}.  EFFORT_ERR_ARG when the group had no such launch. */
EFFORT_API int effort_debug_last_variant(effort_ctx* ctx, int launch, int* out8);
/* The lane scheduler on its own (csrc/lanes.hip: LaneBook, what effort_set_overlap's launches are ordered by): a script of nOps operations
 * played through a fresh book of `lanes` lanes -- no context, no device, no HIP call.  `ops` is nWords int64 words, per operation
 *   kind (EFFORT_LANES_*), capture id of the context's stream (0: not capturing), 1 if that stream answers "busy" / 0 if idle, nRead, nWrite,
 *   then nRead and nWrite address ranges as (lo, hi) pairs -- what the launch reads and writes (a join or a timed launch: none).
 * EFFORT_LANES_LAUNCH is a multiply launch, EFFORT_LANES_TIMED one in a timing / clock mode (the lanes are joined, lane 0), EFFORT_LANES_JOIN
 * an effort_join.  `out` receives EFFORT_LANES_OUT_WORDS words per operation:
 *   [0] the return code of the call; [1] 1 if the lanes were joined first because a lane's book was full; [2] the lanes the context's stream
 *   waited for (a join, a timed launch, or [1]; sets of lanes are bit masks, bit i = lane i); [3] the launch's lane (-1: none); [4] 1 if the
 *   lane's fork waited for the context's stream (busy, or capturing); [5] the lanes the launch's lane waited for;
 *   the state afterwards: [6] the pending lanes, [7] the next round-robin lane, [8] the busy streak, [9] 1 if a chain moved since the last join,
 *   [10..13] ranges read and [14..17] ranges written that each lane holds.
 * Returns nOps, or EFFORT_ERR_ARG for a malformed script. */
#define EFFORT_LANES_LAUNCH 0
#define EFFORT_LANES_TIMED 1
#define EFFORT_LANES_JOIN 2
#define EFFORT_LANES_OUT_WORDS 18
EFFORT_API int effort_debug_lanes(int lanes, int nOps, const int64_t* ops, int64_t nWords, int64_t* out);
/* enable = 3 (device clock + trace): every work item of the most recent multiply launch leaves a 64-byte record
 * {item | workgroup << 32 (bit 63: cutoff job), XCC_ID | HW_ID << 32, six device wall-clock stamps: start, staged,
 * cutoff, selected, streamed, handed over}; copies the first maxRecords (<= 4096) records to host (8 u64 each), followed
 * by 4 u64 per item: the device clock when wave 0 was a quarter, half and three quarters through its rows (host must
 * hold 12 * maxRecords u64). */
EFFORT_API int effort_debug_trace(effort_ctx* ctx, unsigned long long* host, int maxRecords);

#ifdef __cplusplus
}
#endif
#endif /* EFFORT_HIP_DEBUG_H */
