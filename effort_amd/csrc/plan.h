// The launch planner: the shape of a group's multiply launches as a PURE function of plain data -- no context, no weight handle,
// no stream, no HIP runtime call, no environment.  mul.hip gathers the inputs (do_group), plan.hip decides, mul.hip copies the
// plan and the pointers into the launch descriptor.  effort_debug_plan (include/effort_hip_debug.h) runs it without a device.
#pragma once
#include "effort_internal.h"

namespace effort {

constexpr int kMaxLaunches = kMaxGroup / kMaxGeoms + 1;     // a group splits where a call brings the (kMaxGeoms + 1)-th shape of a launch

struct PlanEnv {
    int numCU = 256, nLanes = 1;
    bool laned = false;               // the launch goes to a lane of its own: lanes > 1 and no timing / clock mode
    int persistent = -1;              // workgroups per CU of group launches: -1 heuristic, 0 plain grid, R > 0 persistent
    int tuneW = 0, tuneE = 0, tuneS = 0;      // tuning overrides (0 = heuristic)
    bool splitCutoff = false, clock = false;
    uint32_t ablate = 0;              // lab switches (EFFORT_LAB builds: read from the environment by mul.hip)
    bool noJobs = false, noCompact = false;
    size_t slabBytes = 0;             // a lane's scratch: partial tiles, arrival tickets, per-slice counts
    uint32_t maxTiles = 0, maxSlices = 0;
    bool thinEffort = false;          // the launch being cut streams next to nothing (mean effort under 8 %): the rules that RAISE the slice count of a group stand down
                                      // (at 2 % effort 3 / 6 / 8 calls of 4096x11008 at 13 / 13 / 10 slices are 9 / 14 / 10 % SLOWER
                                      // than at 8 -- more slabs and heads, nothing to stream -- where at 10 % they are 6 / 5 / 0 % faster and at 100 % 28 / 28 / 6 %)
    int tailCalls = 0, tailMult = 0;  // lab: the thin-call rule replaced by "the last tailCalls calls at tailMult x the slices" (tailMult 0 = off)
};
struct PlanCall {                     // the shape fields of a weight handle and what the call asks of the kernel
    uint32_t inDim, outDim, cols, rowsPerIn, rowPitch, numExperts;
    bool hasMeans16;
    uint16_t pre;                     // Prologue
    bool hasResid;
};
struct CallPlan {
    MulGeom g;
    uint32_t mult;                    // slice multiplier (2: a thin call at the end of a mid-size launch)
    uint32_t launch, geom;            // its launch, and its shape's index among that launch's
    uint32_t slabOff, tileOff, sliceOff;      // where it lives in the lane's scratch (slabOff in units of 64 floats)
    uint32_t itemEnd8;                // exclusive end of its item range within the launch, in units of 8 items
};
struct LaunchPlan {
    uint32_t first, count;            // its calls: [first, first + count)
    uint32_t persistent, cutJobs, staggerSleeps;
    bool compact;                     // FP16: the calls stage the compact row means
    uint32_t totalItems, totalTiles, realItems;
};
struct GroupPlan {
    int W = 0, E = 0;
    int err = 0;                      // EFFORT_OK, or why there is no plan
    const char* msg = "";
    uint32_t nLaunches = 0;
    CallPlan call[kMaxGroup];
    LaunchPlan launch[kMaxLaunches];
};

bool supported(int W, int E);        // the (waves per workgroup, columns per lane) pairs the multiply kernel is built for
// Fills *plan for the n calls of one group; returns plan->err.
int plan_group(Format fmt, const PlanEnv& env, int n, const PlanCall* calls, GroupPlan* plan);

}  // namespace effort
