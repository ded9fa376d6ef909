// The launch planner (plan.h): columns per lane, slices per call, which calls are cut thin, plain or persistent grid, cutoff jobs,
// compact means and stagger of a group's launches.  Host only, pure: every rule below is a function of PlanEnv and the calls' shapes.
// The rules were measured on MI355X; the comments are the record of why each constant is what it is.
#include <cstring>

#include "../../include/effort_hip.h"
#include "plan.h"

namespace effort {

// ---- launch geometry ----------------------------------------------------------------------------
static uint32_t round8(uint32_t x) { return (x + 7u) / 8u * 8u; }
// The fewest / the most slices of a call: slices of 512 / 128 input rows, the count a multiple of 8.
static uint32_t min_slices(uint32_t inDim) { return round8((inDim + 511u) / 512u); }
static uint32_t max_slices(uint32_t inDim) { return round8((inDim + 127u) / 128u); }
// Column tiles of a call / of the whole group when a lane owns E columns.
static uint32_t tiles_at(const PlanCall& w, int E) { return (w.cols + 64 * E - 1) / (64 * E); }
static uint32_t group_tiles(int n, const PlanCall* ws, int E) {
    uint32_t t = 0;
    for (int i = 0; i < n; i++) t += tiles_at(ws[i], E);
    return t;
}
// A call's item range: a multiple of 8 (item % 8 = the XCD; locate_item).
static uint32_t padded_items(uint32_t tiles, uint32_t slices) { return round8(tiles * slices); }
// The group's items at the fewest slices, each call's range padded to a multiple of 8.
static uint32_t padded_min_items(int n, const PlanCall* ws, int E) {
    uint32_t t = 0;
    for (int i = 0; i < n; i++) t += padded_items(tiles_at(ws[i], E), min_slices(ws[i].inDim));
    return t;
}
// n calls at s slices each are at most ONE item per CU, counted on the padded ranges the XCDs are dealt from; `tiles`: of the call asked about, `allTiles`: of the group.
static bool fits_one_round(const PlanEnv& env, int n, uint32_t tiles, uint32_t allTiles, uint32_t s) {
    const bool same = allTiles == (uint32_t)n * tiles;          // (a mixed group: every call's padding bounded by 7)
    return (same ? (uint32_t)n * padded_items(tiles, s) : allTiles * s + 7u * (uint32_t)n) <= (uint32_t)env.numCU;
}

bool supported(int W, int E) {
#define EFFORT_CASE(w, e) if (W == w && E == e) return true;
    EFFORT_GEOMS(EFFORT_CASE)
#undef EFFORT_CASE
    return false;
}

// Row slices per call when the launch carries `groupSize` calls and a lane owns E columns.  Measured on MI355X
// (tools/lab/tune.py, 4096x4096 .. 14336x4096, 10-100 % effort): a workgroup's life is mostly fixed-latency steps (staging,
// cutoff, selection, hand-off), so FEWER, fatter items win even when they leave CUs idle -- about 3/4 of an item per CU
// for small groups, with slices between 128 and 512 input rows; from 8 calls on, the fattest slices (512 rows).
// Q4 groups of about 10 to 16 calls on a context WITHOUT lanes (one launch on the chip at a time): the launch as ONE round of workgroups -- just
// under two items per CU -- of 64-column tiles and tall slices.  A Q4 item's stream is bound by its CU's LDS atomic pipe, a CU's two workgroups
// run their heads, streams and tails in step (profiles/r06_q4_timelines.txt), and what a launch then costs is one head + the CU's share of the
// atomics + one tail: the unbalanced 384 items of the general rule (E = 2, 8 slices: half the CUs two items, half one) 65.4 us per 16-call
// launch, 480 items (E = 1, 5 slices) 58.3; 12 calls: 57.1 -> 50.2 at 6 slices (profiles/r06_q4_one_round_sweep.txt).  With several launches in
// flight the other launches fill the idle CUs anyway and the tall items only delay them (four in flight: 45.9 against 40.6 us): lanes keep the
// general rule.  Returns the slices per call, or 0 when the rule does not apply (the slices would be taller than two workgroups' LDS allows).
static uint32_t q4_one_round(const PlanEnv& env, uint32_t inDim, uint32_t groupTiles1) {
    if (env.nLanes > 1 || env.tuneS || !groupTiles1) return 0;
    const uint32_t sMin = (inDim + 831u) / 832u;                  // <= 832 rows per slice: 6656 candidate slots, ~78 KB of LDS, two workgroups per CU
    const uint32_t S = (uint32_t)env.numCU * 15u / 8u / groupTiles1;      // 480 items on 256 CUs
    return S >= sMin && S >= 2u ? S : 0u;
}
// Q4 groups of 3 .. 9 calls on a context without lanes: ONE item per CU -- the tallest slices (>= the slices a workgroup's LDS allows) whose items, counted on the
// padded ranges the XCDs are dealt from (a call's range is a multiple of 8; item % 8 is the XCD), still number at most the CUs.  A launch of one round lasts as long
// as its tallest item, and the first item past one per CU shares its CU for the whole launch: 3 calls of 4096x11008 at 8 slices (144 items of 512 rows) 30.2 us,
// 12 slices (216 of 342) 26.2, 14 slices (252 items, 264 padded) 30.9; 6 calls at 8 slices (288 items) 40.1, at 6 (240 padded) 35.5; 8 calls at E = 2 x 8 (192 fat items)
// 43.7, at E = 1 x 5 (256 padded) 39.5; 8 calls of 4096x4096 at E = 2 x 8 (64 items!) 42.5, at E = 1 x 16 (256) 24.8; 5 x (14336 -> 4096) at 32 slices (320 items) 56.5,
// at 24 (240) 37.9 (round 6, third session, profiles/r06_one_round_groups.txt).  Returns the slices per call, or 0 when such a round does not exist.
static uint32_t q4_one_per_cu(const PlanEnv& env, uint32_t inDim, uint32_t tiles1, int n, uint32_t groupTiles1) {
    if (env.nLanes > 1 || env.tuneS || n < 3 || n > 9) return 0;
    const uint32_t sMin = (inDim + 831u) / 832u, hi = max_slices(inDim);
    auto fits = [&](uint32_t s) { return fits_one_round(env, n, tiles1, groupTiles1 ? groupTiles1 : (uint32_t)n * tiles1, s); };
    uint32_t S = sMin > 2u ? sMin : 2u;
    if (!fits(S)) return 0;
    const uint32_t top = env.thinEffort ? min_slices(inDim) : hi;      // (next to nothing to stream: no more slices than the small groups' minimum)
    while (S < top && S < hi && fits(S + 1u)) S++;
    return S;
}
static uint32_t pick_slices(const PlanEnv& env, Format fmt, const PlanCall& w, int groupSize, int E, uint32_t groupTiles = 0, bool fill = true) {
    const uint32_t tiles = tiles_at(w, E);
    const uint32_t lo = min_slices(w.inDim), hi = max_slices(w.inDim);
    if (fmt != kFp16 && (E == 1 || groupSize >= 8) && fill) {       // (8 / 9 calls that do not fit one E = 1 item per CU run at E = 2: one of THOSE per CU then -- 9 x (14336 ->
        const uint32_t S = q4_one_per_cu(env, w.inDim, tiles, groupSize, groupTiles);     //  4096): 32 slices = 288 items 78.4 us, 24 = 216 items 56.1; 9 x (4096 -> 14336): 8 slices 64.4, 6: 54.8)
        if (S) return S;
    }
    if (fmt != kFp16 && E == 1 && groupSize >= 8 && groupTiles) {       // (pick_elems chose E = 1 for this Q4 group: q4_one_round)
        const uint32_t S = q4_one_round(env, w.inDim, groupTiles);
        if (S) return S;
    }
    // Groups of >= 8 calls: the fewest slices (fat items: less fixed work per byte) -- unless the launch then leaves CUs WITHOUT an item: 8 calls on 4096x4096
    // matrices are 8 x 2 tiles x 8 slices = 128 items on 256 CUs.  FP16 groups then take the small groups' rule below (about 3/4 of an item per CU; it
    // never goes under `lo`): 8 x 4096x4096 31.8 -> 24.8 us per launch at 16 slices (32 slices: 28.7; E = 1 x 16: 27.6; E = 4 x 32: 29.7 -- round 6, third
    // session, profiles/r06_small_matrix_groups.txt).  `fill` = false: the count pick_elems prices its choice of E with (unchanged: E is chosen as before).
    if (groupSize >= 8 && (fmt != kFp16 || !fill || env.nLanes > 1 || env.thinEffort)) return lo;     // (with launches in flight on lanes the other launches fill the idle CUs: fat items stay -- 8 x 4096x4096, four in flight: 14.7 us per launch at 8 slices, 15.7 at 16)
    // (64-column tiles -- narrow matrices, see pick_elems -- are worked best at one item per CU: measured, 14336 -> 4096 lone, 64 slices
    //  26.9 us against 29.2 at 48)
    // (Q4 small groups are worked at E = 1 whatever the shape and want the 3/4 too -- round 6, a pair of 4096x11008 calls: 16 slices = 192 items 23.2 us
    //  against 25.4 at the 24 the full-CU target gave; lone and four per launch land on 192 items either way)
    const uint32_t target = (E == 1 && fmt == kFp16) ? (uint32_t)env.numCU : (uint32_t)env.numCU * 3u / 4u;
    // the launch's items come from ALL its calls: with the column tiles of the whole group known (Wq | Wk | Wv: 4 + 1 + 1 at
    // E = 1) every call takes target / tiles slices; without, the calls are taken as equals
    const uint32_t allTiles = groupTiles ? groupTiles : (uint32_t)groupSize * tiles;
    uint32_t S = (target / allTiles + 4u) / 8u * 8u;       // nearest multiple of 8
    if (S < lo) S = lo;
    if (S > hi) S = hi;
    // A slice's candidate slots are laid out per rank in blocks of 2^ceil(log2(rows)): a row count that is not a power of two wastes the
    // rest of the block in staging, selection and LDS (24 slices of a 4096-row input: 171 rows in blocks of 256, a third of the slots
    // empty).  With a power-of-two input the count snaps to the next power of two when the bounds allow.  Round 6 re-sweep of the decode
    // loop's launches and the lone FFN shapes (tools/lab/geosweep.py, profiles/r06_geosweep.txt): every launch was within 0.3 % of its best
    // geometry except the lone 4096 -> 14336 call -- the shape of the reference's own timing loop (benchmarks/benchmark.swift:245-257) --
    // where the rule above gave 24 slices: 20.0 -> 18.6 us at 25 % effort, 25.4 -> 23.4 at 50 %.
    if ((w.inDim & (w.inDim - 1u)) == 0u && (S & (S - 1u)) != 0u) {
        uint32_t up = 8u;
        while (up < S) up <<= 1;
        S = up <= hi ? up : up >> 1;
    }
    // Groups of >= 3 FP16 calls that fit ONE round of CUs: as many slices as keep the launch at one item per CU, any count, instead of the nearest power of two
    // under 3/4 of the CUs.  A launch of one round lasts as long as its tallest item: 3 calls of 4096x11008 at 8 slices are 144 items of 512 rows, at 13 slices
    // 234 of 316 (30.7 -> 25.3 us per launch).  "One item per CU" is counted the way the items are DEALT: a call's item range is padded to a multiple of 8 and item
    // % 8 is the XCD, so each call puts ceil(items / 8) on XCD 0 -- 7 calls of 33 items are 231 items but 35 on XCD 0's 32 CUs, and the launch takes 69 us
    // where 30 items per call take 45 (round 6, third session, profiles/r06_one_round_groups.txt).  Lone calls and pairs -- the decode loop's launches,
    // re-swept in round 6 -- keep the rule above.
    if (fmt == kFp16 && fill && groupSize >= 3 && env.nLanes <= 1) {          // (four launches in flight: 3 calls of 4096x11008 13.4 us per launch at 8 slices, 15.0 at 13)
        auto fits = [&](uint32_t s) { return fits_one_round(env, groupSize, tiles, allTiles, s); };
        if (fits(S)) { if (!env.thinEffort) while (S < hi && fits(S + 1u)) S++; }
        else {      // the rule above went OVER one item per CU (the power-of-two snap: 9 x (8192 -> 4096) 24 -> 32 slices = 288 items, 62.9 us against 46.1 at 24; the `hi`
                    // bound: 9 x (4096 -> 1024) at 32 slices 20.6 us, at 24 18.9): the most slices that fit, if any do
            uint32_t s2 = S;
            while (s2 > lo && !fits(s2)) s2--;
            if (fits(s2)) S = s2;
        }
    }
    return S;
}

// Columns per lane for the whole launch (one kernel variant serves all its calls).  FP16: 2; 1 when a small group would
// otherwise leave most of the chip without an item (small matrices); 4 for groups of >= 8 calls (fewer, fatter items: less
// fixed work per byte) unless that leaves the launch with between one and three items per CU -- half the chip would then
// run two workgroups per CU in lockstep with the other half's one -- or with less than half an item per CU (measured,
// 4096x11008: 8 calls 7.9 vs 8.4 us/call, 16 calls 7.2 vs 6.6, 32 calls 5.7 vs 6.3).  Q4 (a word = 4 sub-buckets): 1, or 2 from 8 calls on.
static int pick_elems(const PlanEnv& env, Format fmt, int n, const PlanCall* ws) {
    if (env.tuneE) return env.tuneE;
    if (fmt != kFp16) {      // measured, 4096x11008 Q4: 32 calls 5.3 vs 6.4 us/call, 8 calls 8.3 vs 8.3, 2 calls 20.8 vs 18.8
        if (n < 8) return 1;
        uint32_t inMax = 0;
        for (int i = 0; i < n; i++) inMax = inMax > ws[i].inDim ? inMax : ws[i].inDim;
        if (n < 10) {        // (8 / 9 calls: one E = 1 item per CU where that fits: q4_one_per_cu)
            uint32_t tMax = 0;
            bool same = true;
            for (int i = 0; i < n; i++) {
                const uint32_t t = tiles_at(ws[i], 1);
                same = same && (tMax == 0 || t == tMax); tMax = tMax > t ? tMax : t;
            }
            if (q4_one_per_cu(env, inMax, tMax, n, same ? 0u : group_tiles(n, ws, 1))) return 1;
        }
        if (n >= 10) {       // (one round of narrow, tall items where that fits: q4_one_round)
            if (q4_one_round(env, inMax, group_tiles(n, ws, 1))) return 1;
        }
        return 2;
    }
    if (env.tuneS) return 2;
    auto items = [&](int E) {
        uint32_t t = 0;
        const uint32_t gt = group_tiles(n, ws, E);
        for (int i = 0; i < n; i++) t += tiles_at(ws[i], E) * pick_slices(env, fmt, ws[i], n, E, gt, false);
        return t;
    };
    const uint32_t numCU = (uint32_t)env.numCU;
    // the 64-column items outnumber the CUs even at the fewest slices (padded item ranges) while the 128-column ones fit one round
    auto only_wide_tiles_fit = [&] { return padded_min_items(n, ws, 1) > numCU && padded_min_items(n, ws, 2) <= numCU; };
    // how much of its column tiles' lanes a choice keeps busy: a narrow handle -- a column shard of a multi-GPU split, 11008
    // outputs over 8 ranks = 86 columns -- fills a third of ONE 256-column tile (E = 4: 22 of 64 lanes), two thirds at E = 2
    auto fill = [&](int E) {
        double used = 0, have = 0;
        for (int i = 0; i < n; i++) { used += ws[i].cols; have += (double)tiles_at(ws[i], E) * 64 * E; }
        return have > 0 ? used / have : 1.0;
    };
    const double f1 = fill(1), f2 = fill(2), f4 = fill(4), best = f1 > f2 ? (f1 > f4 ? f1 : f4) : (f2 > f4 ? f2 : f4);
    if (n >= 8) {
        const uint32_t i4 = items(4);
        if (((i4 > numCU / 2 && i4 <= numCU) || i4 >= 3u * numCU) && f4 >= 0.8 * best) return 4;
        if (f2 >= 0.8 * best) return 2;
        // 64-column tiles because 128-column ones would leave lanes idle (k sequences' Wq | Wk | Wv: 4096 + 1024 + 1024 outputs fill 3/4 of their 128-column tiles) --
        // unless the 64-column items outnumber the CUs at the fewest slices and the 128-column ones do not: a launch of one item per CU at 3/4 lane fill beats a
        // second round (6 / 7 / 8 sequences, 18 / 21 / 24 calls: 37.6 -> 32.7 / 39.3 -> 33.8 / 39.7 -> 34.0 us per launch; 10 sequences overflow either way and stay)
        if (env.nLanes <= 1 && f2 >= 0.7 * best && only_wide_tiles_fit()) return 2;
        return 1;
    }
    const uint32_t i2 = items(2);
    if (f2 < 0.8 * best) return 1;
    // 3..7 calls of BIG matrices whose E = 2 items overflow one round of CUs even at the fewest slices (6 calls of 4096x11008: 6 x 6 tiles x 8 = 288 items, the 32
    // over the 256 CUs run as a round of their own) while E = 4 items fit: E = 4, and pick_slices then fills the round (18 tiles x 13 slices = 234 items)
    if (n >= 3 && f4 >= 0.8 * best && env.nLanes <= 1) {
        uint32_t lo2 = 0, lo4 = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t lo = min_slices(ws[i].inDim);
            lo2 += tiles_at(ws[i], 2) * lo; lo4 += tiles_at(ws[i], 4) * lo;
        }
        if (lo2 > numCU && lo4 <= numCU * 15u / 16u) return 4;
    }
    // narrow matrices (<= 256 bucket columns: 4096 outputs) in small groups: 64-column tiles -- more tiles, each reduced by its
    // own last arriver (measured, us per launch at 25 %: Wq|Wk|Wv 21.2 vs 23.8, 14336 -> 4096 lone 26.6-27.5 vs 29.7)
    bool narrow = true;
    for (int i = 0; i < n; i++) narrow = narrow && ws[i].cols <= 256u;
    // (... for launches that have the chip to themselves, and for lone calls.  GROUPS on a context with lanes -- launches in flight beside one another, the CUs
    //  never short of items -- want the fatter 128-column tiles: four in flight, us per launch E = 1 / E = 2: 14336 -> 4096 x 2 / 3 / 4 / 6 calls 14.7 / 13.0, 21.6 / 16.9,
    //  28.6 / 22.3, 44.6 / 31.7; 4096x4096 x 2 / 3 / 4 / 6: 7.7 / 6.7, 10.9 / 7.8, 10.7 / 10.2, 13.1 / 11.8; lone calls 9.7 / 10.0 and 5.4 / 5.9 -- round 6, third session,
    //  profiles/r06_one_round_groups.txt)
    // ... unless the 64-column tiles overflow ONE round of CUs even at the fewest slices while the 128-column tiles fit it (tall narrow matrices: 3 calls of 11008 -> 4096
    // are 3 x 4 tiles x 24 slices = 288 items, at E = 2 144 -- and pick_slices then fills the round: 35.6 -> 27.9 us per launch, 4 / 5 calls -15 / -7 %, 3 x (14336 -> 4096) -12 %)
    if (narrow && f1 >= 0.8 * best && n >= 3 && env.nLanes <= 1 && f2 >= 0.8 * best && only_wide_tiles_fit()) return 2;
    if (narrow && f1 >= 0.8 * best && !(env.nLanes > 1 && n >= 3)) return 1;      // (pairs keep the lone calls' tiles: -11 % left on the table, and a pair's bits do not depend on the lanes)
    return (i2 * 10u < numCU * 3u / 4u * 6u && items(1) > i2) ? 1 : 2;
}

// Floats of one partial tile.
static uint32_t tile_floats(Format fmt, int E) { return (fmt == kFp16 ? 16u : 32u) * (uint32_t)E * 64u; }
// The geometry of one call of a group of groupSize calls worked by W waves at E columns per lane, at sliceMult x the slices the rules give.
static int choose_geom(const PlanEnv& env, Format fmt, const PlanCall& w, int groupSize, int W, int E, uint32_t groupTiles, uint32_t sliceMult, MulGeom* g) {
    memset(g, 0, sizeof(*g));
    g->inDim = w.inDim; g->outDim = w.outDim; g->cols = w.cols; g->rowsPerIn = w.rowsPerIn;
    g->expertRows = w.rowsPerIn * w.inDim; g->numExperts = w.numExperts;
    g->tiles = tiles_at(w, E);
    g->elems = (uint32_t)E;
    g->rowPitch = w.rowPitch;
    const uint32_t tileFloats = tile_floats(fmt, E);
    const size_t ldsMax = 160 * 1024;
    uint32_t S;
    if (env.tuneS) S = env.tuneS;                            // any count: the item grid is padded to a multiple of 8 slices
    else {
        const uint32_t want = pick_slices(env, fmt, w, groupSize, E, groupTiles) * sliceMult;
        const uint32_t cap = (env.numCU * 2u) / g->tiles / 8 * 8;              // one round of workgroups
        S = cap < want ? cap : want;
    }
    if (S > w.inDim) S = w.inDim / 8 * 8;
    if (S < 1) S = 1;
    const uint32_t maxCand = bucket_mul_max_candidates(W);
    for (;;) {
        g->sliceRows = (w.inDim + S - 1) / S;
        g->slices = (w.inDim + g->sliceRows - 1) / g->sliceRows;
        g->sliceLog2 = 0; while ((1u << g->sliceLog2) < g->sliceRows) g->sliceLog2++;
        g->slots = fmt == kFp16 ? (g->rowsPerIn << g->sliceLog2) : g->sliceRows * 8u;
        const size_t lds = bucket_mul_lds_bytes(fmt, W, E, *g, true);    // (whether the launch will be a lean plain grid is known only once all its calls are: budget for the larger plan, the lean one's)
        const bool fits = lds <= ldsMax && g->slots <= maxCand && (size_t)g->slots * 4 + (size_t)g->sliceRows * 8 + 1024 <= 65536 &&   // staged regions below 64 KB
                          (fmt == kFp16 ? (1u << g->sliceLog2) <= 64u * (uint32_t)W : g->sliceRows <= 128u * (uint32_t)W);   // a thread stages one (Q4: two) inputs of the slice
        const size_t slab = (size_t)g->slices * g->tiles * tileFloats * 4;
        if (fits && slab <= env.slabBytes) break;
        if (!fits) { S += 1; if (S > w.inDim + 8) return EFFORT_ERR_SHAPE; }
        else return EFFORT_ERR_SHAPE;
    }
    return EFFORT_OK;
}
static int plan_fail(GroupPlan* P, int code, const char* msg) { P->err = code; P->msg = msg; return code; }

// Index of g among the n shapes of a launch, appended when it is new; kMaxGeoms: it is new and the launch is full.
static uint32_t geom_index(MulGeom* geoms, uint32_t& n, const MulGeom& g) {
    uint32_t k = 0;
    while (k < n && memcmp(&geoms[k], &g, sizeof(g)) != 0) k++;
    if (k == n && n < (uint32_t)kMaxGeoms) geoms[n++] = g;
    return k;
}

// The launch's grid and what goes with it, once its calls are known: one kernel launch for the calls gathered in *lp.
static void finish_launch(Format fmt, const PlanEnv& env, int W, const PlanCall* ws, const GroupPlan* P, LaunchPlan* lp) {
    // grid: persistent workgroups once the items outnumber what the chip holds at R per CU
    const uint32_t R = env.persistent < 0 ? 2u : (uint32_t)env.persistent;
    // FP16 on a context WITHOUT lanes -- one launch on the chip at a time -- stays a PLAIN grid: the lean kernel (half the
    // instructions, every workgroup evaluates its cutoff at once instead of awaiting a job), and the dispatcher hands the third round of workgroups
    // to whichever CU frees a slot.  Round 6, 4096x11008, us per launch persistent -> plain: 12 calls 80.0 -> 74.9, 16: 89.9 -> 87.4, 20: 111.9 -> 103.2,
    // 16 at 50 % effort 157.6 -> 145.8, 16 x (4096 -> 14336) 108.9 -> 101.8, 24 / 32 calls level (122.2 / 122.4, 153.0 / 152.2), 32 at 10 % +2 %;
    // with four launches in flight the persistent grid wins (16 calls 66.9 against 67.6, 32: 127.2 against 130.1): lanes keep it from 2 per CU on
    // (profiles/r06_plain_vs_persistent.txt).
    // (1024 items -- 32 calls of 4096 -> 14336 -- 205.4 -> 197.7; 1536 -- 32 calls at E = 2 -- plain 0.98 x the heuristic's launch where persistent was 1.04 x:
    //  plain up to six items per CU, as far as was measured)
    const uint32_t perCU = (env.persistent < 0 && fmt == kFp16 && !env.laned) ? 6u : R;
    lp->persistent = (R && lp->realItems > (uint32_t)env.numCU * perCU) ? R : 0u;      // (the items that exist, not the padded item range)
    // persistent launches evaluate every call's cutoff ONCE, in a job of its own at the head of the item queues, instead
    // of once per workgroup and call (measured: 6.8 of the ~90 us of an item at 32 calls per launch)
    bool plain = true;
    for (uint32_t i = 0; i < lp->count; i++) plain = plain && !ws[lp->first + i].pre;
    lp->cutJobs = (lp->persistent && !env.splitCutoff && plain && !env.noJobs) ? (lp->count + 7u) / 8u * 8u : 0u;
    // FP16: the multiply stages the compact row means where every slice starts on an even row (an LDS-direct load lands two):
    // a quarter of the lines of the 8-byte stats entries, half the loads.  Persistent launches, and the plain grids the lean
    // instantiation serves (8 waves, no stamps): with the path a template parameter it costs them no code (as a run-time
    // switch inside one kernel it cost lone calls 3 %); measured on plain grids: decode 298 -> 300 tokens/s.
    const bool leanGrid = lp->persistent == 0u && W == 8 && !env.clock && !env.ablate;      // (launch_mul_t's condition for the lean instantiations)
    bool compact = fmt == kFp16 && !env.noCompact && (leanGrid || (lp->persistent != 0u && plain));    // lean: with prologues / residuals too
    for (uint32_t i = 0; compact && !leanGrid && i < lp->count; i++) compact = !ws[lp->first + i].hasResid;
    for (uint32_t i = 0; compact && i < lp->count; i++) {
        const MulGeom& g = P->call[lp->first + i].g;
        compact = ws[lp->first + i].hasMeans16 && g.inDim % 2u == 0u && g.sliceRows % 2u == 0u;
    }
    lp->compact = compact;
    // Persistent Q4 launches of a context WITHOUT lanes -- one launch on the chip at a time -- start the second workgroup of every CU ~10 us late,
    // which takes a CU's pair out of step (bucket_mul_kernel; profiles/r06_ab_q4_stagger.txt: 32 calls per launch 109.5 -> 99.8 us).  With lanes the
    // launches overlap, the CUs are busy anyway and the wait is a loss (2-5 %): off.  FP16 launches are bound by the CU's pull from memory, not
    // by an LDS pipe, and their pairs fall out of step by themselves (the older workgroup wins the arbitration two to one): measured, no gain
    // (profiles/r06_ab_fp16_stagger.txt): off.
    lp->staggerSleeps = (lp->persistent && fmt == kQ4 && !env.laned) ? 11u : 0u;
}

int plan_group(Format fmt, const PlanEnv& env, int n, const PlanCall* ws, GroupPlan* P) {
    P->err = EFFORT_OK; P->msg = ""; P->nLaunches = 0;
    const bool laned = env.laned;
    const int W = env.tuneW ? env.tuneW : 8;            // 8 waves per workgroup
    const int E = pick_elems(env, fmt, n, ws);          // columns per lane: one choice for a group launch
    P->W = W; P->E = E;
    const char* const noGeometry = "bucketmul: no launch geometry for this shape/tuning";
    if (!supported(W, E)) return plan_fail(P, EFFORT_ERR_ARG, noGeometry);
    const uint32_t groupTiles = group_tiles(n, ws, E);
    // every call's geometry at the slices the rules give (g1) -- what the thin-call rule prices the launch with and all but the thin calls keep
    MulGeom g1[kMaxGroup], g2[kMaxGroup];               // (g2: at twice the slices, of the thin calls alone)
    uint32_t it1[kMaxGroup], base = 0;                  // the calls' padded item ranges, and their sum
    for (int i = 0; i < n; i++) {
        const int rc = choose_geom(env, fmt, ws[i], n, W, E, groupTiles, 1, &g1[i]);
        if (rc != EFFORT_OK) return plan_fail(P, rc, noGeometry);
        it1[i] = padded_items(g1[i].tiles, g1[i].slices);
        base += it1[i];
    }
    // Thin slices for the LAST TWO calls of an FP16 launch whose last round of workgroups would be nearly empty (round 6, third session;
    // profiles/r06_tail_slices.txt).  A plain grid's workgroups are handed out in call order, two per CU at a time: 11 calls of 48 items are 528 items --
    // one round of 512 and 16 stragglers that start when the others END, a whole item's duration for 3 % of the work.  With the last two calls cut into twice the
    // slices the tail of the launch is made of half-height items: the first of them finish while the round is still running and hand their slots on.  us per
    // launch, 4096x11008 at 25 %, without / with the rule: 11 calls 72.8 -> 66.0 (-9.4 %), 12: 74.5 -> 69.3 (-7 %), 22: 114.2 -> 108.4 (-5 %), 23: 115.6 -> 110.9
    // (-4 %), 12 at 10 / 50 / 100 % effort -5.7 / -9.1 / -11.5 %, 11 at 100 % -13.7 %, 19 x (4096 -> 14336) -4.8 %, 11 x (4096 -> 14336) -6 %.  The gain shrinks as
    // the last round fills -- 13 calls (112 of 512 slots) -2.5 %, 24 calls or 18 x (14336 -> 4096) (128) 0 / +3 % -- so the rule ends at 7/32 of a round.  Applied
    // to EVERY mid-size launch (its first form) it was level or worse from a quarter-full last round on: 14 / 15 calls +2 / +3 %, 16 at 50 / 100 % effort +2.5 /
    // +4.5 %, 16 calls of a 4096x4096 matrix (256 items: not even one round) +12 %.  More than
    // two thin calls, or four times the slices: never better (a thin item pays the same head and hand-off for half the rows); E = 4 launches (32 calls: 149.0 ->
    // 150.8), persistent grids (151 -> 157) and launches in flight on lanes (a launch's tail runs under the next one's head; round 2: 124.3 -> 125.8): worse, off.
    // HOW MANY calls: enough that the thin calls' items cover the stragglers (the items past the last whole round), at least two, at most four -- 24 Q4 calls of 24
    // items are 64 over a round: two thin calls (48 items) 93.7 -> 92.6 us, four (96) 86.3.  Q4 (E = 2 launches past one round of two workgroups per CU are PERSISTENT
    // grids on a context without lanes: the queue hands the items out in call order just the same): 22 / 24 calls of 4096x11008 93.0 -> 84.9 / 93.7 -> 86.3 us, 17 / 18 x
    // (4096 -> 14336) 90.0 -> 83.1 / 91.0 -> 83.8, 24 calls at 50 % effort 139.6 -> 128.7; 26 calls (112 over) level.
    int thinFrom = n;                                     // calls [thinFrom, n) take twice the slices
    if (E == 2 && n >= 8 && !laned && !env.tuneS && env.persistent < 0 && !env.thinEffort) {
        const uint32_t round = 2u * (uint32_t)env.numCU, over = base % round;
        // (FP16 stays a plain grid up to six items per CU; Q4 past one round is a persistent grid whatever its size)
        if (base > round && over != 0u && over * 32u <= round * 7u && (fmt != kFp16 || base <= 6u * (uint32_t)env.numCU)) {
            int tc = 0;
            uint32_t thin = 0;
            while (tc < n && tc < 4 && (tc < 2 || thin < over)) thin += it1[n - 1 - tc++];
            // the thin geometries: they must exist (more slices than the call has) and fit the launch descriptor's kMaxGeoms shapes beside the others
            MulGeom seen[kMaxGeoms];
            uint32_t nSeen = 0, extra = 0;
            bool ok = thin >= over;
            for (int i = 0; ok && i < n; i++) {
                const bool t = i >= n - tc;
                if (t) {
                    ok = choose_geom(env, fmt, ws[i], n, W, E, groupTiles, 2, &g2[i]) == EFFORT_OK;
                    const uint32_t it2 = padded_items(g2[i].tiles, g2[i].slices);
                    ok = ok && it2 > it1[i];
                    extra += it2 - it1[i];
                }
                ok = ok && geom_index(seen, nSeen, t ? g2[i] : g1[i]) < (uint32_t)kMaxGeoms;
            }
            if (ok && (fmt != kFp16 || base + extra <= 6u * (uint32_t)env.numCU)) thinFrom = n - tc;
        }
    }
    uint32_t nGeoms = 0, wg = 0;
    MulGeom geoms[kMaxGeoms];                             // the shapes of the launch being gathered
    size_t slabOff = 0; uint32_t tileOff = 0, sliceOff = 0;
    LaunchPlan* lp = nullptr;
    auto begin = [&](uint32_t firstCall) {
        lp = &P->launch[P->nLaunches++];
        memset(lp, 0, sizeof(*lp));
        lp->first = firstCall;
        nGeoms = 0; wg = 0;
    };
    begin(0);
    for (int i = 0; i < n; i++) {
        // the calls at the END of a mid-size group are cut into thinner slices (thinFrom, above): their items are the last ones handed out, and
        // the launch ends when the last item does
        uint32_t mult = i >= thinFrom ? 2u : 1u;
        MulGeom g = mult == 2u ? g2[i] : g1[i];
        if (n >= 8 && !env.tuneS && env.tailMult) {       // lab knobs: the rule above replaced by "the last tailCalls calls at tailMult x the slices"
            mult = 1;
            if (i >= n - env.tailCalls) mult = (uint32_t)env.tailMult;
            if (env.tailMult >= 4 && i >= n - env.tailCalls && i < n - env.tailCalls / 2) mult = (uint32_t)env.tailMult / 2;      // two steps: ... x2 x2 x4 x4
            const int rc = choose_geom(env, fmt, ws[i], n, W, E, groupTiles, mult, &g);
            if (rc != EFFORT_OK) return plan_fail(P, rc, noGeometry);
        }
        uint32_t gi = geom_index(geoms, nGeoms, g);
        if (gi == (uint32_t)kMaxGeoms) {                  // a launch carries kMaxGeoms distinct shapes: this call opens the next one
            finish_launch(fmt, env, W, ws, P, lp);
            begin((uint32_t)i);
            gi = geom_index(geoms, nGeoms, g);
        }
        CallPlan& a = P->call[i];
        const size_t slab = (size_t)g.slices * g.tiles * tile_floats(fmt, E) * 4;
        if (tileOff + g.tiles + 1 > env.maxTiles || sliceOff + g.slices > env.maxSlices || slabOff + slab > env.slabBytes)
            return plan_fail(P, EFFORT_ERR_SHAPE, "bucketmul: group exceeds the context scratch");
        a.g = g; a.mult = mult; a.launch = P->nLaunches - 1u; a.geom = gi;
        a.slabOff = (uint32_t)(slabOff / 256); a.tileOff = tileOff; a.sliceOff = sliceOff;
        wg += padded_items(g.tiles, g.slices);
        if (wg / 8u > 0xFFFFu) return plan_fail(P, EFFORT_ERR_SHAPE, "bucketmul: group exceeds the launch descriptor's item range");
        a.itemEnd8 = wg / 8u;
        lp->count = (uint32_t)i - lp->first + 1u;
        lp->totalItems = wg; lp->totalTiles += g.tiles; lp->realItems += g.tiles * g.slices;
        slabOff += (slab + 255) / 256 * 256; tileOff += g.tiles; sliceOff += g.slices;
    }
    finish_launch(fmt, env, W, ws, P, lp);
    return EFFORT_OK;
}

}  // namespace effort
