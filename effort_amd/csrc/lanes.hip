// The lane scheduler (lanes.h).  Host only: plain data in, plain data out.
#include "lanes.h"

#include "../../include/effort_hip.h"
#include "../../include/effort_hip_debug.h"

namespace effort {

const char* const kLanesPendingBeforeCapture =
    "lanes hold launches enqueued BEFORE this hipGraph capture began: call effort_join (or effort_sync) before beginning the capture";

void LaneBook::Entry::clear() { pending = false; capId = 0; reads.clear(); writes.clear(); }

void LaneBook::reset(int lanes) { nLanes = lanes; nextLane = 0; }

uint32_t LaneBook::pending_lanes() const {
    uint32_t m = 0;
    for (int i = 0; i < nLanes; i++) if (lane[i].pending) m |= 1u << i;
    return m;
}

bool LaneBook::match_capture(unsigned long long now, uint32_t* dropped) {
    for (int i = 0; i < nLanes; i++) {
        Entry& L = lane[i];
        if (!L.pending || L.capId == now) continue;
        if (L.capId == 0) return false;
        L.clear();
        *dropped |= 1u << i;
    }
    return true;
}

bool LaneBook::full() const {
    for (int i = 0; i < nLanes; i++) if (lane[i].reads.size() + lane[i].writes.size() > kMaxRanges) return true;
    return false;
}

static bool overlaps(const Range* a, int na, const std::vector<Range>& b) {
    for (int i = 0; i < na; i++) for (const auto& y : b) if (a[i].lo < y.hi && y.lo < a[i].hi) return true;
    return false;
}
// RAW, WAW or WAR between the launch and what the lane holds.
static bool conflicts(const LaunchRanges& r, const LaneBook::Entry& L) {
    return overlaps(r.rd, r.nrd, L.writes) || overlaps(r.wr, r.nwr, L.writes) || overlaps(r.wr, r.nwr, L.reads);
}
// A range the lane holds already is not recorded twice: a loop that multiplies into the same vectors over and over (the reference's
// timing loop) would otherwise grow the lists to their cap, and every call scan thousands of ranges.
static void add_new(std::vector<Range>& have, const Range* more, size_t n) {
    for (size_t i = 0; i < n; i++) {
        bool seen = false;
        for (const auto& y : have) if (y.lo == more[i].lo && y.hi == more[i].hi) { seen = true; break; }
        if (!seen) have.push_back(more[i]);
    }
}

LanePick LaneBook::pick(const LaunchRanges& r) const {
    LanePick p;
    for (int i = 0; i < nLanes; i++) if (lane[i].pending && conflicts(r, lane[i])) p.hazards |= 1u << i;
    p.lane = p.hazards ? __builtin_ctz(p.hazards) : nextLane;
    if (p.hazards == 1u << p.lane && busyStreak >= 4 && !migrated) {           // a pure chain: one hazard, its own lane
        for (int k = 1; k < nLanes && !p.moved; k++) {
            const int cand = (p.lane + k) % nLanes;
            if (!lane[cand].pending) { p.lane = cand; p.moved = true; }
        }
    }
    return p;
}

uint32_t LaneBook::commit(const LanePick& p, const LaunchRanges& r, unsigned long long capNow, bool forkWaited) {
    Entry& L = lane[p.lane];
    busyStreak = (forkWaited && p.hazards == 1u << p.lane) ? busyStreak + 1 : 0;          // (a dependent chain's link that had to fork)
    if (p.moved) migrated = true;
    if (!p.hazards) nextLane = (nextLane + 1) % nLanes;
    const uint32_t waits = p.hazards & ~(1u << p.lane);
    for (int i = 0; i < nLanes; i++) if (waits >> i & 1u) {
        add_new(L.reads, lane[i].reads.data(), lane[i].reads.size());
        add_new(L.writes, lane[i].writes.data(), lane[i].writes.size());
        lane[i].clear();
    }
    add_new(L.reads, r.rd, (size_t)r.nrd);
    add_new(L.writes, r.wr, (size_t)r.nwr);
    L.pending = true;
    L.capId = capNow;
    return waits;
}

void LaneBook::keep_pending(uint32_t lanes, unsigned long long capNow) {
    for (int i = 0; i < nLanes; i++) if (lanes >> i & 1u) { lane[i].pending = true; lane[i].capId = capNow; }
}

uint32_t LaneBook::join() {
    const uint32_t joined = pending_lanes();
    for (int i = 0; i < nLanes; i++) lane[i].clear();
    busyStreak = 0; migrated = false;
    return joined;
}

}  // namespace effort

using namespace effort;

// The scheduler without a context: the sequence of mul.hip's do_group and ctx.hip's join_lanes with the HIP calls left out.
extern "C" int effort_debug_lanes(int lanes, int nOps, const int64_t* ops, int64_t nWords, int64_t* out) {
    if (lanes < 1 || lanes > kMaxLanes || nOps < 0 || !ops || !out) return EFFORT_ERR_ARG;
    LaneBook B;
    B.reset(lanes);
    int64_t at = 0;
    for (int op = 0; op < nOps; op++, out += EFFORT_LANES_OUT_WORDS) {
        if (at + 5 > nWords) return EFFORT_ERR_ARG;
        const int64_t kind = ops[at], nrd = ops[at + 3], nwr = ops[at + 4];
        const unsigned long long cap = (unsigned long long)ops[at + 1];
        const bool busy = ops[at + 2] != 0;
        if (kind < EFFORT_LANES_LAUNCH || kind > EFFORT_LANES_JOIN || nrd < 0 || nrd > 4 * kMaxGroup || nwr < 0 || nwr > kMaxGroup ||
            at + 5 + 2 * (nrd + nwr) > nWords) return EFFORT_ERR_ARG;
        LaunchRanges r;
        const int64_t* w = ops + at + 5;
        for (int64_t i = 0; i < nrd; i++, w += 2) r.read((const void*)(uintptr_t)w[0], (size_t)(w[1] - w[0]));
        for (int64_t i = 0; i < nwr; i++, w += 2) r.write((const void*)(uintptr_t)w[0], (size_t)(w[1] - w[0]));
        at += 5 + 2 * (nrd + nwr);
        int rc = EFFORT_OK, lane = -1;
        bool joinedFirst = false, forkWaited = false;
        uint32_t joined = 0, waits = 0, dropped = 0;
        const bool laned = kind == EFFORT_LANES_LAUNCH && lanes > 1;
        if (laned) {
            if (!B.match_capture(cap, &dropped)) rc = EFFORT_ERR_ARG;
            else {
                if (B.full()) { joinedFirst = true; joined = B.join(); }      // (the capture rule of the join: passed just above)
                const LanePick p = B.pick(r);
                lane = p.lane;
                forkWaited = cap != 0 || busy;
                waits = B.commit(p, r, cap, forkWaited);
            }
        } else {                                                              // a join, or the join of a launch in a timing mode
            if (B.pending_lanes() && !B.match_capture(cap, &dropped)) rc = EFFORT_ERR_ARG;
            else {
                joined = B.join();
                if (kind != EFFORT_LANES_JOIN) lane = 0;
            }
        }
        out[0] = rc; out[1] = joinedFirst; out[2] = joined; out[3] = lane; out[4] = forkWaited; out[5] = waits;
        out[6] = B.pending_lanes(); out[7] = B.nextLane; out[8] = B.busyStreak; out[9] = B.migrated;
        for (int i = 0; i < kMaxLanes; i++) { out[10 + i] = (int64_t)B.lane[i].reads.size(); out[10 + kMaxLanes + i] = (int64_t)B.lane[i].writes.size(); }
    }
    return at == nWords ? nOps : EFFORT_ERR_ARG;
}
