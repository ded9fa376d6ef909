// The lane scheduler: which lane of a context a multiply launch goes to, which lanes it must follow, when the lanes are joined and when a
// chain of dependent launches changes lanes -- as a host-only unit of plain data: no stream, no event, no HIP runtime call, no context, no
// environment.  ctx.hip asks (capture rule, full?, pick), issues the HIP calls the answers call for, and reports back (commit, join);
// effort_debug_lanes (include/effort_hip_debug.h) plays a script of operations through a fresh book without a device.
//
// The rules.  A launch may run beside the launches in flight on the OTHER lanes unless it reads or writes what one of them writes, or writes
// what one of them reads (RAW / WAW / WAR on address ranges); then it goes to the first such lane -- a lane's stream is in order -- and waits
// for the others, whose ranges it takes over: from there on its lane's order covers theirs, and they are no longer pending.  Without a
// hazard the lanes are dealt round-robin.  Every launch is also ordered after what was enqueued on the context's stream before it: the fork,
// which the executor skips when that stream is idle.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "effort_internal.h"

namespace effort {

constexpr int kMaxLanes = 4;
// address ranges a lane records between joins: a caller may enqueue arbitrarily many multiplies before its one eval()
// (helpers/gpu.swift:109-119); a book past this is JOINED -- the context's stream waits for every lane, later launches fork from it --
// never forgotten
constexpr size_t kMaxRanges = 1024;
// (the refusal of LaneBook::match_capture, as the caller reads it)
extern const char* const kLanesPendingBeforeCapture;

struct Range { uintptr_t lo, hi; };

// What one group launch reads and writes.
struct LaunchRanges {
    Range rd[4 * kMaxGroup], wr[kMaxGroup];
    int nrd = 0, nwr = 0;
    static void add(Range* list, int& n, const void* p, size_t bytes) { if (p && bytes) list[n++] = Range{(uintptr_t)p, (uintptr_t)p + bytes}; }
    void read(const void* p, size_t bytes) { add(rd, nrd, p, bytes); }
    void write(const void* p, size_t bytes) { add(wr, nwr, p, bytes); }
    // One call of the group (null: the call has none).
    void call(const void* v, const void* expNo, const void* vAux, const void* resid, const void* out, uint32_t inDim, uint32_t outDim) {
        read(v, (size_t)inDim * 4);
        read(expNo, 4);
        read(vAux, (size_t)inDim * 4);
        read(resid, (size_t)outDim * 4);
        write(out, (size_t)outDim * 4);
    }
};

// Sets of lanes are bit masks (bit i: lane i); the executor walks them in ascending order.
struct LanePick {
    int lane = 0;
    uint32_t hazards = 0;             // the pending lanes the launch conflicts with
    bool moved = false;               // a chain that leaves its lane (see LaneBook::pick)
};

struct LaneBook {
    struct Entry {
        bool pending = false;         // launches enqueued since the last join that nothing waited for yet
        unsigned long long capId = 0; // the hipGraph capture they were enqueued in (0: none -- real work on the lane's queue)
        std::vector<Range> reads, writes;         // what they read / write: each range once
        void clear();
    };
    Entry lane[kMaxLanes];
    int nLanes = 1, nextLane = 0;
    int busyStreak = 0;               // consecutive links of a dependent chain whose fork had to wait
    bool migrated = false;            // ... and the chain was moved to another lane for it (once between joins)

    void reset(int lanes);            // effort_set_overlap: nothing pending (the caller joined)
    uint32_t pending_lanes() const;
    // Lanes and hipGraph captures.  A lane's pending launches are either real work on its queue or nodes of ONE capture, the one its fork
    // edge came from.  `now`: the capture the context's stream is in (0: none).  (a) real work pending while the stream captures: the
    // capture would have to wait on an event recorded outside it, which stream capture forbids -- false, nothing changed: the caller
    // joins BEFORE beginning the capture (kLanesPendingBeforeCapture); (b) nodes of a capture that has ended, or of another one: the
    // graph's own edges order them -- the lanes are dropped from the book and returned in *dropped.
    bool match_capture(unsigned long long now, uint32_t* dropped);
    bool full() const;                // some lane holds more than kMaxRanges ranges: the caller joins, then picks
    // The lane of a launch.  A chain of dependent launches lives on ONE lane and forks from the context's stream only when that stream is
    // busy.  HIP multiplexes streams over a few hardware queues, and a lane that shares its queue with the context's stream makes that
    // stream answer "busy" while the LANE works: every link then pays the fork (+8 us per call).  Four busy answers in a row on a pure
    // chain (one hazard, its own lane) and the chain MOVES to the first idle lane after it -- one cross-lane edge, the ordinary hazard
    // wait -- where the stream's answer is its own again.  Once between joins: if the answers were true nothing is lost but that edge.
    LanePick pick(const LaunchRanges& r) const;
    // The launch is going to `p.lane`, forked from the context's stream (forkWaited: that stream was busy, or capturing).  Returns the
    // lanes the chosen lane must wait for: their ranges move to it and they are no longer pending.
    uint32_t commit(const LanePick& p, const LaunchRanges& r, unsigned long long capNow, bool forkWaited);
    // A wait commit() asked for could not be enqueued: those lanes stay pending, so that a later join covers them.
    void keep_pending(uint32_t lanes, unsigned long long capNow);
    // The context's stream waits for the returned lanes; from here on its order covers them and the book is empty.
    uint32_t join();
};

}  // namespace effort
