"""The lane scheduler (effort_amd/csrc/lanes.hip: LaneBook, what orders the launches of effort_set_overlap) through effort_debug_lanes, on a
machine without a GPU: the hook needs no context and no device.

(a) literal cases, derived by hand from the rules (lanes.h), on four lanes;
(b) tests/golden/lane_table.json: every field the hook reports over the scripts of (a) and seeded random ones.  The table was recorded
    from the scheduler as it was MOVED out of api.hip (the host layer, since split: its executor is ctx.hip), before any simplification, and is never regenerated from later code: a rule edit
    shows here as a diff of the operations it moves, and the table changes only together with the rule;
(c) the ordering property, which needs no recording: under a happens-before model of the streams, every launch is ordered after every
    earlier launch it conflicts with (RAW, WAW or WAR on overlapping ranges), and a join orders the context's stream after everything.
"""
import json
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "lane_table.json")
ERR_ARG = -1
MAX_RANGES = 1024                   # lanes.h: kMaxRanges


@pytest.fixture(scope="module")
def lanes(hip_lib_built):
    from effort_amd import runtime
    return runtime.lanes


def buf(k, part=None):
    """The address range of buffer k (16 KiB, 64 KiB apart), or of its lower / upper half."""
    lo = 0x7F0000000000 + k * 0x10000
    return {None: (lo, lo + 0x4000), 0: (lo, lo + 0x2000), 1: (lo + 0x2000, lo + 0x4000)}[part]


V, X, Y, Z, W, K = (buf(k) for k in range(6))


def launch(reads, writes, busy=False, cap=0):
    return ("launch", cap, busy, list(reads), list(writes))


def join(cap=0):
    return ("join", cap)


# ---------------------------------------------------------------- the happens-before model of (c)
def conflicts(a, b):
    """Launch b after launch a: b reads or writes what a writes, or writes what a reads."""
    hit = lambda p, q: any(x[0] < y[1] and y[0] < x[1] for x in p for y in q)
    (ar, aw), (br, bw) = a, b
    return hit(br, aw) or hit(bw, aw) or hit(bw, ar)


def check_order(ops, res, n_lanes):
    """Walks a script and its report.  A frontier is the set of launches a stream's next work is ordered after.  A launch inherits the
    context's stream's frontier (an idle stream's earlier work is complete, so whether or not the fork waited) and that of every lane it
    is reported to wait for; a join gives the joined lanes' frontiers to the context's stream.  Returns the launches checked."""
    ctx, lane = set(), [set() for _ in range(n_lanes)]
    done = {}                                               # launch -> (reads, writes)
    for i, (op, r) in enumerate(zip(ops, res)):
        if r["rc"] != 0:
            continue                                        # refused: nothing was enqueued
        for j in r["joined"]:
            ctx |= lane[j]
        if op[0] == "launch" and n_lanes > 1:
            mine = lane[r["lane"]]
            mine |= ctx
            for j in r["waits"]:
                mine |= lane[j]
            me = (op[3], op[4])
            for e in set(done) - mine:
                assert not conflicts(done[e], me), (i, e, r)
            mine.add(i)
            done[i] = me
        else:
            assert set(done) <= ctx, (i, sorted(set(done) - ctx))
            if op[0] != "join":                             # a launch in a timing mode: on the context's stream itself
                ctx.add(i)
                done[i] = ((), ())
    return len(done)


# ---------------------------------------------------------------- (a) literal cases
def chain_link(i, busy, cap=0):
    """Link i of a pure chain: ping-pong through X / Y."""
    return launch([X if i % 2 == 0 else Y], [Y if i % 2 == 0 else X], busy, cap)


def script_round_robin():
    return [launch([buf(2 * i)], [buf(2 * i + 1)]) for i in range(5)]


def script_six_launch_chain():
    """test_gpu_overlap.py::test_overlap_orders_dependent_launches, the same buffers as ranges."""
    return [launch([V], [X]),                               # x = A v
            launch([V], [Y]),                               # y = B v          (independent of the first)
            launch([X], [Z]),                               # z = B x          (RAW on x)
            launch([Y], [V]),                               # v = A y          (WAR on v: launches 1, 2 read it; RAW on y)
            launch([Z], [X]),                               # x = A z          (WAW on x, WAR vs launch 3; RAW on z)
            launch([V, X], [W, Y]),                         # RAW on v and x, WAW on y
            join()]


def script_two_hazards():
    return [launch([V], [X]), launch([V], [Y]), launch([X, Y], [Z]), launch([Y], [W]), join()]


def script_migration():
    ops = [chain_link(i, True) for i in range(12)]          # link 0 starts the chain; links 1..4 are the four busy answers
    ops.append(join())
    ops += [chain_link(i, True) for i in range(7)]
    return ops


def script_no_migration_when_idle():
    return [chain_link(i, False) for i in range(12)]


def script_no_migration_without_an_idle_lane():
    ops = [launch([buf(10 + i)], [buf(20 + i)]) for i in range(3)]          # lanes 0, 1, 2
    ops += [chain_link(i, True) for i in range(8)]                          # the chain: lane 3
    return ops


def script_no_migration_with_two_hazards():
    ops = [launch([V], [Z], True)]                                          # lane 0
    ops += [chain_link(i, True) for i in range(5)]                          # lane 1, four busy links
    ops.append(launch([Y, Z], [X], True))                                   # the chain's next link also reads z: two hazards
    return ops


def script_capture():
    return [launch([V], [X]),                               # real work on lane 0
            launch([X], [Y], cap=7), join(cap=7),           # refused inside a capture
            join(),                                         # the remedy
            launch([X], [Y], cap=7), launch([V], [Z], cap=7),       # lanes 1 and 2 hold nodes of capture 7
            launch([Y], [W]), join(),                       # the capture has ended: dropped, no wait (RAW on y, whose writer was dropped)
            launch([V], [X], cap=7),                        # lane 0, capture 7
            launch([X], [Y], cap=8), launch([V], [Z], cap=8), join(cap=8),  # another capture: dropped
            launch([V], [X], cap=7), join()]                # a join outside the capture drops too


def script_repeats():
    return [launch([V], [X]) for _ in range(5000)]


def script_full_book():
    """Distinct addresses, 16 reads and 8 writes a launch; then a launch that overwrites what the very first one read."""
    ops = [launch([buf(100 + 24 * i + k) for k in range(16)], [buf(100 + 24 * i + 16 + k) for k in range(8)]) for i in range(200)]
    ops.append(launch([K], [buf(100)]))
    return ops


def script_timed():
    return [launch([V], [X]), launch([V], [Y]), ("timed", 0), launch([X], [Z]), join()]


def field(res, name):
    return [r[name] for r in res]


def test_independent_launches_go_round_robin(lanes):
    res = lanes(script_round_robin())
    assert field(res, "lane") == [0, 1, 2, 3, 0] and all(r["waits"] == () and r["rc"] == 0 for r in res)
    assert res[-1]["pending"] == (0, 1, 2, 3) and res[-1]["nextLane"] == 1


def test_the_six_launch_chain(lanes):
    res = lanes(script_six_launch_chain())
    assert field(res, "lane") == [0, 1, 0, 0, 0, 0, -1]
    assert field(res, "waits") == [(), (), (), (1,), (), (), ()]
    assert field(res, "pending") == [(0,), (0, 1), (0, 1), (0,), (0,), (0,), ()]
    assert res[-1]["joined"] == (0,) and res[-1]["reads"] == [0] * 4 and res[-1]["writes"] == [0] * 4
    assert not any(field(res, "fork_waited")) and not any(field(res, "joined_first"))


def test_a_launch_with_two_hazards_takes_the_second_lane_over(lanes):
    res = lanes(script_two_hazards())
    assert field(res, "lane") == [0, 1, 0, 0, -1]
    assert field(res, "waits") == [(), (), (1,), (), ()]             # the later reader of y follows lane 0 only
    assert res[2]["pending"] == (0,) and res[2]["reads"] == [3, 0, 0, 0] and res[2]["writes"] == [3, 0, 0, 0]
    assert res[-1]["joined"] == (0,)


def test_a_busy_chain_moves_once_between_joins(lanes):
    res = lanes(script_migration())
    first, second = res[:12], res[13:]
    assert field(first, "lane") == [0] * 5 + [1] * 7                  # the call after the fourth consecutive busy link
    assert field(first, "busyStreak") == [0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 5, 6]
    assert field(first, "waits") == [()] * 5 + [(0,)] + [()] * 6
    assert field(first, "migrated") == [False] * 5 + [True] * 7
    assert first[5]["pending"] == (1,) and first[5]["reads"][0] == 0
    assert res[12]["joined"] == (1,) and not res[12]["migrated"] and res[12]["busyStreak"] == 0
    assert field(second, "lane") == [1] * 5 + [2] * 2                 # round-robin went on at lane 1; the chain moves again after the join
    assert field(second, "waits") == [()] * 5 + [(1,)] + [()]


def test_a_chain_stays_when_it_should(lanes):
    res = lanes(script_no_migration_when_idle())
    assert field(res, "lane") == [0] * 12 and field(res, "busyStreak") == [0] * 12 and not any(field(res, "migrated"))
    res = lanes(script_no_migration_without_an_idle_lane())
    assert field(res, "lane") == [0, 1, 2] + [3] * 8 and not any(field(res, "migrated")) and res[-1]["busyStreak"] == 7
    res = lanes(script_no_migration_with_two_hazards())
    assert field(res, "lane") == [0] + [1] * 5 + [0] and res[5]["busyStreak"] == 4
    assert res[-1]["waits"] == (1,) and not res[-1]["migrated"] and res[-1]["busyStreak"] == 0


def test_captures(lanes):
    res = lanes(script_capture())
    state = lambda r: {k: r[k] for k in ("pending", "nextLane", "busyStreak", "migrated", "reads", "writes")}
    assert field(res, "rc") == [0, ERR_ARG, ERR_ARG] + [0] * 11
    assert state(res[1]) == state(res[0]) and state(res[2]) == state(res[0]) and res[1]["lane"] == res[2]["lane"] == -1
    assert res[3]["joined"] == (0,)
    assert (res[4]["lane"], res[4]["fork_waited"], res[4]["waits"]) == (1, True, ())       # the same launch goes through
    assert res[5]["pending"] == (1, 2)
    assert (res[6]["lane"], res[6]["waits"], res[6]["joined"], res[6]["pending"]) == (3, (), (), (3,))
    assert res[6]["reads"] == [0, 0, 0, 1] and res[7]["joined"] == (3,)
    assert (res[8]["lane"], res[8]["pending"]) == (0, (0,))
    assert (res[9]["lane"], res[9]["waits"], res[9]["joined"], res[9]["pending"]) == (1, (), (), (1,))
    assert res[11]["joined"] == (1, 2) and res[11]["pending"] == ()
    assert (res[12]["lane"], res[12]["pending"]) == (3, (3,))
    assert (res[13]["rc"], res[13]["joined"], res[13]["pending"], res[13]["reads"]) == (0, (), (), [0] * 4)


def test_repeated_launches_keep_the_book_small(lanes):
    res = lanes(script_repeats())
    assert all(r["reads"] == [1, 0, 0, 0] and r["writes"] == [1, 0, 0, 0] and r["lane"] == 0 for r in res)


def test_a_full_book_joins_and_keeps_the_order(lanes):
    ops = script_full_book()
    res = lanes(ops)
    assert sum(field(res, "joined_first")) >= 1
    assert max(r + w for x in res for r, w in zip(x["reads"], x["writes"])) <= MAX_RANGES + 24
    assert check_order(ops, res, 4) == len(ops)
    full = next(r for r in res if r["joined_first"])
    assert full["joined"] == (0, 1, 2, 3) and full["waits"] == ()


def test_a_timed_launch_joins_and_takes_lane_0(lanes):
    res = lanes(script_timed())
    assert (res[2]["rc"], res[2]["lane"], res[2]["joined"], res[2]["pending"]) == (0, 0, (0, 1), ())
    assert res[3]["lane"] == 2 and res[3]["waits"] == () and res[4]["joined"] == (2,)


# ---------------------------------------------------------------- seeded random scripts
def random_script(seed, n_ops, caps=(0,), timed=False):
    """Groups of 1..3 calls over 6..12 buffers (whole, or a half), random busy answers, a join about every 20th operation.  `caps`: the
    capture ids the script walks through (a change about every 40th operation)."""
    rng = random.Random(seed)
    n_buf = rng.randint(6, 12)
    pick = lambda: buf(rng.randrange(n_buf), rng.choice((None, None, None, 0, 1)))
    cap, ops = caps[0], []
    for _ in range(n_ops):
        if len(caps) > 1 and rng.random() < 1 / 40:
            cap = rng.choice(caps)
        x = rng.random()
        if x < 1 / 20:
            ops.append(join(cap))
        elif timed and x < 1 / 20 + 1 / 50:
            ops.append(("timed", cap))
        else:
            reads, writes = [], []
            for _ in range(rng.randint(1, 3)):              # a call: v, sometimes aux / resid, out
                reads.append(pick())
                if rng.random() < 0.2:
                    reads.append(pick())
                writes.append(pick())
            ops.append(launch(reads, writes, rng.random() < 0.5, cap))
    ops.append(join(cap))
    return ops


# ---------------------------------------------------------------- (b) the golden table
LITERAL = [script_round_robin, script_six_launch_chain, script_two_hazards, script_migration, script_no_migration_when_idle,
           script_no_migration_without_an_idle_lane, script_no_migration_with_two_hazards, script_capture, script_repeats, script_full_book,
           script_timed]


def table_scripts():
    """(key, lanes, ops)"""
    for fn in LITERAL:
        yield fn.__name__[len("script_"):], 4, fn()
    for n_lanes in (2, 3, 4):
        for caps in ((0,), (5,), (0, 7, 8)):
            for seed in range(3):
                yield f"random lanes={n_lanes} caps={'/'.join(map(str, caps))} seed={seed}", n_lanes, random_script(1000 * n_lanes + seed, 100, caps, timed=True)
    yield "random lanes=1", 1, random_script(77, 40, (0,), timed=True)


def rows(res):
    """Run-length over the operations: [[count, [rc, joinedFirst, joined, lane, forkWaited, waits, pending, nextLane, busyStreak, migrated,
    reads per lane, writes per lane]], ...]; sets of lanes as bit masks."""
    mask = lambda lanes_: sum(1 << i for i in lanes_)
    out = []
    for r in res:
        row = [r["rc"], int(r["joined_first"]), mask(r["joined"]), r["lane"], int(r["fork_waited"]), mask(r["waits"]), mask(r["pending"]),
               r["nextLane"], r["busyStreak"], int(r["migrated"]), r["reads"], r["writes"]]
        if out and out[-1][1] == row:
            out[-1][0] += 1
        else:
            out.append([1, row])
    return out


def test_golden_table(lanes):
    want = json.load(open(TABLE))["scripts"]
    seen = 0
    for key, n_lanes, ops in table_scripts():
        assert key in want, key
        got = rows(lanes(ops, lanes=n_lanes))
        assert len(got) == len(want[key]), key
        for i, (a, b) in enumerate(zip(got, want[key])):
            assert a == b, (key, i, a, b)
        seen += 1
    assert seen == len(want)


# ---------------------------------------------------------------- (c) the ordering property
@pytest.mark.parametrize("cap", [0, 5])
def test_every_conflicting_launch_is_ordered(lanes, cap):
    checked = 0
    for seed in range(200):
        n_lanes = 2 + seed % 3
        ops = random_script(5000 + seed, 300, (cap,))
        res = lanes(ops, lanes=n_lanes)
        assert all(r["rc"] == 0 for r in res)
        checked += check_order(ops, res, n_lanes)
    assert checked > 200 * 250
