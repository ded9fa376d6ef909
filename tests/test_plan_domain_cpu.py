"""The launch planner (csrc/plan.hip through effort_debug_plan: no context, no device) over the whole domain registration accepts --
inDim 4096 .. 65535, odd ones included, outDim 32 .. 16384, percentLoad 1 .. 16 -- where tests/test_plan_cpu.py pins the rules on the
decode loop's shapes.  The grid is tests/edge_shapes.py's (the shapes of tests/test_gpu_edge_shapes.py are on it): uniform groups of
1 .. 32 calls, both formats, 64 / 256 / 304 CUs, with and without lanes, and the workgroup sizes the tuning override reaches.

Every plan that is returned must be a geometry the kernel can run:
  * the slices cover the inputs, none is empty:      sliceRows * slices >= inDim > sliceRows * (slices - 1)
  * the tiles cover the columns, none is empty:      tiles * 64 * E >= cols > (tiles - 1) * 64 * E
  * a launch on the compact row means (one LDS-direct dword = two u16 means: stage_issue) has only even inDim and even sliceRows
  * every call belongs to exactly one launch, the launches in call order
Where the planner refuses, the code is EFFORT_ERR_SHAPE and the group is one that cannot fit the context's scratch (``must_overflow``).
"""
import os

import pytest

from tests import edge_shapes as es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_TILES, MAX_SLICES, SLAB_BYTES = 1024, 4096, 64 << 20          # a lane's scratch (csrc/host.h: effort_ctx)


@pytest.fixture(scope="module")
def plan(hip_lib_built):
    from effort_amd import runtime
    return runtime.plan


def check_plan(p, calls, q4):
    E = p["E"]
    assert (p["W"], E) in {(16, 1), (16, 2), (16, 4), (8, 1), (8, 2), (8, 4), (4, 1), (4, 2), (4, 4), (2, 4)}, (p["W"], E)
    k = len(p["persistent"])
    assert p["launch"] == sorted(p["launch"]) and set(p["launch"]) == set(range(k)), p["launch"]       # one launch each, none empty
    for i, c in enumerate(calls):
        inDim, outDim = c[0], c[1]
        cols = outDim // (32 if q4 else 16)
        S, T, B = p["slices"][i], p["tiles"][i], p["sliceRows"][i]
        assert S >= 1 and B >= 1 and B * S >= inDim > B * (S - 1), (c, S, B)
        assert T * 64 * E >= cols > (T - 1) * 64 * E, (c, T, E)
        if p["compact"][p["launch"][i]]:
            assert not q4 and inDim % 2 == 0 and B % 2 == 0, (c, B)


def must_overflow(calls, q4, W, E):
    """The group cannot fit a lane's scratch even at the FEWEST slices any rule gives a call: a lower bound of its needs, worked out here from
    the shapes alone.  Per call: ceil(cols / (64 * E)) tiles, each with an arrival ticket (+ 1 word behind the last call's); at least
    ceil(inDim / B) slices, B the tallest slice there is -- 512 input rows (plan.hip: min_slices), 832 for Q4 at E = 1 (its one-round rules),
    and never more than a workgroup of W waves stages (a thread lands one input of the slice, Q4 two: 64 * W / 128 * W); slices x tiles partial
    tiles of 16 (Q4: 32) x E x 64 floats.  Over the ticket words, the per-slice counters or the slab bytes: the refusal is the scratch's."""
    per = 32 if q4 else 16
    B = min(832 if E == 1 else 512, 128 * W) if q4 else min(512, 64 * W)
    tiles = [-(-(c[1] // per) // (64 * E)) for c in calls]
    slices = [-(-c[0] // B) for c in calls]
    slab = sum(s * t for s, t in zip(slices, tiles)) * per * E * 64 * 4
    return sum(tiles) + 1 > MAX_TILES or sum(slices) > MAX_SLICES or slab > SLAB_BYTES


def grid():
    for q4 in (False, True):
        for inDim in es.PLAN_IN_DIMS:
            for outDim in es.PLAN_OUT_DIMS:
                for load in ((8,) if q4 else es.PLAN_LOADS):
                    yield q4, inDim, outDim, load


def test_every_returned_plan_is_a_runnable_geometry(plan):
    from effort_amd import EffortError
    plans = 0
    refused = []
    for q4, inDim, outDim, load in grid():
        for n in es.PLAN_GROUPS:
            calls = [(inDim, outDim, (0.25, 1.0, 0.02)[i % 3], load) for i in range(n)]
            for numCU, lanes in es.PLAN_ENVS:
                for waves, elems in es.PLAN_TUNES:
                    try:
                        p = plan(calls, q4=q4, numCU=numCU, lanes=lanes, waves=waves, elems=elems)
                    except EffortError as e:
                        assert e.code == -2, (q4, calls[0], n, numCU, lanes, waves, e)
                        refused.append((q4, inDim, outDim, load, n, numCU, lanes, waves, elems))
                        continue
                    check_plan(p, calls, q4)
                    plans += 1
    assert plans > 10000
    # the refusals: every one a group that cannot fit a lane's scratch (64 MiB of partial tiles, 4096 per-slice counters, 1024 tickets) at the
    # columns per lane the override names -- or, the heuristic choosing them, at one of the three there are.  Which ones (4853 of the grid's
    # 63000): no lone call and no pair; groups of three only on 2-wave workgroups (slices of 128 rows at most) at 65534 / 65535 inputs and 11008
    # outputs or more; up to 4500 inputs only 32 calls of 16352 / 16384 outputs on 2-wave workgroups.  The rest are groups of 8 calls or more at
    # 8191 inputs or more.
    for q4, inDim, outDim, load, n, numCU, lanes, waves, elems in refused:
        calls = [(inDim, outDim)] * n
        assert any(must_overflow(calls, q4, waves or 8, e) for e in ((elems,) if elems else (1, 2, 4))), (q4, inDim, outDim, load, n, numCU, lanes, waves, elems)
        assert n >= 3 and inDim >= 4097
    assert not [r for r in refused if r[4] == 3 and not (r[7] == 2 and r[1] >= 65534 and r[2] >= 11008)]
    assert not [r for r in refused if r[1] <= 4500 and not (r[4] == 32 and r[7] == 2 and r[2] >= 16352)]
    assert not [r for r in refused if r[1] > 4500 and r[4] > 3 and not (r[4] >= 8 and r[1] >= 8191)]
    print(f"{plans} plans checked, {len(refused)} groups refused (EFFORT_ERR_SHAPE, past the scratch)")


def test_mixed_parity_groups_leave_the_compact_means(plan):
    """A launch is compact only if EVERY call of it can be: an odd inDim beside an even one takes the whole launch to the 8-byte stats."""
    for n in (2, 3, 8, 17):
        for odd, even in ((4097, 4096), (65535, 65534)):
            calls = [((odd, even)[i & 1], 64, 0.25, 16) for i in range(n)]
            for persistent in (-1, 1):
                p = plan(calls, persistent=persistent)
                check_plan(p, calls, False)
                assert not any(p["compact"]), (n, odd, persistent, p["compact"])
            same = plan([(even, 64, 0.25, 16)] * n)
            check_plan(same, [(even, 64, 0.25, 16)] * n, False)


def test_edge_shapes_is_numpy_only_and_inside_the_domain(hip_lib_built):
    """tests/edge_shapes.py imports without torch (and without the package), builds a bundle, and asks for no shape registration refuses."""
    import subprocess
    import sys

    import effort_amd
    code = ("import sys; from tests import edge_shapes as es; lay = es.bundle(es.FP16_CASES[1]); q = es.bundle(es.Q4_CASES[0]); "
            "assert lay['buckets'].shape == (16 * 4099, 6) and q['buckets'].shape == (8 * 4097, 1) and len(q['outliers']) == 600; "
            "assert 'torch' not in sys.modules and 'effort_amd' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    lib = effort_amd.lib()
    for c in es.FP16_CASES:
        assert lib.effort_debug_check_bundle(0, c.inDim, c.outDim, c.percentLoad, 1, 0) == 0, c
    for c in es.Q4_CASES:
        assert lib.effort_debug_check_bundle(1, c.inDim, c.outDim, 8, 1, 0) == 0, c
    s = es.STACK
    assert lib.effort_debug_check_bundle(0, s["inDim"], s["outDim"], s["percentLoad"], s["experts"], 0) == 0
    assert lib.effort_debug_check_bundle(0, s["inDim"], s["outDim"], s["percentLoad"], s["experts"] + 1, 0) == -2


def test_the_gpu_test_shapes_plan_as_lone_calls_and_groups_of_three(plan):
    for case in es.FP16_CASES:
        for n in (1, 3):
            calls = [(case.inDim, case.outDim, es.GROUP_EFFORTS[i % 3], case.percentLoad) for i in range(n)]
            p = plan(calls)
            check_plan(p, calls, False)
            assert (case.inDim % 2 == 1) <= (not any(p["compact"])), case
    for case in es.Q4_CASES:
        for n in (1, 3):
            calls = [(case.inDim, case.outDim, es.GROUP_EFFORTS[i % 3], 8) for i in range(n)]
            check_plan(plan(calls, q4=True), calls, True)
