"""The multiply kernel's instantiations and the launches that pin them (tests/variant_scenarios.py), on a machine without a GPU: the
variant hook (effort_debug_variants) and the planner hook (effort_debug_plan) need no context and no device.

(a) ``runtime.variants`` against the list written here: an instantiation added or dropped shows as a diff of one row.
(b) the census: the (variant, mode) pairs the scenario table is predicted to run are exactly the rows of the hook, each in every mode
    it serves (variant_scenarios.modes_served).  A scenario the planner refuses fails the test.
(c) every cached-cutoff scenario is ONE call with more items than its launch has workgroups, at 256 CUs and at 64 and 304: some
    workgroup must work two items of that call.
"""
import pytest

from tests import variant_scenarios as vs

# (W, E, fused, compact, lean) in the order the library walks them: EFFORT_GEOMS, and per geometry each_variant
FP16 = [
    (16, 1, 0, 0, 0), (16, 1, 1, 0, 0), (16, 1, 0, 1, 0),
    (16, 2, 0, 0, 0), (16, 2, 1, 0, 0), (16, 2, 0, 1, 0),
    (16, 4, 0, 0, 0), (16, 4, 1, 0, 0), (16, 4, 0, 1, 0),
    (8, 1, 0, 0, 0), (8, 1, 1, 0, 0), (8, 1, 0, 1, 0), (8, 1, 0, 0, 1), (8, 1, 1, 0, 1), (8, 1, 0, 1, 1), (8, 1, 1, 1, 1),
    (8, 2, 0, 0, 0), (8, 2, 1, 0, 0), (8, 2, 0, 1, 0), (8, 2, 0, 0, 1), (8, 2, 1, 0, 1), (8, 2, 0, 1, 1), (8, 2, 1, 1, 1),
    (8, 4, 0, 0, 0), (8, 4, 1, 0, 0), (8, 4, 0, 1, 0), (8, 4, 0, 0, 1), (8, 4, 1, 0, 1), (8, 4, 0, 1, 1), (8, 4, 1, 1, 1),
    (4, 1, 0, 0, 0), (4, 1, 1, 0, 0), (4, 1, 0, 1, 0),
    (4, 2, 0, 0, 0), (4, 2, 1, 0, 0), (4, 2, 0, 1, 0),
    (4, 4, 0, 0, 0), (4, 4, 1, 0, 0), (4, 4, 0, 1, 0),
    (2, 4, 0, 0, 0), (2, 4, 1, 0, 0), (2, 4, 0, 1, 0),
]
Q4 = [
    (16, 1, 0, 0, 0), (16, 1, 1, 0, 0),
    (16, 2, 0, 0, 0), (16, 2, 1, 0, 0),
    (16, 4, 0, 0, 0), (16, 4, 1, 0, 0),
    (8, 1, 0, 0, 0), (8, 1, 1, 0, 0), (8, 1, 0, 0, 1), (8, 1, 1, 0, 1),
    (8, 2, 0, 0, 0), (8, 2, 1, 0, 0), (8, 2, 0, 0, 1), (8, 2, 1, 0, 1),
    (8, 4, 0, 0, 0), (8, 4, 1, 0, 0), (8, 4, 0, 0, 1), (8, 4, 1, 0, 1),
    (4, 1, 0, 0, 0), (4, 1, 1, 0, 0),
    (4, 2, 0, 0, 0), (4, 2, 1, 0, 0),
    (4, 4, 0, 0, 0), (4, 4, 1, 0, 0),
    (2, 4, 0, 0, 0), (2, 4, 1, 0, 0),
]


@pytest.fixture(scope="module")
def runtime(hip_lib_built):
    from effort_amd import runtime
    return runtime


def planned(runtime, s, numCU):
    """The scenario's plan; the planner refusing it is a failure of the table, never a skip."""
    from effort_amd import EffortError
    rows, kw = vs.plan_args(s, numCU)
    try:
        return runtime.plan(rows, **kw)
    except EffortError as e:
        pytest.fail(f"the planner refuses scenario {s['name']!r} at {numCU} CUs: {e}")


@pytest.mark.parametrize("q4,want", [(False, FP16), (True, Q4)], ids=["fp16", "q4"])
def test_the_instantiations_that_exist(runtime, q4, want):
    got = [(W, E, int(fu), int(co), int(le)) for W, E, fu, co, le in runtime.variants(q4)]
    assert got == want
    assert len(got) == (26 if q4 else 42) and len(set(got)) == len(got)
    assert sorted({(W, E) for W, E, *_ in got}) == sorted(vs.GEOMS)


def test_variant_hook_argument_checks(runtime):
    import ctypes as C
    from effort_amd import _lib
    lib = _lib.lib()
    assert lib.effort_debug_variants(0, None, 0) == 42 and lib.effort_debug_variants(1, None, 0) == 26      # the count alone
    assert lib.effort_debug_variants(0, None, 4) == -1 and lib.effort_debug_variants(0, None, -1) == -1
    buf = (C.c_int * 15)(*([-7] * 15))
    assert lib.effort_debug_variants(0, buf, 2) == 42                   # a short buffer: filled as far as it goes, the count still whole
    assert list(buf) == [16, 1, 0, 0, 0, 16, 1, 1, 0, 0] + [-7] * 5
    assert lib.effort_debug_last_variant(None, 0, buf) == -1


def test_census_covers_every_variant_in_every_mode(runtime):
    full = {(q4, v, mode) for q4 in (False, True) for v in runtime.variants(q4) for mode in vs.modes_served(v)}
    assert len(full) == 56 + 40       # FP16: 7 geometries x 5 + 3 x 7; Q4: 7 x 4 + 3 x 4
    seen = {}
    for s in vs.table(256):
        for launch in vs.predict(s, planned(runtime, s, 256), 256):
            seen.setdefault((s["q4"], launch["variant"], launch["mode"]), []).append(s["name"])
    assert set(seen) - full == set(), sorted(set(seen) - full)          # nothing is predicted that does not exist
    assert full - set(seen) == set(), sorted(full - set(seen))          # nothing that exists is left out
    census = {}
    for s in vs.census(256):
        p = vs.predict(s, planned(runtime, s, 256), 256)
        assert len(p) == 1, s["name"]
        census.setdefault((s["q4"], p[0]["variant"], p[0]["mode"]), []).append(s["name"])
    assert set(census) == full                                           # the census alone covers it, one scenario per pair
    assert all(len(names) == 1 for names in census.values()), [n for n in census.values() if len(n) > 1]


@pytest.mark.parametrize("numCU", [256, 64, 304])
def test_cached_cutoff_scenarios_give_a_workgroup_two_items_of_one_call(runtime, numCU):
    table = vs.cached_cutoff(numCU)
    assert len(table) == 4 * (10 + 3 * 4) * 2
    for s in table:
        p = planned(runtime, s, numCU)
        R = s["persistent"]
        assert len(s["calls"]) == 1 and p["persistent"] == [R] and p["cutJobs"] == [0] and p["compact"] == [0], (s["name"], p)
        assert vs.real_items(s, p) > numCU * R, (s["name"], p)          # pigeonhole: more items of the call than workgroups
        (launch,) = vs.predict(s, p, numCU)
        assert launch["variant"] == (s["tuning"][0], s["tuning"][1], True, False, False) and launch["grid"] == numCU * R, s["name"]


def test_the_items_the_issue_counted(runtime):
    """One call of 4096 -> 1024 at 512 slices is 512 items (a persistent launch at R = 1 on 256 CUs); two such calls are 1024 (R = 2)."""
    one = runtime.plan([(4096, 1024, 0.25, 16, 2, 0)], persistent=1, waves=8, elems=1, slices=512)
    assert one["slices"] == [512] and one["tiles"] == [1] and one["persistent"] == [1]
    two = runtime.plan([(4096, 1024, 0.25, 16, 2, 0)] * 2, persistent=2, waves=8, elems=1, slices=512)
    assert two["slices"] == [512, 512] and two["persistent"] == [2]
    eight = runtime.plan([(4096, 256, 0.25, 16, 2, 0)] * 8, persistent=1, waves=8, elems=1, slices=64)
    assert (eight["persistent"], eight["cutJobs"], eight["compact"]) == ([1], [0], [0])


def test_two_wave_workgroups_raise_small_slice_counts(runtime):
    """FP16 at (2, 4): 128 threads stage at most 128 rows of a slice, so slice counts under 32 of a 4096-row input are raised to 32, not
    refused -- the counts test_launch_geometries_agree_and_are_deterministic runs at that geometry."""
    got = [runtime.plan([(4096, 1024, 0.3)], waves=2, elems=4, slices=S)["slices"] for S in (0, 8, 12, 20, 64, 512)]
    assert got == [[32], [32], [32], [32], [64], [512]]


@pytest.mark.parametrize("q4", [False, True], ids=["fp16", "q4"])
def test_mixed_group_plans(runtime, q4):
    """Four shapes share one persistent launch without cutoff jobs (prologues); with residuals alone the jobs stay on; a fifth shape
    opens a second launch."""
    s = vs.mixed(q4)
    p = planned(runtime, s, 256)
    assert set(p["launch"]) == {0} and p["persistent"] == [1] and p["cutJobs"] == [0] and p["compact"] == [0]
    assert len({(c["inDim"], c["outDim"], c["load"]) for c in s["calls"]}) == 4                     # kMaxGeoms
    r = planned(runtime, vs.mixed(q4, resid_only=True), 256)
    assert r["persistent"] == [1] and r["cutJobs"] == [16] and r["compact"] == [0]
    f = planned(runtime, vs.mixed(q4, fifth=True), 256)
    assert f["launch"] == [0] * len(s["calls"]) + [1] and len(f["persistent"]) == 2
