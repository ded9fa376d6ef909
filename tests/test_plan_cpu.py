"""The launch planner (effort_amd/csrc/plan.hip: plan_group) through effort_debug_plan, on a machine without a GPU: the hook needs no
context and no device.

(a) the slice counts tests/test_gpu_parity.py::test_geometry_rules_of_round_six asserts on hardware, as literals (256 CUs);
(b) tests/golden/plan_table.json: every output of the hook over formats x lanes x CUs x thin / normal effort x group shapes.  The table was
    recorded from the planner as it was MOVED out of api.hip (the host layer, since split: its caller is mul.hip), before any simplification, and is never regenerated from later code: a
    rule edit that moves a case shows here as a diff of that case, and the table changes only together with the rule, by hand or
    by a run of the parent's library.
"""
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "plan_table.json")
CYCLE = (0.25, 0.5, 0.1)            # the efforts test_geometry_rules_of_round_six cycles through
LOAD = 16                           # percentLoad of oracle.cpu.convert_fp16, the GPU test's `converted`


@pytest.fixture(scope="module")
def plan(hip_lib_built):
    from effort_amd import runtime
    return runtime.plan


def uniform(inDim, outDim, n, efforts=(0.25,)):
    return [(inDim, outDim, efforts[i % len(efforts)], LOAD) for i in range(n)]


# ---------------------------------------------------------------- (a) the cases pinned on hardware
@pytest.mark.parametrize("lanes,n,slices", [(1, 16, 5), (4, 16, 8), (1, 2, 16), (1, 12, 6), (1, 32, 8), (1, 3, 13), (1, 6, 6), (1, 8, 5), (1, 9, 8),
                                            (4, 3, 8), (1, 22, 16), (1, 24, 16), (1, 20, 8), (1, 26, 8), (4, 22, 8)])
def test_q4_groups_of_4096x11008(plan, lanes, n, slices):
    assert plan(uniform(4096, 11008, n), q4=True, lanes=lanes)["slices"][n - 1] == slices


def test_fp16_lone_4096x14336(plan):
    assert plan(uniform(4096, 14336, 1))["slices"] == [32]


@pytest.mark.parametrize("lanes,n,thin", [(1, 11, 2), (1, 12, 2), (1, 23, 2), (1, 13, 3), (1, 10, 0), (1, 14, 0), (1, 16, 0), (1, 24, 0), (4, 12, 0)])
def test_fp16_thin_last_calls_of_4096x11008(plan, lanes, n, thin):
    assert plan(uniform(4096, 11008, n, CYCLE), lanes=lanes)["slices"] == [8] * (n - thin) + [16] * thin


@pytest.mark.parametrize("n,slices", [(8, 16), (9, 12), (11, 8), (16, 8)])
def test_fp16_groups_of_4096x4096(plan, n, slices):
    assert plan(uniform(4096, 4096, n, CYCLE))["slices"] == [slices] * n


@pytest.mark.parametrize("lanes,n,slices,E", [(1, 3, 13, 2), (1, 4, 10, 2), (1, 5, 8, 2), (1, 6, 13, 4), (1, 7, 10, 4), (4, 3, 8, None)])
def test_fp16_small_groups_of_4096x11008(plan, lanes, n, slices, E):
    p = plan(uniform(4096, 11008, n, CYCLE), lanes=lanes)
    assert p["slices"] == [slices] * n
    if E is not None:
        assert p["E"] == E


# ---------------------------------------------------------------- (b) the golden table
UNIFORM = [(4096, 11008), (4096, 14336), (14336, 4096), (11008, 4096), (4096, 4096), (4096, 1024)]
QKV = [(4096, 4096), (4096, 1024), (4096, 1024)]
FIVE = [(4096, 11008), (4096, 14336), (4096, 4096), (4096, 1024), (4096, 2048)]
FUSED_N = (1, 2, 3, 8, 12, 16, 24, 32)


def sweeps(q4):
    """(name, [group, ...]) -- a group is a list of (inDim, outDim, prologue, hasResid)."""
    out = [(f"{i}x{o}", [[(i, o, 0, 0)] * n for n in range(1, 33)]) for i, o in UNIFORM]
    out.append(("wq|wk|wv x 1..10", [[(i, o, 0, 0) for i, o in QKV] * k for k in range(1, 11)]))
    out.append(("w1|w3", [[(4096, 14336, 0, 0)] * 2, [(4096, 11008, 0, 0)] * 2]))
    if not q4:
        out.append(("shard 4096x1376", [[(4096, 1376, 0, 0)] * n for n in (1, 2, 3, 4, 8)]))
    out.append(("five shapes", [[(i, o, 0, 0) for i, o in FIVE], [(i, o, 0, 0) for i, o in FIVE] * 2]))
    for name, pre, res in (("rmsnorm", 2, 0), ("silu", 1, 0), ("resid", 0, 1)):
        out.append((f"{name} 4096x11008", [[(4096, 11008, pre, res)] * n for n in FUSED_N]))
    out.append(("rmsnorm wq|wk|wv, resid on the first", [[(i, o, 2, int(k == 0)) for k, (i, o) in enumerate(QKV)]]))
    return out


def blocks():
    for q4 in (False, True):
        for lanes in (1, 4):
            for numCU in (256, 64):
                for effort in (0.25, 0.02):
                    for name, groups in sweeps(q4):
                        yield f"{'q4' if q4 else 'fp16'} lanes={lanes} cu={numCU} effort={effort} {name}", dict(q4=q4, lanes=lanes, numCU=numCU), effort, groups


def row(plan, kw, effort, group):
    """One compact row: [W, E, [[calls, slices, tiles, sliceRows, launch], ...] run-length over the calls, [[persistent, cutJobs, compact,
    stagger], ...] per launch], or the error code."""
    from effort_amd import EffortError
    try:
        p = plan([(i, o, effort, LOAD, pre, res) for i, o, pre, res in group], **kw)
    except EffortError as e:
        return e.code
    runs = []
    for c in zip(p["slices"], p["tiles"], p["sliceRows"], p["launch"]):
        if runs and tuple(runs[-1][1:]) == c:
            runs[-1][0] += 1
        else:
            runs.append([1, *c])
    return [p["W"], p["E"], runs, [list(l) for l in zip(p["persistent"], p["cutJobs"], p["compact"], p["stagger"])]]


# what overflows: a slice count (tuning override) at which no slab layout fits the lane's scratch; a group past the scratch's slice slots
OVERFLOWS = {
    "no geometry at tuneS": (dict(slices=4096), [(4096, 16384, 0, 0)]),
    "past the scratch caps": (dict(slices=200), [(4096, 4096, 0, 0)] * 32),
}


def test_golden_table(plan):
    table = json.load(open(TABLE))
    want = table["blocks"]
    seen = 0
    for key, kw, effort, groups in blocks():
        assert key in want, key
        got = [row(plan, kw, effort, g) for g in groups]
        assert len(got) == len(want[key]), key
        for g, a, b in zip(groups, got, want[key]):
            assert a == b, (key, len(g), a, b)
        seen += 1
    assert seen == len(want)
    for q4 in (False, True):
        for name, (kw, group) in OVERFLOWS.items():
            key = f"{'q4' if q4 else 'fp16'} {name}"
            code = row(plan, dict(q4=q4, **kw), 0.25, group)
            assert isinstance(code, int) and code < 0 and code == table["errors"][key], (key, code)
