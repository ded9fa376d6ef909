"""The case table of tests/cutoff_cases.py on the CPU: the model of block_find_cutoff (tests/cutoff_model.py) against the oracle's
findCutoff32 at every table size and with and without the fixed window -- and WHICH BRANCHES the table reaches.

The shipped kernels carry no stamps, so the GPU test (tests/test_gpu_cutoff_paths.py) cannot read the path a call took; what it can
rely on is this file: the model restates the device's control flow, agrees with the oracle bit for bit, and its path records over the
table contain every label of the list written out below, at each of the four table sizes.  The list is a condition on the TABLE: a
refactor of the cases (or of the selection code and, with it, of the model) that stops reaching a branch fails here."""
import numpy as np
import pytest

from tests import cutoff_cases as cc
from tests.cutoff_model import CAPS, EXITS, GUARDS, model_cutoff

_RUN = {}


def run(oracle):
    """{(case name, effort, cap, window): (path record | None, what went wrong | None)}, computed once."""
    if not _RUN:
        for case in cc.table():
            for effort in cc.efforts(case):
                q = cc.effort_to_q(effort)
                assert q == oracle.effort_to_q(effort), (effort, q)
                want, _ = oracle.find_cutoff(case.v, case.probes, 0, effort)
                for cap in CAPS:
                    for window in (False, True):
                        try:
                            got, path = model_cutoff(case.v, case.probes, q, cap=cap, window=window)
                            same = np.float32(want).tobytes() == np.float32(got).tobytes()
                            _RUN[(case.name, effort, cap, window)] = (path, None if same else f"cutoff {got!r}, the oracle's {want!r}")
                        except AssertionError as e:                            # one of the model's own assertions: a shortcut against its count
                            _RUN[(case.name, effort, cap, window)] = (None, f"model assertion: {e!r}")
    return _RUN


def test_boundary_efforts_hit_their_quantiles(oracle_cpu):
    assert [oracle_cpu.effort_to_q(e) for e in cc.BOUNDARY_EFFORTS] == list(cc.BOUNDARY_QS) == [1, 2, 4093, 4094]
    assert [cc.effort_to_q(e) for e in cc.EFFORTS] == [oracle_cpu.effort_to_q(e) for e in cc.EFFORTS]


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_model_matches_oracle_on_every_case(oracle_cpu, family):
    """Every case and effort, cap in (1024, 2048, 4096, 8192), window in (False, True): the model's cutoff bits are the oracle's and the
    model's internal assertions hold (each shortcut against the count it stands for)."""
    names = {c.name for c in cc.table() if c.family == family}
    assert names
    bad = {k: why for k, (_, why) in run(oracle_cpu).items() if k[0] in names and why}
    assert not bad, bad


def test_every_case_family_is_there():
    t = cc.table()
    assert {c.family for c in t} == set(cc.FAMILIES)
    assert all(np.isfinite(c.v).all() for c in t)
    names = {c.name for c in t}
    assert {"all-zero", "one-nonzero", "all-equal", "probes-zero", "above-1000", "subnormal", "near-max", "two-level", "late-tail", "wide-0", "wide-1"} <= names
    for cap in CAPS:
        assert {f"span-{cap}-{d}{z}" for d in ("under", "full", "over") for z in ("", "-zeros")} <= names
        assert {f"window-{cap}-{w}" for w in ("min-on-base", "min-below-base", "max-on-last", "max-beyond-last")} <= names
    assert {f"{k}-{s}" for k in ("gauss", "heavy", "zeros", "few", "tiny", "ties") for s in (0, 1)} <= names


@pytest.mark.parametrize("cap", CAPS)
def test_constructed_cases_take_the_branch_they_aim_at(oracle_cpu, cap):
    """The boundaries themselves, per table size: a span of cap - 2 and cap - 1 cells runs no ballot pass and cap cells runs one or more;
    the window is used with the smallest nonzero value on its first cell and the largest on its last, and the table is rebuilt one
    cell either side; the two-level vector leaves the loop inside its first ballot pass, at every table size."""
    R = run(oracle_cpu)
    paths = lambda name, window: [R[(name, e, cap, window)][0] for e in cc.EFFORTS + cc.BOUNDARY_EFFORTS]      # noqa: E731
    for z in ("", "-zeros"):
        for window in (False, True):
            assert all(p["passes"] == 0 for p in paths(f"span-{cap}-under{z}", window))
            assert all(p["passes"] == 0 for p in paths(f"span-{cap}-full{z}", window))
            assert all(p["passes"] >= 1 for p in paths(f"span-{cap}-over{z}", window))
    for name, label in (("min-on-base", "window"), ("min-below-base", "rebuilt-low"), ("max-on-last", "window"), ("max-beyond-last", "rebuilt-high")):
        got = {p["table"] for p in paths(f"window-{cap}-{name}", True)}
        assert got == {label}, (name, got)
        assert {p["table"] for p in paths(f"window-{cap}-{name}", False)} == {"range"}
    two = next(c for c in cc.table() if c.name == "two-level")
    p = R[("two-level", two.extra[0], cap, True)][0]
    assert (p["passes"], p["after_passes"], p["exit"], p["rounds"]) == (1, "exit", "count-equal", 1), p
    if cap == 8192:
        assert max(p["passes"] for name in ("wide-0", "wide-1") for p in paths(name, True)) >= 5


@pytest.mark.parametrize("cap", CAPS)
def test_the_table_reaches_every_branch(oracle_cpu, cap):
    """The union of the path records over the table, per table size, holds every label below.  The list is written out, not derived
    from what the table happens to reach.

    ONE label is unreachable, and the test asserts that no case reaches it (so a change that makes it reachable is noticed):

      after_passes = "adjacent" (cutoff_device.h: "adjacent cells already (possible only after ballot passes)").  A ballot pass runs
      only while the cells between the bounds outnumber the table: pHi - max(pLo, pminNZ) + 1 > cap >= 1024, i.e. more than eight
      octaves between the float bounds, so lo <= hi / 256 (a bound never set stands for the smallest / largest value, and a lower
      bound below pminNZ is farther still).  The pass's midpoint (lo + hi) / 2 then lies in [hi / 2, hi / 2 * (1 + 2^-8)]: 127 or 128
      cells under hi's, and at least cap - 128 cells above lo's.  Whichever bound it replaces, the other is more than one cell away.
      The bounds can only become adjacent in the table phase, where the code takes the tail after the table.

    The other label the search's comments call rare, a tail entered after more than 60 rounds (bisect_to_cell_edge's closed form then
    gives way to the loop although X >= 128), IS reached: the `late-tail` case walks its upper bound down 64 octaves before the
    bracket closes on a tie, and the list requires it."""
    recs = [(k, p) for k, (p, _) in run(oracle_cpu).items() if k[2] == cap and p is not None]
    assert len(recs) == sum(len(cc.efforts(c)) for c in cc.table()) * 2
    win = [p for k, p in recs if k[3]]
    rng = [p for k, p in recs if not k[3]]
    for group in (win, rng):                                      # (each instantiation kind on its own)
        passes = {p["passes"] for p in group}
        assert 0 in passes and any(n >= 1 for n in passes) and any(n >= 5 for n in passes), sorted(passes)
        assert {p["after_passes"] for p in group} == {"exit", "table"}                    # "adjacent": unreachable, see above
        assert any(p["after_passes"] == "table" and p["lo_set"] and p["hi_set"] and p["above"] > 0 for p in group)
        assert {p["exit"] for p in group} == set(EXITS) == {"count-equal", "bounds-1e-5", "counts-within-3", "hundred-rounds", "fixed-point",
                                                            "tail-closed-form", "tail-loop"}
        assert any(p["exit"] in EXITS[:5] for p in group if p["after_passes"] == "exit")    # an exit of the reference inside a ballot round
        assert any(p["tail_late"] and p["exit"] == "tail-loop" for p in group)
        assert any(p["table_rounds"] > 16 and p["table_blocks"] > 1 for p in group)
        assert {g for p in group for gs in p["guards"] for g in gs} == set(GUARDS) == {"k<=0", "k>4096", "allGE<k", "sgAll>=64"}
    assert {p["table"] for p in win} == {None, "window", "rebuilt-low", "rebuilt-high", "rebuilt-after-passes"}
    assert {p["table"] for p in rng} == {None, "range"}
    assert all((p["table"] is None) == (p["after_passes"] != "table") for p in win + rng)
