"""block_find_cutoff (effort_amd/csrc/cutoff_device.h) branch by branch, at every workgroup size that instantiates it.

The table of tests/cutoff_cases.py -- degenerate vectors, spans of exactly cap - 2 / cap - 1 / cap cells for each table size, the edges of
the fixed window, ~100 octaves of range, the kinds that leave the loop through each exit -- goes through every route that runs the search:

  route                                                       instantiation
  BucketMul.calcDispatch                                      standalone kernel: 1024 threads (8192 cells), no window; the dispatch list too
  a group of three under set_split_cutoff(True)               find_cutoff_group_kernel: 1024 threads, no window
  lone bucketMul at set_tuning(W, E, 32), a plain grid        W = 16, 8, 4, 2: 8192, 4096, 2048, 1024 cells, the WINDOW variant (W = 8: the lean kernel)
  the same W, the launch made persistent                      cutoff_job<64 W> of the persistent instantiation: no window; the call's items read what it published
  one persistent group of 8 calls, each a different case      eight cutoff jobs in one launch, every call's items reading its own

FP16 on all routes; Q4 (separate instantiations of the same template) on the lone plain and persistent routes with the degenerate, span and
window families.  The shipped kernels carry no stamps, so which branch a call took cannot be read here: tests/test_cutoff_cases_cpu.py shows,
with the model of tests/cutoff_model.py, that the table reaches every branch at each of the four table sizes, and that the model's bits are
the oracle's.  Here every call's cutoff BITS and dispatch count are the oracle's; the launch is the one the route intends
(Gpu.last_variant, runtime.plan: a silent fallback to another geometry fails); the output, NaN before the call, holds no NaN and is
exactly zero where no row was dispatched; and for inputs inside the scales tests/test_gpu_parity.py::test_cutoff_across_input_scales covers it
passes the project's bar (close(): 2e-5 of max|want|, cosine >= 0.999999) against float64 over exactly the oracle's rows
(tests/edge_shapes.py::reference).  Subnormal and near-maximal inputs check selection only.

The handles are the smallest bundles registration takes (4096 x 64 FP16, 4096 x 32 Q4: the weights do not matter to the cutoff) with the
case's probes in place of the bundle's.  Every loop of the search is bounded by the reference's 100 rounds for finite inputs; all inputs are finite."""
import numpy as np
import pytest
import torch

from tests import cutoff_cases as cc
from tests import edge_shapes as es
from tests.test_gpu_parity import DEV, close, dev16, devf

pytestmark = pytest.mark.gpu

GEOMS = ((16, 1), (8, 1), (4, 1), (2, 4))                   # (W, E): 8 x 64 W cells
PLAIN_SLICES = 32
GROUP_TUNING = (8, 1, 64)                                   # the group of 8: 8 x 64 items
Q4_FAMILIES = ("degenerate", "span", "window")


@pytest.fixture(scope="module")
def ea(hip_lib_built):
    import effort_amd
    assert torch.cuda.is_available()
    effort_amd.gpu(0)
    return effort_amd


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


_BASE, _STATE, _REFS = {}, {}, {}


def base(q4):
    """The bundle's host layout and its buckets / stats on the device, shared by every case's handle."""
    if q4 not in _BASE:
        lay = es.q4_bundle(4096, 32) if q4 else es.fp16_bundle(4096, 64)
        _BASE[q4] = (lay, dev16(lay["buckets"]), (devf if q4 else dev16)(lay["stats"]))
    return _BASE[q4]


def state(ea, q4, case):
    """The case on the device: a handle with the case's probes, its input, and the layout its reference is computed from."""
    key = (q4, case.name)
    if key not in _STATE:
        lay, b, s = base(q4)
        kw = {"q4": True} if q4 else {"percentLoad": lay["percentLoad"]}
        ew = ea.ExpertWeights(b, s, dev16(case.probes.copy()), inSize=lay["inDim"], outSize=lay["outDim"], **kw)
        _STATE[key] = {"case": case, "q4": q4, "ew": ew, "vd": devf(case.v.copy()), "lay": dict(lay, probes=case.probes.view(np.float16))}
    return _STATE[key]


def ref(oracle, st, effort):
    """edge_shapes.reference of one call (the oracle's cutoff and rows, float64 over those rows), computed once."""
    key = (st["q4"], st["case"].name, effort)
    if key not in _REFS:
        with np.errstate(all="ignore"):                       # (the oracle's own f32 product of the near-maximal inputs may overflow: not compared)
            _REFS[key] = es.reference(oracle, st["lay"], st["case"].v, effort)
    return _REFS[key]


def cases(families):
    return [c for c in cc.table() if c.family in families]


def nan_out(n):
    return torch.full((n,), float("nan"), device=DEV)


def check(g, idx, out, R, case, tag, misses):
    """Selection and the written output are asserted on the spot; a product outside the bar is noted in ``misses`` and asserted by the caller
    once the route is through, so that one product does not hide the selection of the cases behind it."""
    cutoff, count = g.last_cutoff(idx), g.last_dispatch_count(idx)
    assert np.float32(cutoff).tobytes() == np.float32(R["cutoff"]).tobytes(), (tag, cutoff, R["cutoff"])
    assert count == R["count"], (tag, count, R["count"])
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), tag                                    # every output was written
    if R["count"] == 0:
        assert not got.any(), tag
    if cc.product_checked(case):
        for name, want in (("float64 over the oracle's rows", R["want"]), ("the oracle's own product", R["full"])):
            if want is not None and not close(got, want):
                err = float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))
                print(f"{tag}: |out - want| / max|want| = {err:.2e} against {name}")
                misses.append((tag, name, err))


def planned(st, n_calls, efforts, **kw):
    from effort_amd import runtime
    lay = st["lay"]
    return runtime.plan([(lay["inDim"], lay["outDim"], e, lay["percentLoad"]) for e in efforts[:n_calls]], q4=st["q4"], numCU=num_cu(), **kw)


def lone(ea, st, effort):
    out = nan_out(st["ew"].outSize)
    (ea.bucketMulQ4 if st["q4"] else ea.bucketMul)(st["vd"], st["ew"], None, out, effort)
    ea.gpu().eval()
    return out


# ------------------------------------------------------------------------------------------------ the standalone kernels
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_standalone_kernel(ea, oracle_cpu, family):
    """effort_calc_dispatch: find_cutoff_kernel (1024 threads, no window), then the dispatch list -- its bytes against prepare_dispatch."""
    g, bm = ea.gpu(), ea.BucketMul.shared()
    for case in cases((family,)):
        st = state(ea, False, case)
        lay = st["lay"]
        for effort in cc.efforts(case):
            cutoff, _ = oracle_cpu.find_cutoff(case.v, case.probes, 0, effort)
            disp, n = oracle_cpu.prepare_dispatch(case.v, lay["stats"], 0, cutoff, lay["inDim"], lay["outDim"] // 16, lay["percentLoad"])
            bm.calcDispatch(st["vd"], st["ew"], None, effort)
            g.eval()
            assert np.float32(bm.cutoff).tobytes() == np.float32(cutoff).tobytes(), (case.name, effort, bm.cutoff, cutoff)
            assert int(bm.dispatch_size.item()) == n == g.last_dispatch_count(), (case.name, effort)
            assert bm.dispatch[:n].cpu().numpy().tobytes() == disp[:n].tobytes(), (case.name, effort)


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_group_of_three_with_the_split_cutoff(ea, oracle_cpu, family):
    """set_split_cutoff(True): find_cutoff_group_kernel evaluates the three cutoffs in a launch of its own, the multiply reads them."""
    g, misses = ea.gpu(), []
    try:
        g.set_split_cutoff(True)
        for case in cases((family,)):
            st = state(ea, False, case)
            eff = list(cc.efforts(case))
            eff += eff[:-len(eff) % 3]                                     # (whole groups of three)
            for i in range(0, len(eff), 3):
                trio = eff[i:i + 3]
                outs = [nan_out(st["ew"].outSize) for _ in trio]
                ea.bucketMulGroup([(st["vd"], st["ew"], None, o, e) for o, e in zip(outs, trio)])
                g.eval()
                lv = g.last_variant()
                assert lv["persistent"] == 0 and lv["variant"][0] == 8 and lv["grid"] == lv["totalItems"], lv
                for k, (o, e) in enumerate(zip(outs, trio)):
                    check(g, k, o, ref(oracle_cpu, st, e), case, (case.name, "split group", e), misses)
    finally:
        g.set_split_cutoff(False)
    assert not misses, misses


# ------------------------------------------------------------------------------------------------ lone calls, every workgroup size
def lone_route(ea, oracle_cpu, q4, W, E, persistent, families):
    g, misses = ea.gpu(), []
    numCU = num_cu()
    S = next(s for s in (512, 1024, 2048) if s > numCU) if persistent else PLAIN_SLICES      # one tile: S items, more than a persistent grid has workgroups
    first = state(ea, q4, cases(families)[0])
    p = planned(first, 1, [0.25], persistent=1 if persistent else -1, waves=W, elems=E, slices=S)
    # what the route intends: W waves; a plain grid where every workgroup cuts for itself, or a persistent launch with the call's cutoff job
    assert (p["W"], p["E"], p["tiles"], p["slices"]) == (W, E, [1], [S]), p
    assert (p["persistent"], p["cutJobs"]) == (([1], [8]) if persistent else ([0], [0])), p
    try:
        g.set_tuning(W, E, S)
        g.set_persistent(1 if persistent else -1)
        for case in cases(families):
            st = state(ea, q4, case)
            for effort in cc.efforts(case):
                out = lone(ea, st, effort)
                lv = g.last_variant()
                assert lv["variant"][:2] == (W, E) and lv["totalItems"] == S, lv
                if persistent:
                    assert lv["persistent"] == 1 and lv["grid"] == numCU < S and not lv["variant"][4], lv
                else:
                    assert lv["persistent"] == 0 and lv["grid"] == S and lv["variant"][4] == (W == 8), lv
                check(g, 0, out, ref(oracle_cpu, st, effort), case, (case.name, "q4" if q4 else "fp16", W, "persistent" if persistent else "plain", effort), misses)
    finally:
        g.set_persistent(-1)
        g.set_tuning(0, 0, 0)
    assert not misses, (len(misses), misses[:8])


@pytest.mark.parametrize("W,E", GEOMS)
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_lone_plain_grid_fp16(ea, oracle_cpu, family, W, E):
    """The window variant at 64 W threads: every workgroup of the grid counts into the fixed window and keeps or rebuilds the table."""
    lone_route(ea, oracle_cpu, False, W, E, False, (family,))


@pytest.mark.parametrize("W,E", GEOMS)
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_lone_persistent_fp16(ea, oracle_cpu, family, W, E):
    """The same geometry with more items than workgroups: the persistent instantiation's cutoff job (no window) publishes the cutoff."""
    lone_route(ea, oracle_cpu, False, W, E, True, (family,))


@pytest.mark.parametrize("W,E", GEOMS)
@pytest.mark.parametrize("persistent", [False, True], ids=["plain", "persistent"])
def test_lone_q4(ea, oracle_cpu, W, E, persistent):
    """The Q4 kernels' own instantiations of the search, plain and persistent, with the degenerate, span and window families.

    (W, E) = (2, 4) on the 4096 x 32 handle -- one 16-bit word per row, lane 0 loading eight bytes of it -- is also where the multiply's row
    stream once lost the LAST word of the buffer: the dword holding it straddles the end of the buffer descriptor's records, the range
    check answers 0 for the whole dword, and the row added its value to outputs 0, 8, 16, 24 instead of its own four.  Measured then, with
    that row kept: 9.4e-4 of max|want| on `probes-zero` (cutoff 0: all 32768 rows), 4.6e-4 on a Gaussian input at effort 1, against 1.8e-6 /
    1.1e-6 at E = 1, and the same figures at (4, 4) and (8, 4).  csrc/bucket_mul.hip now corrects that one word before the stream starts;
    E = 4 gives E = 1's figures."""
    lone_route(ea, oracle_cpu, True, W, E, persistent, Q4_FAMILIES)


# ------------------------------------------------------------------------------------------------ cutoff jobs of several calls
def test_persistent_group_of_eight_cases(ea, oracle_cpu):
    """Eight calls, each a different case, in one persistent launch: eight cutoff jobs at the head of the queues, one workgroup
    publishing each call's cutoff, the calls' items reading their own.  Every (case, effort) of the table takes part once."""
    g, misses = ea.gpu(), []
    numCU = num_cu()
    table = cc.table()
    pairs = [(c, cc.efforts(c)[i]) for i in range(max(len(cc.efforts(c)) for c in table)) for c in table if i < len(cc.efforts(c))]
    pairs += pairs[:-len(pairs) % 8]
    W, E, S = GROUP_TUNING
    assert 8 * S > numCU
    p = planned(state(ea, False, table[0]), 8, [e for _, e in pairs[:8]], persistent=1, waves=W, elems=E, slices=S)
    assert (p["W"], p["E"], p["slices"], p["persistent"], p["cutJobs"]) == (W, E, [S] * 8, [1], [8]), p
    try:
        g.set_tuning(W, E, S)
        g.set_persistent(1)
        for i in range(0, len(pairs), 8):
            group = pairs[i:i + 8]
            assert len({c.name for c, _ in group}) == 8
            sts = [state(ea, False, c) for c, _ in group]
            outs = [nan_out(st["ew"].outSize) for st in sts]
            ea.bucketMulGroup([(st["vd"], st["ew"], None, o, e) for st, o, (_, e) in zip(sts, outs, group)])
            g.eval()
            lv = g.last_variant()
            assert lv["persistent"] == 1 and lv["grid"] == numCU and lv["totalItems"] == 8 * S and lv["variant"][:2] == (W, E), lv
            for k, (st, o, (c, e)) in enumerate(zip(sts, outs, group)):
                check(g, k, o, ref(oracle_cpu, st, e), c, (c.name, "group of eight", k, e), misses)
    finally:
        g.set_persistent(-1)
        g.set_tuning(0, 0, 0)
    assert not misses, misses
