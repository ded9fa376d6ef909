"""The multiply at the borders of the shapes registration accepts (tests/edge_shapes.py has the bundles, the case tables and the reference).

The other GPU tests run on inDim in {4096, 4500, 4608, 11008, 14336, 16448} -- all multiples of 4 -- and FP16 rows of 4 columns or more.
Registration takes any inDim from 4096 to 65535, any outDim that is a multiple of 32 up to 16384, and stacks up to 4 GiB; the kernel has code
that runs only out there: the 8-byte stats path an odd inDim forces (odd row offsets), tiles with 2 or 6 live lanes, Q4 rows of 1 and 3 words,
the widest and the ragged-widest row, the rmsNorm prologue's tail loop at 4097 and 65535 inputs, the largest row numbers, 32-bit offsets next
to 2^32.

Bars, the project's (tests/test_gpu_parity.py): dispatch count and cutoff equal the oracle's exactly; the output passes close() -- within 2e-5
of max|want|, cosine >= 0.999999 -- against float64 over exactly the oracle's rows, and against the oracle's own product where its full
call takes the shape.  Output buffers hold NaN before every call.  Every launch prints its worst error over max|want| (run with -s).

Measured on an MI355X, the worst |out - want| / max|want| of a case over its efforts (the bar is 2e-5; no case needed the fixed-point
envelope of tests/fixedpoint_reference.py; dense and aligned rows give the same bits):

    case (inDim x outDim)              lone / group of three    persistent group    norm prologue + residual
    odd-2col        4097 x 32          1.8e-6                   1.8e-6              8.6e-7
    odd-6col        4099 x 96          2.0e-6
    odd-widest      4097 x 16384       3.1e-6                   2.9e-6              2.9e-6
    ragged-top      4096 x 16352       5.7e-6
    largest-odd     65535 x 64         6.0e-6 / 1.1e-5          6.0e-6              3.9e-6
    largest-even    65534 x 32         8.8e-6
    odd-load3       16385 x 160, 3     8.2e-7
    q4-one-word     4097 x 32          3.3e-7
    q4-three-words  4099 x 96          2.6e-7
    q4-largest-odd  65535 x 64         3.1e-6 / 5.9e-6
    q4-lds-limit    16384 x 4096       6.9e-7 / 2.3e-6                              1.2e-6
    stack of 31 experts, expNo 30      2.9e-6   (expNo 0 and 29: 1.3e-6)

(largest-odd has 65535 addends per output at full effort; its group of three runs 128 slices of 512 rows where the lone call runs 256 of
256: a grid twice as coarse.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import edge_shapes as es
from tests.test_gpu_parity import DEV, close, dev16, devf
from tests.util import make_v, structured_norm_w

pytestmark = pytest.mark.gpu

WORST = {}                     # case -> the worst error / max|want| seen (printed as the tests go)


@pytest.fixture(scope="module")
def ea(hip_lib_built):
    import effort_amd
    assert torch.cuda.is_available()
    effort_amd.gpu(0)
    return effort_amd


def nan_out(n):
    return torch.full((n,), float("nan"), device=DEV)


_DATA, _REFS = {}, {}


def case_data(ea, case):
    """The case's host layout, its input, and two handles on ONE set of device buffers: rows on the dense pitch, and after align_rows()."""
    key = (type(case).__name__, case.name)
    if key not in _DATA:
        lay = es.bundle(case)
        q4 = lay["q4"]
        b, s, p = dev16(lay["buckets"]), (devf if q4 else dev16)(lay["stats"]), dev16(lay["probes"])
        kw = {"outliers": None if lay["outliers"] is None else devf(lay["outliers"]), "q4": True} if q4 else {"percentLoad": lay["percentLoad"]}
        dense = ea.ExpertWeights(b, s, p, inSize=lay["inDim"], outSize=lay["outDim"], **kw)
        aligned = ea.ExpertWeights(b, s, p, inSize=lay["inDim"], outSize=lay["outDim"], **kw)
        cols = lay["buckets"].shape[1]
        assert dense.rowPitch == 2 * cols
        assert aligned.align_rows() == (2 * cols + 127) // 128 * 128
        _DATA[key] = {"key": key, "lay": lay, "dense": dense, "aligned": aligned, "v": make_v(lay["inDim"], heavy=True)}
    return _DATA[key]


def refs(oracle_cpu, d, v, tag="v"):
    """{effort: reference} of the case on input ``v``, computed once."""
    key = d["key"] + (tag,)
    if key not in _REFS:
        _REFS[key] = {e: es.reference(oracle_cpu, d["lay"], v, e) for e in es.EFFORTS}
    return _REFS[key]


def check(g, idx, out, ref, tag, resid=None):
    assert g.last_dispatch_count(idx) == ref["count"], tag
    assert np.float32(g.last_cutoff(idx)).tobytes() == np.float32(ref["cutoff"]).tobytes(), tag
    got = out.cpu().numpy()
    assert not np.isnan(got).any(), tag                                   # every output was written
    want = ref["want"] if resid is None else ref["want"] + resid.astype(np.float64)
    err = float(np.abs(got - want).max() / max(float(np.abs(want).max()), 1e-300))
    WORST[tag[0]] = max(WORST.get(tag[0], 0.0), err)
    print(f"{str(tag):72s} rows {ref['count']:8d}  err / max|want| {err:.2e}")
    assert close(got, want), (tag, err)
    if ref["full"] is not None and resid is None:
        assert close(got, ref["full"]), (tag, "against the oracle's own product")


def lone(ea, ew, vd, effort):
    out = nan_out(ew.outSize)
    (ea.bucketMulQ4 if ew.q4 else ea.bucketMul)(vd, ew, None, out, effort)
    ea.gpu().eval()
    return out


def lone_calls_and_a_group(ea, d, R, ew, form):
    """Every effort as a lone call, then a group of three on the one input; returns the outputs."""
    g, vd, name = ea.gpu(), devf(d["v"]), d["key"][1]
    outs = []
    for effort in es.EFFORTS:
        outs.append(lone(ea, ew, vd, effort))
        check(g, 0, outs[-1], R[effort], (name, form, "lone", effort))
    trio = [nan_out(ew.outSize) for _ in es.GROUP_EFFORTS]
    ea.bucketMulGroup([(vd, ew, None, o, e) for o, e in zip(trio, es.GROUP_EFFORTS)])
    g.eval()
    for i, (o, e) in enumerate(zip(trio, es.GROUP_EFFORTS)):
        check(g, i, o, R[e], (name, form, "group of three", e))
    return outs + trio


def normed_input(ea, h, wn_d):
    """What effort_add_rmsnorm_mul writes for h and the norm weights: the input the fused prologue derives inside the launch."""
    from effort_amd import _lib
    g, lib = ea.gpu(), _lib.lib()
    n = h.shape[0]
    hd, hn = devf(h), torch.zeros(n, device=DEV)
    g._bind_stream()
    g.check(lib.effort_add_rmsnorm_mul(g.ctx, C.c_void_p(hd.data_ptr()), None, C.c_void_p(wn_d.data_ptr()), C.c_void_p(hn.data_ptr()), n), "rmsnorm")
    g.eval()
    assert torch.equal(hd.cpu(), torch.from_numpy(h))                      # (no delta: h itself is left alone)
    return hd, hn.cpu().numpy()


def fused_norm_and_residual(ea, oracle_cpu, d):
    """effort_bucketmul(_q4)_group_fused with the rmsNorm prologue and a residual: every effort in one launch, and one lone fused call."""
    g, lay, name = ea.gpu(), d["lay"], d["key"][1]
    inDim, outDim = lay["inDim"], lay["outDim"]
    wn_d = torch.from_numpy(structured_norm_w(inDim, seed=5)).to(DEV)
    hd, vn = normed_input(ea, make_v(inDim, seed=73, heavy=True), wn_d)
    R = refs(oracle_cpu, d, vn, "normed")
    resid = make_v(outDim, seed=74)
    rd = devf(resid)
    outs = [nan_out(outDim) for _ in es.EFFORTS]
    ea.bucketMulGroup([(hd, d["dense"], None, o, e, {"norm": wn_d, "resid": rd}) for o, e in zip(outs, es.EFFORTS)])
    g.eval()
    for i, (o, e) in enumerate(zip(outs, es.EFFORTS)):
        check(g, i, o, R[e], (name, "fused norm + residual", "group", e), resid)
    one = nan_out(outDim)
    ea.bucketMulGroup([(hd, d["aligned"], None, one, 0.25, {"norm": wn_d, "resid": rd})])
    g.eval()
    check(g, 0, one, R[0.25], (name, "fused norm + residual", "lone", 0.25), resid)
    assert torch.equal(rd.cpu(), torch.from_numpy(resid))


# ------------------------------------------------------------------------------------------------ FP16
@pytest.mark.parametrize("case", es.FP16_CASES, ids=[c.name for c in es.FP16_CASES])
def test_fp16_edge_shapes(ea, oracle_cpu, case):
    """Lone calls at every effort and a group of three, on the dense row pitch and after align_rows() -- 4-byte rows on 128-byte lines --
    bit-equal to one another."""
    d = case_data(ea, case)
    R = refs(oracle_cpu, d, d["v"])
    dense = lone_calls_and_a_group(ea, d, R, d["dense"], "dense pitch")
    aligned = lone_calls_and_a_group(ea, d, R, d["aligned"], "aligned rows")
    for i, (a, b) in enumerate(zip(dense, aligned)):
        assert torch.equal(a, b), (case.name, i)


DEEP = [c for c in es.FP16_CASES if c.deep]


@pytest.mark.parametrize("case", DEEP, ids=[c.name for c in DEEP])
def test_fp16_edge_shapes_as_persistent_group(ea, oracle_cpu, case):
    """set_persistent(1) and enough calls that the items outnumber the CUs: persistent workgroups pull items of several calls in turn (cutoff
    jobs at the head of the queues).  The geometry is pinned to the lone call's own, so the results equal the lone calls' bit for bit."""
    from effort_amd import runtime
    d = case_data(ea, case)
    R = refs(oracle_cpu, d, d["v"])
    g, ew, vd = ea.gpu(), d["dense"], devf(d["v"])
    numCU = torch.cuda.get_device_properties(0).multi_processor_count
    one = (case.inDim, case.outDim, 0.25, case.percentLoad)
    p1 = runtime.plan([one], numCU=numCU)
    tune = (p1["W"], p1["E"], p1["slices"][0])
    n = max(4, numCU // (p1["tiles"][0] * p1["slices"][0]) + 1)
    assert n <= 32
    efforts = [es.EFFORTS[(i + 2) % 4] for i in range(n)]
    pn = runtime.plan([one[:2] + (e, case.percentLoad) for e in efforts], numCU=numCU, persistent=1, waves=tune[0], elems=tune[1], slices=tune[2])
    assert pn["persistent"] == [1] and pn["slices"] == [tune[2]] * n and pn["sliceRows"] == p1["sliceRows"] * n
    try:
        g.set_tuning(*tune)
        singles = {}
        for e in es.EFFORTS:
            singles[e] = lone(ea, ew, vd, e)
            check(g, 0, singles[e], R[e], (case.name, "pinned geometry", "lone", e))
            assert g.last_variant()["persistent"] == 0
        g.set_persistent(1)
        for rep in range(2):                                               # (the queues rewind)
            outs = [nan_out(case.outDim) for _ in efforts]
            ea.bucketMulGroup([(vd, ew, None, o, e) for o, e in zip(outs, efforts)])
            g.eval()
            ran = g.last_variant()
            assert ran["persistent"] == 1 and ran["totalItems"] > ran["grid"] == numCU, ran
            for i, (o, e) in enumerate(zip(outs, efforts)):
                assert g.last_dispatch_count(i) == R[e]["count"] and np.float32(g.last_cutoff(i)).tobytes() == np.float32(R[e]["cutoff"]).tobytes(), (i, e)
                assert torch.equal(o, singles[e]), (case.name, rep, i, e)
    finally:
        g.set_persistent(-1)
        g.set_tuning(0, 0, 0)


@pytest.mark.parametrize("case", DEEP, ids=[c.name for c in DEEP])
def test_fp16_edge_shapes_with_the_norm_prologue(ea, oracle_cpu, case):
    """The fused rmsNorm prologue's tail loop (inputs past 4096, 1024 a trip) at 4097 and at 65535 inputs, with the residual epilogue."""
    fused_norm_and_residual(ea, oracle_cpu, case_data(ea, case))


# ------------------------------------------------------------------------------------------------ Q4
@pytest.mark.parametrize("case", es.Q4_CASES, ids=[c.name for c in es.Q4_CASES])
def test_q4_edge_shapes(ea, oracle_cpu, case):
    d = case_data(ea, case)
    R = refs(oracle_cpu, d, d["v"])
    dense = lone_calls_and_a_group(ea, d, R, d["dense"], "dense pitch")
    aligned = lone_calls_and_a_group(ea, d, R, d["aligned"], "aligned rows")
    for i, (a, b) in enumerate(zip(dense, aligned)):
        assert torch.equal(a, b), (case.name, i)
    if case.fused:
        fused_norm_and_residual(ea, oracle_cpu, d)


# ------------------------------------------------------------------------------------------------ effort -> q
@pytest.mark.parametrize("case", [es.BOUNDARY_FP16, es.BOUNDARY_Q4], ids=["fp16", "q4"])
def test_effort_boundaries_select_the_oracles_rows(ea, oracle_cpu, case):
    """q = Int(Double(4095) * (1 - effort)) (bucketMul.swift:39) on the host side of the launch: at effort = 1 - k / 4095, the doubles either
    side of it and a step of 1e-6 either side, where the quantile goes from k to k - 1; counts and cutoffs follow the oracle's exactly."""
    d = case_data(ea, case)
    lay, v, g = d["lay"], d["v"], ea.gpu()
    vd = devf(v)
    for k in es.BOUNDARY_KS:
        efforts = [e for kk, e in es.boundary_efforts() if kk == k]
        qs = [oracle_cpu.effort_to_q(e) for e in efforts]
        assert set(qs[:3]) <= {k, k - 1} and qs[3:] == [k - 1, k], (k, qs)
        for e in efforts:
            cutoff, _ = oracle_cpu.find_cutoff(v, lay["probes"], 0, e)
            if lay["q4"]:
                _, n = oracle_cpu.prepare_dispatch_q4(v, lay["stats"], 0, cutoff, lay["inDim"], 1)
            else:
                _, n = oracle_cpu.prepare_dispatch(v, lay["stats"], 0, cutoff, lay["inDim"], 1, lay["percentLoad"])
            lone(ea, d["dense"], vd, e)
            assert g.last_dispatch_count() == n and np.float32(g.last_cutoff()).tobytes() == np.float32(cutoff).tobytes(), (k, e)


def test_efforts_outside_0_1_are_refused_everywhere(ea):
    """-1e-9, 1 + 1e-9, NaN and inf at every multiply entry point: EFFORT_ERR_EFFORT, nothing enqueued, the output buffers untouched -- a
    group with one bad call launches none of its calls."""
    import effort_amd
    from effort_amd import _lib
    g, lib = ea.gpu(), _lib.lib()
    for case in (es.BOUNDARY_FP16, es.BOUNDARY_Q4):
        d = case_data(ea, case)
        ew, lay = d["dense"], d["lay"]
        q4, inDim, outDim = lay["q4"], lay["inDim"], lay["outDim"]
        vd = devf(d["v"])
        wn_d = torch.from_numpy(structured_norm_w(inDim, seed=5)).to(DEV)
        rd = devf(make_v(outDim, seed=74))
        disp = torch.full((lay["expertRows"], 2), float("nan"), device=DEV)
        count = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        for bad in es.BAD_EFFORTS:
            outs = [nan_out(outDim) for _ in range(8)]
            with pytest.raises(effort_amd.EffortError, match="EFFORT_ERR_EFFORT"):
                (ea.bucketMulQ4 if q4 else ea.bucketMul)(vd, ew, None, outs[0], bad)
            with pytest.raises(effort_amd.EffortError, match="EFFORT_ERR_EFFORT"):
                ea.bucketMulGroup([(vd, ew, None, outs[1], 0.25), (vd, ew, None, outs[2], 1.0), (vd, ew, None, outs[3], bad)])
            with pytest.raises(effort_amd.EffortError, match="EFFORT_ERR_EFFORT"):
                ea.bucketMulGroup([(vd, ew, None, outs[4], bad, {"norm": wn_d, "resid": rd}), (vd, ew, None, outs[5], 0.25, {"resid": rd})])
            with pytest.raises(effort_amd.EffortError, match="EFFORT_ERR_EFFORT"):
                ea.bucketMulGroup([(vd, ew, None, outs[6], bad, {"resid": rd})])
            g._bind_stream()
            rc = lib.effort_calc_dispatch(g.ctx, ew.handle, C.c_void_p(vd.data_ptr()), None, bad, C.c_void_p(disp.data_ptr()), C.c_void_p(count.data_ptr()))
            assert rc == -3, (bad, rc)
            g.eval()
            assert all(bool(torch.isnan(o).all()) for o in outs), bad
            assert bool(torch.isnan(disp).all()) and int(count[0]) == -7, bad
        # the borders themselves are efforts
        for ok in (0.0, 1.0):
            assert not torch.isnan(lone(ea, ew, vd, ok)).any()


# ------------------------------------------------------------------------------------------------ offsets next to 2^32
def test_expert_30_of_a_stack_of_3_875_gib(ea, oracle_cpu):
    """31 experts of 4096 x 16384 at percentLoad 16: 31 x 128 MiB of buckets, the largest stack registration takes (32 experts are 4 GiB).
    Experts 0 .. 29 hold one synthetic expert A, expert 30 another, B (copied on the device: the stack is never built on the host).  The rows
    of expert 30 start 3.75 GiB into the buffer: a bucket-row offset that wrapped or was cut to fewer than 32 bits would read rows of A -- and
    expNo = 30 must give B's product, count and cutoff.  The same pointers as 32 experts are refused before anything is read."""
    from effort_amd import _lib
    inDim, outDim, load, E = (es.STACK[k] for k in ("inDim", "outDim", "percentLoad", "experts"))
    rows, cols = inDim * load, outDim // 16
    need = E * rows * (cols * 2 + 8 + 4 + 2) + (1 << 30)                  # buckets, stats, registration's row scratch and means, and room to work
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip(f"the stack needs {need >> 20} MiB of device memory, {free >> 20} MiB are free")
    g, lib = ea.gpu(), _lib.lib()
    A, B = es.fp16_bundle(inDim, outDim, load, seed=1), es.fp16_bundle(inDim, outDim, load, seed=2)
    try:
        buckets = torch.empty((E, rows, cols), dtype=torch.int16, device=DEV)
        stats = torch.empty((E, rows, 4), dtype=torch.int16, device=DEV)
        probes = torch.empty((E, 4096), dtype=torch.int16, device=DEV)
        for dst, name in ((buckets, "buckets"), (stats, "stats"), (probes, "probes")):
            dst[:E - 1] = dev16(A[name])                                       # (broadcast over the experts, on the device)
            dst[E - 1] = dev16(B[name])
        ew = ea.ExpertWeights(buckets, stats, probes, inSize=inDim, outSize=outDim, percentLoad=load, numExperts=E)
        assert ew.handle and ew.buckets.data_ptr() == buckets.data_ptr()
        v = make_v(inDim, heavy=True)
        vd = devf(v)
        refB = {e: es.reference(oracle_cpu, B, v, e) for e in (0.25, 1.0)}
        refA = es.reference(oracle_cpu, A, v, 0.25)
        assert not close(refA["want"].astype(np.float32), refB[0.25]["want"])       # (A's product would not pass for B's)
        for expNo, ref, effort in ((E - 1, refB[0.25], 0.25), (E - 1, refB[1.0], 1.0), (0, refA, 0.25), (E - 2, refA, 0.25)):
            out = nan_out(outDim)
            ea.bucketMul(vd, ew, torch.tensor([expNo], dtype=torch.int32, device=DEV), out, effort)
            g.eval()
            check(g, 0, out, ref, ("stack of 31", f"expNo {expNo}", "lone", effort))
        P = lambda t: C.c_void_p(t.data_ptr())                                  # noqa: E731
        g._bind_stream()
        assert not lib.effort_weights_fp16(g.ctx, P(buckets), P(stats), P(probes), inDim, outDim, load, E + 1)
        assert b"unsupported shape" in lib.effort_last_error(g.ctx)
    finally:
        ew = buckets = stats = probes = None
        torch.cuda.empty_cache()
