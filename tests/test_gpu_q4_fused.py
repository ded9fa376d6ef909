"""effort_bucketmul_q4_group_fused on the GPU: the silu gate, the rmsNorm prologue and the residual epilogue folded into Q4 launches.
The derived input is what the glue kernels materialise, bit for bit, so cutoff and row selection are EXACTLY those of the
materialise-first path and of the CPU oracle (oracle.cpu.bucket_mul_q4 fed the materialised input copied back from the GPU); the
output is within the multiply's own bar (close(): 2e-5 * max|want|) of the oracle, and without outliers (integer accumulation, one
f32 add of the residual) it is the materialise-first path's to the bit.  The Q4 layout comes from the GPU converter
(tests/test_gpu_parity.py pins it byte-equal to oracle/q4_layout.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_parity import DEV, close, converted, devf, gpu_weights
from tests.util import make_v, make_w

pytestmark = pytest.mark.gpu

SHAPES = [(4096, 4096), (14336, 4096)]          # (inDim, outDim): the early LDS copy of v (<= 4096 inputs), the late one (<= 16384)
EFFORTS = (0.15, 0.25, 1.0)
_LAYOUTS = {}


@pytest.fixture(scope="module")
def ea(hip_lib_built):
    import effort_amd
    assert torch.cuda.is_available()
    effort_amd.gpu(0)
    return effort_amd


def layout(ea, inDim, outDim):
    """The GPU converter's Q4 layout of a Gaussian matrix, as numpy arrays for the oracle."""
    if (inDim, outDim) not in _LAYOUTS:
        W = make_w(outDim, inDim, seed=31 + inDim % 97)
        t = ea.q4_convert(torch.from_numpy(np.ascontiguousarray(W.T)).to(DEV))
        _LAYOUTS[(inDim, outDim)] = {"buckets": t["buckets"].cpu().numpy().view(np.uint16), "bucket.stats": t["bucket.stats"].cpu().numpy(),
                                     "probes": t["probes"].cpu().numpy().view(np.uint16)[:4096].copy(), "outliers": t["outliers"].cpu().numpy()}
    return _LAYOUTS[(inDim, outDim)]


def bundle(ea, L, inDim, outDim, with_outliers):
    return ea.ExpertWeights(torch.from_numpy(L["buckets"].view(np.int16)).to(DEV), devf(L["bucket.stats"]), torch.from_numpy(L["probes"].view(np.int16)).to(DEV),
                            inSize=inDim, outSize=outDim, outliers=devf(L["outliers"]) if with_outliers else None, q4=True)


def oracle(oracle_cpu, L, v, inDim, outDim, effort, with_outliers):
    return oracle_cpu.bucket_mul_q4(v.cpu().numpy(), L["buckets"], L["bucket.stats"], L["probes"].view(np.float16), L["outliers"] if with_outliers else None,
                                    inDim, outDim, effort)


def P(t):
    return C.c_void_p(t.data_ptr())


def silu(ea, x1, x3):
    from effort_amd import _lib
    g = ea.gpu()
    x2 = torch.zeros_like(x1)
    g._bind_stream()
    g.check(_lib.lib().effort_silu_mul(g.ctx, P(x1), P(x3), P(x2), x1.numel()), "silu")
    return x2


def rmsnorm(ea, h, wn):
    from effort_amd import _lib
    g = ea.gpu()
    hn, hc = torch.zeros_like(h), h.clone()
    g._bind_stream()
    g.check(_lib.lib().effort_add_rmsnorm_mul(g.ctx, P(hc), None, P(wn), P(hn), h.numel()), "rmsnorm")
    return hn


def norm_weights(inDim):
    return torch.from_numpy((1 + 0.1 * np.random.default_rng(5).standard_normal(inDim)).astype(np.float16)).to(DEV)


@pytest.mark.parametrize("with_outliers", [True, False])
@pytest.mark.parametrize("inDim,outDim", SHAPES)
def test_silu_gate_and_residual(ea, oracle_cpu, inDim, outDim, with_outliers):
    """{"gate": x3, "resid": out} in place against effort_silu_mul then bucketMulQ4."""
    L = layout(ea, inDim, outDim)
    ew = bundle(ea, L, inDim, outDim, with_outliers)
    g = ea.gpu()
    x1, x3 = devf(make_v(inDim, seed=71)), devf(make_v(inDim, seed=72, heavy=True))
    resid = devf(make_v(outDim, seed=74))
    x2 = silu(ea, x1, x3)
    for effort in EFFORTS:
        plain = torch.full((outDim,), float("nan"), device=DEV)
        ea.bucketMulQ4(x2, ew, None, plain, effort)
        g.eval()
        n0, c0 = g.last_dispatch_count(), g.last_cutoff()
        want, n_or, c_or = oracle(oracle_cpu, L, x2, inDim, outDim, effort, with_outliers)
        assert n0 == n_or and c0 == c_or, effort
        fused = resid.clone()
        ea.bucketMulGroup([(x1, ew, None, fused, effort, {"gate": x3, "resid": fused})])            # out = resid + product, in place
        g.eval()
        n1, c1 = g.last_dispatch_count(), g.last_cutoff()
        print(f"gate {inDim}->{outDim} outliers={with_outliers} effort={effort}: rows {n1} (oracle {n_or}) cutoff {c1} (oracle {c_or}) "
              f"max|fused - (resid + want)| / max|want| = {float(np.abs(fused.cpu().numpy() - (resid.cpu().numpy() + want)).max() / np.abs(want).max()):.3e}")
        assert n1 == n0 == n_or and c1 == c0 == c_or, effort
        assert close(fused.cpu().numpy(), resid.cpu().numpy() + want), effort
        if not with_outliers:
            assert torch.equal(fused, resid + plain), effort
        else:
            assert close(fused.cpu().numpy(), (resid + plain).cpu().numpy()), effort


@pytest.mark.parametrize("with_outliers", [True, False])
@pytest.mark.parametrize("inDim,outDim", SHAPES)
def test_rmsnorm_prologue(ea, oracle_cpu, inDim, outDim, with_outliers):
    """{"norm": w} against effort_add_rmsnorm_mul then bucketMulQ4; also from 256, 1024 and 128 threads standing for that kernel's 1024."""
    L = layout(ea, inDim, outDim)
    ew = bundle(ea, L, inDim, outDim, with_outliers)
    g = ea.gpu()
    hvec, wn = devf(make_v(inDim, seed=73, heavy=True)), norm_weights(inDim)
    hn = rmsnorm(ea, hvec, wn)
    for effort in EFFORTS:
        plain = torch.full((outDim,), float("nan"), device=DEV)
        ea.bucketMulQ4(hn, ew, None, plain, effort)
        g.eval()
        n0, c0 = g.last_dispatch_count(), g.last_cutoff()
        want, n_or, c_or = oracle(oracle_cpu, L, hn, inDim, outDim, effort, with_outliers)
        assert n0 == n_or and c0 == c_or, effort
        fused = torch.full((outDim,), float("nan"), device=DEV)
        ea.bucketMulGroup([(hvec, ew, None, fused, effort, {"norm": wn})])
        g.eval()
        print(f"norm {inDim}->{outDim} outliers={with_outliers} effort={effort}: rows {g.last_dispatch_count()} (oracle {n_or}) cutoff {g.last_cutoff()} (oracle {c_or})")
        assert g.last_dispatch_count() == n0 and g.last_cutoff() == c0, effort               # exact: same input bits
        assert close(fused.cpu().numpy(), want), effort
        if not with_outliers:
            assert torch.equal(fused, plain), effort
    want, n_or, c_or = oracle(oracle_cpu, L, hn, inDim, outDim, 0.25, with_outliers)
    for tune in ((4, 2, 0), (16, 1, 0), (2, 4, 0)):
        g.set_tuning(*tune)
        try:
            f3 = torch.full((outDim,), float("nan"), device=DEV)
            ea.bucketMulGroup([(hvec, ew, None, f3, 0.25, {"norm": wn})])
            g.eval()
            assert g.last_dispatch_count(0) == n_or and g.last_cutoff(0) == c_or and close(f3.cpu().numpy(), want), tune
        finally:
            g.set_tuning(0, 0, 0)


@pytest.mark.parametrize("with_outliers", [True, False])
def test_group_of_fused_and_plain_calls(ea, oracle_cpu, with_outliers):
    """Two fused Q4 calls (gate + resid; norm) and one plain Q4 call in ONE launch: every call's hooks and outputs."""
    inDim, outDim = 4096, 4096
    L = layout(ea, inDim, outDim)
    ews = [bundle(ea, L, inDim, outDim, with_outliers) for _ in range(3)]
    g = ea.gpu()
    x1, x3 = devf(make_v(inDim, seed=81)), devf(make_v(inDim, seed=82, heavy=True))
    hvec, wn = devf(make_v(inDim, seed=83, heavy=True)), norm_weights(inDim)
    vp = devf(make_v(inDim, seed=84))
    resid = devf(make_v(outDim, seed=85))
    x2, hn = silu(ea, x1, x3), rmsnorm(ea, hvec, wn)
    outs = [torch.full((outDim,), float("nan"), device=DEV) for _ in range(3)]
    ea.bucketMulGroup([(x1, ews[0], None, outs[0], 0.25, {"gate": x3, "resid": resid}),
                       (hvec, ews[1], None, outs[1], 0.15, {"norm": wn}),
                       (vp, ews[2], None, outs[2], 1.0)])
    g.eval()
    for k, (vin, effort, add) in enumerate(((x2, 0.25, resid), (hn, 0.15, None), (vp, 1.0, None))):
        want, n, cutoff = oracle(oracle_cpu, L, vin, inDim, outDim, effort, with_outliers)
        assert g.last_dispatch_count(k) == n and g.last_cutoff(k) == cutoff, k
        if add is not None:
            want = add.cpu().numpy() + want
        assert close(outs[k].cpu().numpy(), want), k


@pytest.mark.parametrize("with_outliers", [True, False])
def test_dependent_pair_on_lanes(ea, oracle_cpu, with_outliers):
    """effort_set_overlap(4): a fused w2 whose resid is the previous launch's output must wait for it (the hazard ranges cover
    resid and aux).  Against lanes = 1: equal bits without outliers, the multiply's bar with them (the outlier sums follow the
    launch geometry, which follows the lanes setting)."""
    inDim, outDim = 4096, 4096
    L = layout(ea, inDim, outDim)
    wa, wb = bundle(ea, L, inDim, outDim, with_outliers), bundle(ea, L, inDim, outDim, with_outliers)
    g = ea.gpu()
    v0 = devf(make_v(inDim, seed=91))
    x1, x3 = devf(make_v(inDim, seed=92)), devf(make_v(inDim, seed=93, heavy=True))

    def run():
        h = torch.full((outDim,), float("nan"), device=DEV)
        out = torch.full((outDim,), float("nan"), device=DEV)
        ea.bucketMulQ4(v0, wa, None, h, 0.25)                                                       # h = wa(v0)
        ea.bucketMulGroup([(x1, wb, None, out, 0.25, {"gate": x3, "resid": h})])                    # out = h + wb(silu(x1) * x3)
        g.eval()
        return out.clone()
    one = run()
    g.set_overlap(4)
    try:
        four = [run() for _ in range(3)]
    finally:
        g.set_overlap(1)
    for o in four:
        assert torch.isfinite(o).all()
        if with_outliers:
            assert close(o.cpu().numpy(), one.cpu().numpy())
        else:
            assert torch.equal(o, one)


@pytest.mark.parametrize("with_outliers", [True, False])
@pytest.mark.parametrize("inDim,outDim", SHAPES)
def test_in_place_and_repeatable(ea, oracle_cpu, inDim, outDim, with_outliers):
    """resid aliasing out equals the run with a separate resid (no store to out precedes the read of resid: the Q4 call's implied
    out.zero() is not visible), and the same launch twice gives the same bits, outliers included."""
    L = layout(ea, inDim, outDim)
    ew = bundle(ea, L, inDim, outDim, with_outliers)
    g = ea.gpu()
    x1, x3 = devf(make_v(inDim, seed=61)), devf(make_v(inDim, seed=62, heavy=True))
    resid = devf(make_v(outDim, seed=63))
    buf = torch.full((3 * outDim,), float("nan"), device=DEV)                                       # NaN either side of the vector
    sep = buf[outDim:2 * outDim]
    ea.bucketMulGroup([(x1, ew, None, sep, 0.25, {"gate": x3, "resid": resid})])
    g.eval()
    first = sep.clone()
    assert torch.isfinite(first).all() and torch.isnan(buf[:outDim]).all() and torch.isnan(buf[2 * outDim:]).all()
    sep.copy_(resid)
    ea.bucketMulGroup([(x1, ew, None, sep, 0.25, {"gate": x3, "resid": sep})])                      # in place
    g.eval()
    assert torch.isfinite(sep).all() and torch.equal(sep, first)
    assert torch.isnan(buf[:outDim]).all() and torch.isnan(buf[2 * outDim:]).all()
    again = torch.full((outDim,), float("nan"), device=DEV)
    ea.bucketMulGroup([(x1, ew, None, again, 0.25, {"gate": x3, "resid": resid})])
    g.eval()
    assert torch.equal(again, first)
    only = torch.full((outDim,), float("nan"), device=DEV)                                          # a residual alone
    plain = torch.full((outDim,), float("nan"), device=DEV)
    x2 = silu(ea, x1, x3)
    ea.bucketMulGroup([(x2, ew, None, only, 0.25, {"resid": resid})])
    ea.bucketMulQ4(x2, ew, None, plain, 0.25)
    g.eval()
    assert torch.equal(only, resid + plain) if not with_outliers else close(only.cpu().numpy(), (resid + plain).cpu().numpy())


def test_refusals(ea, oracle_cpu):
    """A prologue on a Q4 handle WITH outliers whose input the outlier phase cannot keep in LDS (inDim > 16384) is EFFORT_ERR_SHAPE
    and enqueues nothing; the same bundle without outliers works, and so does a residual alone with them; the FP16 entry keeps
    refusing Q4 handles."""
    from effort_amd import _lib
    inDim, outDim = 20480, 4096
    rng = np.random.default_rng(inDim + outDim)
    rows, cols = inDim * 8, outDim // 32
    buckets = rng.integers(0, 65536, size=(rows, cols), dtype=np.uint16)              # (any nibble pattern is a valid bucket word)
    mean = np.abs(rng.normal(0, 0.02, size=rows)).astype(np.float32)
    stats = np.stack([mean, mean], axis=1)
    probes = rng.normal(0, 0.02, size=4096).astype(np.float16)
    ol = np.zeros((5000, 4), np.float32)
    ol[:, 0] = rng.normal(0, 0.3, size=5000).astype(np.float16)
    ol[:, 1] = rng.integers(0, inDim, size=5000)
    ol[:, 2] = rng.integers(0, outDim, size=5000)
    mk = lambda o: ea.ExpertWeights(torch.from_numpy(buckets.view(np.int16)).to(DEV), devf(stats), torch.from_numpy(probes.view(np.int16)).to(DEV),      # noqa: E731
                                    inSize=inDim, outSize=outDim, outliers=None if o is None else devf(o), q4=True)
    with_ol, without = mk(ol), mk(None)
    g = ea.gpu()
    x1, x3 = devf(make_v(inDim, seed=51)), devf(make_v(inDim, seed=52))
    resid = devf(make_v(outDim, seed=53))
    out = torch.full((outDim,), float("nan"), device=DEV)
    with pytest.raises(_lib.EffortError) as err:
        ea.bucketMulGroup([(x1, with_ol, None, out, 0.25, {"gate": x3})])
    assert err.value.code == -2                                                       # EFFORT_ERR_SHAPE
    g.eval()
    assert torch.isnan(out).all()                                                     # nothing was enqueued
    x2 = silu(ea, x1, x3)
    want, n, cutoff = oracle_cpu.bucket_mul_q4(x2.cpu().numpy(), buckets, stats, probes, None, inDim, outDim, 0.25)
    ea.bucketMulGroup([(x1, without, None, out, 0.25, {"gate": x3, "resid": resid})])
    g.eval()
    assert g.last_dispatch_count() == n and g.last_cutoff() == cutoff
    assert close(out.cpu().numpy(), resid.cpu().numpy() + want)
    want_ol, n, cutoff = oracle_cpu.bucket_mul_q4(x2.cpu().numpy(), buckets, stats, probes, ol, inDim, outDim, 0.25)
    ea.bucketMulGroup([(x2, with_ol, None, out, 0.25, {"resid": resid})])             # a residual alone: any size (v is gathered from memory, untransformed)
    g.eval()
    assert g.last_dispatch_count() == n and g.last_cutoff() == cutoff
    assert close(out.cpu().numpy(), resid.cpu().numpy() + want_ol)
    # the FP16 entry point on a Q4 handle: EFFORT_ERR_KIND, as before
    lib = _lib.lib()
    small = bundle(ea, layout(ea, 4096, 4096), 4096, 4096, False)
    v, o2 = devf(make_v(4096, seed=54)), torch.zeros(4096, device=DEV)
    Pp = C.c_void_p * 1
    g._bind_stream()
    h = small.handle
    rc = lib.effort_bucketmul_group_fused(g.ctx, 1, Pp(h.value if hasattr(h, "value") else h), Pp(v.data_ptr()), Pp(None), Pp(o2.data_ptr()), (C.c_double * 1)(0.25),
                                          (C.c_int * 1)(0), Pp(None), Pp(o2.data_ptr()))
    assert rc == -5                                                                   # EFFORT_ERR_KIND
    # and a mixed group is still refused up front
    with pytest.raises(ValueError):
        ea.bucketMulGroup([(v, small, None, o2, 0.25, {"resid": o2}), (v, gpu_weights(ea, *converted(oracle_cpu, 256, 4096)), None, torch.zeros(256, device=DEV), 0.25)])
