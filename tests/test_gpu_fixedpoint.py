"""bucketMul's fixed-point sums on the GPU against float64 (tests/fixedpoint_reference.py), on weight scales that strain the scale.

Every case passes three checks:
  * HARD ENVELOPE  |gpu - f64| <= envelope for every output, nothing excluded (the worst case of the documented scheme);
  * MEAN OF z      z = (gpu - f64) / sigma over the outputs: |mean z| within the family's bar;
  * RMS OF z       within the family's bar.
The two statistical bars of a family are TWICE the largest value the CPU emulation of the documented scheme
(tests/test_fixedpoint_reference_cpu.py: emulate) reaches over the family's cases, on the same inputs, selection and slices.  The
emulation lacks only the kernel's order of adding the slices' f32 values, which the envelope's last term covers.

The selection (cutoff, rows) is the oracle's integer work, pinned bit-exact elsewhere; count and cutoff are asserted equal again, and
the kept rows per slice are compared with what the launch reports, which pins the slice geometry the model assumes.  The layouts come
from the project's GPU converters (bit-exact with the oracle's, test_gpu_parity.py), read back to the host.

Measured on an MI355X, worst case of each family over its cases (the bars are twice the emulation's column; run with -s for every case):

    family (test)                  emulation |mean z|  rms z     GPU |mean z|  rms z    GPU max |err| / envelope
    gauss                                    0.3010   0.8860         0.3009   0.8859    0.102
    structured                               0.1331   1.0092         0.1331   1.0092    0.127
    structured_heavy                         0.0948   1.0228         0.0948   1.0228    0.126
    channel                                  0.1173   1.0436         0.1173   1.0436    0.097
    channel_v0                               0.1193   1.0716         0.1193   1.0716    0.096
    lone_v0                                  0.1177   1.0831         0.1177   1.0831    0.097
    subnormal                                0.4233   0.8997         0.4233   0.8997    0.093
    large                                    0.2919   0.8858         0.2919   0.8858    0.102
    flat                                     0.1226   0.2338         0.1361   0.2225    0.068
    input scales (k = 99, 100, -84, -83)     0.2919   1.0317         0.2919   1.0317    0.136
    experts x1, x1/64, x64                   0.1433   1.0360         0.1433   1.0360    0.075
    percentLoad 8, 3                         0.0651   0.9534         0.0651   0.9534    0.089
    group of x64 and x1/64                   0.0861   0.3328         0.0861   0.3328    0.065
    fused rmsNorm call                       0.0713   0.2882         0.0710   0.2882    0.059
    bound doubled by hand                    0.0020   0.9998         0.0020   0.9998    0.071
    q4 structured_heavy                      0.0004   0.0755         0.0003   0.0750    0.057
    q4 channel                               0.0005   0.0265         0.0004   0.0235    0.090
    q4 subnormal                             0.0004   0.0269         0.0004   0.0268    0.045
    q4 large                                 0.0004   0.0268         0.0004   0.0267    0.046
    q4 gauss                                 0.0010   0.0501         0.0010   0.0500    0.046

With 8 slices the grid roundings dominate sigma and the GPU equals the emulation to the digits shown: the kernels are the documented
scheme.  With 32 or 64 slices, and in Q4 (f32 outlier sums), the f32 terms -- taken at their bound in sigma -- dominate, rms z is far
below 1 and the two differ by the order of the f32 additions.  mean z is above zero by design: floor(x + 0.5) sends exact halves up
(test_fixedpoint_reference_cpu.mean_limit).  max |err| / max|out| per family and slice count: DESIGN.md 2.1 -- ``structured`` at 8
slices, ``channel`` and ``lone`` at every slice count exceed the 2e-5 of test_gpu_parity.close() INSIDE the envelope: a finding about
the bound (a worst case over every input channel), not a defect of the kernel.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import fixedpoint_reference as fr
from tests.test_fixedpoint_reference_cpu import (COSINE_SIZES, EFFORTS, FP16_FAMILIES, SLICES, cosine_pairs, emulate, family_bars,
                                                 layout_bound, model_kw, select)
from tests.util import family_v, family_w, structured_norm_w

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def ea(hip_lib_built):
    import effort_amd
    assert torch.cuda.is_available()
    effort_amd.gpu(0)
    return effort_amd


def devf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


_W = {}


def gpu_fp16(ea, family, outDim, inDim, mult=1.0, seed=1234):
    """(ExpertWeights, host layout) of a family matrix through the GPU converter."""
    key = (family, outDim, inDim, mult, seed)
    if key not in _W:
        W = family_w(family, outDim, inDim, seed, mult)
        ew = ea.ExpertWeights.from_core(torch.from_numpy(W).to(DEV))
        ea.gpu().eval()
        assert ea.gpu().convert_status() == 0
        _W[key] = (ew, host_layout(ew))
    return _W[key]


def host_layout(ew, percentLoad=None):
    cols = ew.buckets.shape[2]
    pl = percentLoad or ew.percentLoad
    lay = {"q4": ew.q4, "inDim": ew.inSize, "outDim": ew.outSize, "percentLoad": pl, "expertRows": ew.inSize * pl,
           "buckets": ew.buckets.cpu().numpy().view(np.uint16).reshape(-1, cols),
           "probes": ew.probes.cpu().numpy().view(np.float16).reshape(-1)}
    if ew.q4:
        lay["stats"] = ew.stats.cpu().numpy().reshape(-1, 2)
        lay["outliers"] = None if ew.outliers is None else ew.outliers.cpu().numpy()
    else:
        lay["stats"] = ew.stats.cpu().numpy().view(np.float16).reshape(-1, 4)
    return lay


def plan_slice_rows(ea, lay, effort, slices, **kw):
    from effort_amd import runtime
    numCU = torch.cuda.get_device_properties(0).multi_processor_count
    plan = runtime.plan([(lay["inDim"], lay["outDim"], effort, lay["percentLoad"])], q4=lay["q4"], numCU=numCU, lanes=1, slices=slices, **kw)
    return plan["sliceRows"][0], plan["slices"][0]


def relerr(got, model):
    return float(np.abs(got - model["f64"]).max() / max(float(np.abs(model["f64"]).max()), 1e-300))


def check_call(ea, oracle_cpu, ew, lay, v, effort, slices=0, expNo=0, rank_bound=None, tag=""):
    """One multiply on the GPU against the model; returns (gpu stats, emulation stats, max err / max|out| of the gpu), the hard
    envelope asserted here."""
    g = ea.gpu()
    B, S = plan_slice_rows(ea, lay, effort, slices)
    rows, cutoff = select(oracle_cpu, v, lay, effort, expNo)
    assert rows.size > 0 and np.isfinite(cutoff), tag
    rb = layout_bound(lay, expNo) if rank_bound is None else rank_bound
    model = fr.error_model(v, lay["buckets"], rows, lay["outDim"], rb, B, **model_kw(lay))
    out = torch.full((lay["outDim"],), float("nan"), device=DEV)
    e_t = None if expNo == 0 and ew.numExperts == 1 else torch.tensor([expNo], dtype=torch.int32, device=DEV)
    g.set_tuning(0, 0, slices)
    try:
        (ea.bucketMulQ4 if lay["q4"] else ea.bucketMul)(devf(v), ew, e_t, out, effort)
        g.eval()
    finally:
        g.set_tuning(0, 0, 0)
    assert g.last_dispatch_count() == rows.size and np.float32(g.last_cutoff()).tobytes() == np.float32(cutoff).tobytes(), tag
    assert g.slice_counts() == model["counts"] and len(model["counts"]) == S, (tag, B, S)      # the slices the model assumes are the launch's
    got = out.cpu().numpy()
    st = fr.z_stats(got, model)
    em = fr.z_stats(emulate(v, lay["buckets"], rows, lay["outDim"], rb, B, **model_kw(lay)), model)
    print(f"{tag:44s} S {S:3d} k {min(s[3] for s in model['slices']):4d}..{max(s[3] for s in model['slices']):4d}  "
          f"emul {em[1]:+.4f} {em[2]:.4f} {em[0]:.3f}  gpu {st[1]:+.4f} {st[2]:.4f} {st[0]:.3f}  err/max|out| {relerr(got, model):.2e}")
    assert st[0] <= 1.0, (tag, "outside the hard envelope", st)
    return st, em, got, model


def assert_bars(results, family):
    bar_mean, bar_rms = family_bars([em for _, em in results])
    print(f"{family}: emulation worst {bar_mean / 2:.4f} {bar_rms / 2:.4f} (the bars are twice these);  gpu worst "
          f"{max(abs(st[1]) for st, _ in results):.4f} {max(st[2] for st, _ in results):.4f} {max(st[0] for st, _ in results):.3f}")
    for st, _ in results:
        assert abs(st[1]) <= bar_mean and st[2] <= bar_rms, (family, st, bar_mean, bar_rms)


CROSS = [(e, s) for e in EFFORTS for s in SLICES]
THIN = [(0.25, 0), (1.0, 8), (0.1, 64)]


# ------------------------------------------------------------------------------------------------ FP16 families
@pytest.mark.parametrize("family", list(FP16_FAMILIES))
def test_fp16_families(ea, oracle_cpu, family):
    """(256, 4096): every effort x slice count; (1024, 4500), ragged last slice: the same for the control and the heaviest family, three
    cases for the others."""
    wf, vkw = FP16_FAMILIES[family]
    results = []
    for (outDim, inDim), cases in (((256, 4096), CROSS), ((1024, 4500), CROSS if family in ("gauss", "structured_heavy") else THIN)):
        ew, lay = gpu_fp16(ea, wf, outDim, inDim)
        v = family_v(inDim, seed=42, **vkw)
        for effort, slices in cases:
            st, em, _, _ = check_call(ea, oracle_cpu, ew, lay, v, effort, slices, tag=f"{family} {outDim}x{inDim} e{effort} s{slices}")
            results.append((st, em))
    assert_bars(results, family)


def test_fp16_input_scales_across_the_clamp(ea, oracle_cpu):
    """The input scaled by 2^e.  k is clamped to [-100, 100].  Upper clamp: with eight slices, one scale at which the coarsest slice
    sits at k = 99 (no slice is clamped: the unclamped k is at most 100) and one eight times smaller, where every slice is (unclamped
    102 or more).  Lower clamp: k = 29 - floor(log2 L) >= 29 - 127 for every finite f32 L, so -100 is out of reach; the largest scale
    is taken at which the cutoff's own arithmetic on 100000 * |v| * mean stays finite with 2^8 to spare (an infinite cutoff selects
    nothing; NaN / Inf are out of scope), and half of it: k near -84."""
    ew, lay = gpu_fp16(ea, "gauss", 256, 4096)
    v0 = family_v(4096, seed=42)
    B, _ = plan_slice_rows(ea, lay, 0.25, 8)
    E_max = max(int(np.floor(np.log2(L))) for _, _, L, _ in fr.slice_exponents(v0, layout_bound(lay), B))
    biggest = max(float(np.abs(lay["probes"].astype(np.float32)).max()), float(np.abs(lay["stats"].astype(np.float32)).max()))
    e_top = int(np.floor(np.log2(2.0 ** 120 / (1.0e5 * float(np.abs(v0).max()) * biggest))))      # (2^8 of room: the bisection adds its bounds)
    results = []
    for e, want in ((-70 - E_max, "below"), (-73 - E_max, "clamped"), (e_top, "top"), (e_top - 1, "top")):
        v = np.ldexp(v0, e).astype(np.float32)
        assert np.isfinite(v).all() and (v != 0).sum() == (v0 != 0).sum()
        st, em, _, model = check_call(ea, oracle_cpu, ew, lay, v, 0.25, 8, tag=f"gauss 256x4096 v*2^{e}")
        ks = [s[3] for s in model["slices"]]
        unclamped = [29 - int(np.floor(np.log2(s[2]))) for s in model["slices"]]
        if want == "below":
            assert min(ks) == 99 and max(unclamped) <= 100
        elif want == "clamped":
            assert set(ks) == {100} and min(unclamped) >= 102
        else:
            assert max(ks) < -75
        results.append((st, em))
    assert_bars(results, "input scales")


def test_fp16_experts_and_percentload(ea, oracle_cpu):
    """Experts at x1, x1/64 and x64 in one stack, every expNo (a kernel reading expert 0's bound for all of them multiplies the
    x1/64 expert on a grid 64 times too coarse); percentLoad 8 and 3."""
    parts = [gpu_fp16(ea, "structured", 256, 4096, mult=m, seed=100 + i) for i, m in enumerate((1.0, 1.0 / 64.0, 64.0))]
    stacked = ea.ExpertWeights.stack([p[0] for p in parts])
    lay = host_layout(stacked)
    assert lay["buckets"].shape[0] == 3 * 4096 * 16
    v = family_v(4096, seed=42, heavy=True)
    results = []
    for e in range(3):
        for slices in (0, 8):
            st, em, _, _ = check_call(ea, oracle_cpu, stacked, lay, v, 0.25, slices, expNo=e, tag=f"expert {e} s{slices}")
            results.append((st, em))
    assert_bars(results, "experts")
    results = []
    for pl in (8, 3):
        ewt = parts[0][0].truncated(pl)
        layt = host_layout(ewt)
        for slices in (0, 8):
            st, em, _, _ = check_call(ea, oracle_cpu, ewt, layt, v, 0.6, slices, tag=f"percentLoad {pl} s{slices}")
            results.append((st, em))
    assert_bars(results, "percentLoad")


def _group(ea, oracle_cpu, calls, tune, persistent, tag):
    """calls: [(ew, lay, v, effort, extras, v_model)]; one group launch, every call against its model."""
    from effort_amd import runtime
    g = ea.gpu()
    numCU = torch.cuda.get_device_properties(0).multi_processor_count
    plan = runtime.plan([(l["inDim"], l["outDim"], eff, l["percentLoad"], 2 if x else 0, 0) for _, l, _, eff, x, _ in calls], q4=False,
                        numCU=numCU, lanes=1, persistent=persistent, waves=tune[0], elems=tune[1], slices=tune[2])
    outs = [torch.full((l["outDim"],), float("nan"), device=DEV) for _, l, _, _, _, _ in calls]
    g.set_tuning(*tune)
    g.set_persistent(persistent)
    try:
        ea.bucketMulGroup([(devf(v), ew, None, o, eff) + ((x,) if x else ()) for (ew, _, v, eff, x, _), o in zip(calls, outs)])
        g.eval()
    finally:
        g.set_persistent(-1)
        g.set_tuning(0, 0, 0)
    results = []
    for i, ((ew, lay, v, eff, x, vm), o) in enumerate(zip(calls, outs)):
        rows, cutoff = select(oracle_cpu, vm, lay, eff)
        B, rb = plan["sliceRows"][i], layout_bound(lay)
        model = fr.error_model(vm, lay["buckets"], rows, lay["outDim"], rb, B, **model_kw(lay))
        assert g.last_dispatch_count(i) == rows.size and np.float32(g.last_cutoff(i)).tobytes() == np.float32(cutoff).tobytes(), (tag, i)
        assert g.slice_counts(i) == model["counts"], (tag, i)
        got = o.cpu().numpy()
        st = fr.z_stats(got, model)
        em = fr.z_stats(emulate(vm, lay["buckets"], rows, lay["outDim"], rb, B, **model_kw(lay)), model)
        print(f"{tag} call {i}: S {len(model['counts'])} emul {em[1]:+.4f} {em[2]:.4f} {em[0]:.3f}  gpu {st[1]:+.4f} {st[2]:.4f} {st[0]:.3f}  "
              f"err/max|out| {relerr(got, model):.2e}")
        assert st[0] <= 1.0, (tag, i, st)
        results.append((st, em))
    return results, plan


def test_fp16_group_of_two_scales(ea, oracle_cpu):
    """A x64 and a x1/64 matrix side by side in one launch, plain and as persistent workgroups (one workgroup then takes items of
    both matrices in turn: each item must be summed on its own matrix's grid)."""
    big, small = gpu_fp16(ea, "structured", 256, 4096, mult=64.0), gpu_fp16(ea, "structured", 256, 4096, mult=1.0 / 64.0, seed=77)
    v = family_v(4096, seed=42, heavy=True)
    two = [(big[0], big[1], v, 0.25, None, v), (small[0], small[1], v, 0.25, None, v)]
    results, plan = _group(ea, oracle_cpu, two, (0, 0, 0), 0, "group plain")
    assert plan["persistent"] == [0]
    more, plan = _group(ea, oracle_cpu, two * 4, (8, 1, 64), 1, "group persistent")
    assert plan["persistent"][0] > 0, plan
    assert_bars(results + more, "group")


def test_fp16_fused_norm_call(ea, oracle_cpu):
    """One fused call: the input is rmsNorm(h) * w evaluated inside the launch, w with the spread of trained norm weights.  The
    reference's input is what effort_add_rmsnorm_mul writes (pinned bit-equal with the fused prologue, test_gpu_parity.py)."""
    from effort_amd import _lib
    ew, lay = gpu_fp16(ea, "structured", 1024, 4096)
    g, lib = ea.gpu(), _lib.lib()
    h = family_v(4096, seed=73, heavy=True)
    wn = torch.from_numpy(structured_norm_w(4096, seed=5)).to(DEV)
    hd, hn = devf(h), torch.zeros(4096, device=DEV)
    g._bind_stream()
    g.check(lib.effort_add_rmsnorm_mul(g.ctx, C.c_void_p(hd.data_ptr()), None, C.c_void_p(wn.data_ptr()), C.c_void_p(hn.data_ptr()), 4096), "rmsnorm")
    g.eval()
    assert torch.equal(hd.cpu(), torch.from_numpy(h))                       # (no delta: h itself is left alone)
    results, _ = _group(ea, oracle_cpu, [(ew, lay, h, 0.25, {"norm": wn}, hn.cpu().numpy())], (0, 0, 0), -1, "fused norm")
    assert_bars(results, "fused norm")


# ------------------------------------------------------------------------------------------------ Q4
_Q4 = {}


def gpu_q4(ea, family, seed=31):
    if family not in _Q4:
        W = family_w(family, 4096, 4096, seed)
        ew = ea.ExpertWeights.from_core_q4(torch.from_numpy(W).to(DEV))
        ea.gpu().eval()
        _Q4[family] = (ew, host_layout(ew))
    return _Q4[family]


Q4_THIN = [(0.25, 0), (0.25, 8), (0.1, 64)]


@pytest.mark.parametrize("family,cases", [("structured_heavy", Q4_THIN + [(0.1, 0), (0.25, 64), (1.0, 0)]), ("channel", Q4_THIN),
                                          ("subnormal", Q4_THIN), ("large", Q4_THIN), ("gauss", Q4_THIN + [(1.0, 8)])])
def test_q4_families(ea, oracle_cpu, family, cases):
    """4096 x 4096 (the smallest shape whose probes exist), the outlier table included.  (The Q4 converter makes outliers of the
    largest 2 % of the weights: ``lone`` and ``channel`` with a zero input on the large channel are ``gauss`` again to the bit, so
    ``channel`` runs with its input alive -- the whole channel then goes through the f32 outlier sums.)"""
    wf, vkw = FP16_FAMILIES[family]
    ew, lay = gpu_q4(ea, wf)
    assert lay["outliers"] is not None and len(lay["outliers"]) == int(4096 * 4096 * 0.02)
    v = family_v(4096, seed=42, **vkw)
    results = []
    for effort, slices in cases:
        st, em, _, _ = check_call(ea, oracle_cpu, ew, lay, v, effort, slices, tag=f"q4 {family} e{effort} s{slices}")
        results.append((st, em))
    assert_bars(results, "q4 " + family)


# ------------------------------------------------------------------------------------------------ the bound's getters and setters
def test_rank_bound_getters_and_setters(ea, oracle_cpu):
    parts = [gpu_fp16(ea, "structured", 256, 4096, mult=m, seed=100 + i) for i, m in enumerate((1.0, 1.0 / 64.0, 64.0))]
    stacked = ea.ExpertWeights.stack([p[0] for p in parts])
    for ew in (stacked, stacked.truncated(8), stacked.truncated(3)):
        lay = host_layout(ew)
        got = ew.rank_bound()
        for e in range(3):
            want = fr.rank_bound(lay["buckets"], 4096, ew.percentLoad, e)
            assert np.float32(got[e]).tobytes() == np.float32(want).tobytes(), (ew.percentLoad, e, got[e], want)
    assert 32.0 < stacked.rank_bound()[2] / stacked.rank_bound()[0] < 128.0          # (different matrices: the scales differ, by about 64)
    ewq, layq = gpu_q4(ea, "structured")
    assert np.float32(ewq.rank_bound()[0]).tobytes() == np.float32(fr.rank_bound(layq["stats"], 4096, 8, 0, q4=True)).tobytes()
    # a column shard reports the full handle's bound
    ew, lay = gpu_fp16(ea, "structured", 1024, 4096)
    computed = ew.rank_bound()
    for r in range(2):
        assert ew.column_shard(r, 2).rank_bound() == computed
    # a bound set by hand (never below the computed one) moves the grid: the product meets the NEW grid's envelope, and differs
    v = family_v(4096, seed=42, heavy=True)
    _, _, before, _ = check_call(ea, oracle_cpu, ew, lay, v, 0.25, 8, tag="bound as computed")
    try:
        ew.set_rank_bound([2.0 * computed[0]])
        assert ew.rank_bound() == [2.0 * computed[0]]
        st, em, after, model = check_call(ea, oracle_cpu, ew, lay, v, 0.25, 8, rank_bound=2.0 * computed[0], tag="bound doubled")
        assert [s[3] for s in model["slices"]] == [k - 1 for k in [s[3] for s in fr.slice_exponents(v, computed[0], model["slices"][0][1])]]
        assert (after.view(np.uint32) != before.view(np.uint32)).any()
        assert_bars([(st, em)], "bound doubled")
    finally:
        ew.refresh()
    assert ew.rank_bound() == computed
    _, _, again, _ = check_call(ea, oracle_cpu, ew, lay, v, 0.25, 8, tag="bound refreshed")
    assert again.tobytes() == before.tobytes()


# ------------------------------------------------------------------------------------------------ cosine
@pytest.mark.parametrize("n", COSINE_SIZES)
def test_cosine_matches_float64(ea, n):
    """effort_cosine against float64 inside the bound of three f32 sums of n terms in any order (fixedpoint_reference.cosine_bar);
    a zero vector gives NaN, as aux.metal:311 does (0 / (sqrt(|a|^2) * sqrt(0)))."""
    for name, a, b in cosine_pairs(n):
        got = ea.cosineSimilarityTo(devf(a), devf(b))
        want = fr.cosine_f64(a, b)
        if name == "zero":
            assert np.isnan(want) and np.isnan(got), (n, got)
            continue
        bar = fr.cosine_bar(a, b)
        print(f"cosine n {n:5d} {name:10s}: {got:+.9f} vs {want:+.12f}  err {abs(got - want):.2e}  bar {bar:.2e}")
        assert abs(got - want) <= bar, (n, name, got, want, bar)
        if name == "orthogonal":
            assert got == 0.0                                  # disjoint supports: every product is an exact zero
