"""tests/fixedpoint_reference.py checked on a machine without a GPU, against an emulation of the documented fixed-point scheme.

``emulate`` is a numpy restatement of what csrc/bucket_mul.hip says it does -- exact v * 2^k, the product rounded once to f32,
floor(x + 0.5) to the grid (Q4: the row's v * mean rounded to f32, scaled, rounded to nearest), integer sums per slice wrapped to
int32, each slice's sum converted to f32 and the slices added in f32 in slice order (Q4: plus an f32 chain over the outliers) --
that lives HERE, in the tests, and shares with the reference only the layout decoding.  On every input family of
tests/test_gpu_fixedpoint.py (``FP16_FAMILIES``; Q4 once) it must stay inside the reference's envelope, keep rms z within
``rms_limit`` and |mean z| within ``mean_limit`` (both reasoned there), and use at most half of the statistical bars the GPU test
asserts (``family_bars``: twice the largest value the emulation reaches over the family's cases); and the bars must reject the
mistakes listed in ``MUTATIONS``.

Here a request for 0 slices means ONE slice (no device to ask for its heuristic), the case with the coarsest grid; the figures of
every case are printed (pytest -s).  Measured, (256, 4096), worst of each family over efforts 0.1 / 0.25 / 1.0 and 1 / 8 / 64 slices:
|mean z| 0.11 .. 0.42 (0.29 gauss, 0.42 subnormal, 0.37 flat), rms z 1.00 .. 1.11, max |err| / envelope 0.13 at most.  The emulation's
figures on the GPU test's own slices stand beside the GPU's in tests/test_gpu_fixedpoint.py's docstring.
"""
import numpy as np
import pytest

from tests import fixedpoint_reference as fr
from tests.util import family_v, family_w, structured_norm_w


# ------------------------------------------------------------------------------------------------ the emulation
def _wrap32(x: np.ndarray) -> np.ndarray:
    return ((x.astype(np.int64) + 2 ** 31) % 2 ** 32) - 2 ** 31


def _f32_chain(idx: np.ndarray, terms_a: np.ndarray, terms_b: np.ndarray, outDim: int) -> np.ndarray:
    """Per output, fma(a, b, acc) over its entries in table order, in f32 (one rounding per step)."""
    order = np.argsort(idx, kind="stable")
    idx, a, b = idx[order], terms_a[order].astype(np.float64), terms_b[order].astype(np.float64)
    first = np.searchsorted(idx, np.arange(outDim))
    count = np.bincount(idx, minlength=outDim)
    acc = np.zeros(outDim, np.float32)
    for k in range(int(count.max()) if idx.size else 0):
        live = np.nonzero(count > k)[0]
        at = first[live] + k
        acc[live] = (a[at] * b[at] + acc[live].astype(np.float64)).astype(np.float32)       # a*b exact in f64: a single rounding
    return acc


def emulate(v, buckets, rows, outDim, rankBound, sliceRows, *, stats=None, outliers=None, expertRows=None,
            trunc=False, kshift=0, whole_input_grid=False) -> np.ndarray:
    """The documented scheme in numpy; the keyword switches are the MUTATIONS."""
    v32 = np.asarray(v, np.float32)
    v64 = v32.astype(np.float64)
    b = fr._u16(buckets)
    rows = np.asarray(rows, np.int64)
    q4 = stats is not None
    mean = None if not q4 else np.ascontiguousarray(stats, dtype=np.float32).reshape(-1, 2)[:, 1]
    expertRows = expertRows or b.shape[0]
    inDim = v32.shape[0]
    local = rows % expertRows
    j = local // 8 if q4 else local % inDim
    out = np.zeros(outDim, np.float32)
    k_whole = fr.grid_exponent(float(np.abs(v64).sum()) * float(rankBound), coarser_near_pow2=False)
    cols = b.shape[1]
    x = np.arange(cols, dtype=np.int64)
    for j0, j1 in fr.slice_bounds(inDim, sliceRows):
        L = float(np.abs(v64[j0:j1]).sum()) * float(rankBound)
        k = k_whole if whole_input_grid else fr.grid_exponent(L, coarser_near_pow2=False)
        k -= kshift
        sel = np.nonzero((j >= j0) & (j < j1))[0]
        acc = np.zeros(outDim, np.int64)
        for c0 in range(0, sel.size, 8192):
            r = rows[sel[c0:c0 + 8192]]
            w = b[r]
            jj = j[sel[c0:c0 + 8192]]
            if not q4:
                dv = np.ldexp(v64[jj], k)                                                        # exact
                prod = (dv[:, None] * w.view(np.float16).astype(np.float64)).astype(np.float32).astype(np.float64)
                q = np.floor(prod) if trunc else np.floor(prod + 0.5)
                o = x[None, :] * 16 + (w & 15)
                acc += np.bincount(o.ravel(), weights=q.ravel(), minlength=outDim)[:outDim].astype(np.int64)
            else:
                d = (v64[jj] * mean[r].astype(np.float64)).astype(np.float32).astype(np.float64)  # v * mean, one f32 rounding
                d = np.ldexp(d, k)
                d = np.floor(d) if trunc else np.rint(d)
                for qn in range(4):
                    n = (w >> (4 * qn)) & 15
                    o = x[None, :] * 32 + (n & 7) + (3 - qn) * 8
                    sg = np.where(n & 8, -d[:, None], d[:, None])
                    acc += np.bincount(o.ravel(), weights=sg.ravel(), minlength=outDim)[:outDim].astype(np.int64)
        part = np.ldexp(_wrap32(acc).astype(np.float32), -k)                                      # one rounding, then exact
        out = (out + part).astype(np.float32)
    if outliers is not None and len(outliers):
        ol = np.asarray(outliers, np.float32).reshape(-1, 4)
        out = (out + _f32_chain(ol[:, 2].astype(np.int64), v32[ol[:, 1].astype(np.int64)], ol[:, 0], outDim)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ cases shared with the GPU test
EFFORTS = (0.1, 0.25, 1.0)
SLICES = (0, 8, 64)


def select(oracle_cpu, v, layout, effort, expNo=0, percentLoad=None):
    """(rows, cutoff) the oracle's integer work selects (pinned bit-exact against the kernels elsewhere)."""
    q4 = layout["q4"]
    inDim, outDim = layout["inDim"], layout["outDim"]
    cutoff, _ = oracle_cpu.find_cutoff(v, layout["probes"], expNo, effort)
    if q4:
        cols = outDim // 32
        disp, n = oracle_cpu.prepare_dispatch_q4(v, layout["stats"], expNo, cutoff, inDim, cols)
    else:
        cols = outDim // 16
        pl = percentLoad or layout["percentLoad"]
        disp, n = oracle_cpu.prepare_dispatch(v, layout["stats"], expNo, cutoff, inDim, cols, pl)
    assert layout["buckets"].reshape(-1, cols).shape[0] * cols < 2 ** 24          # the list's float row offsets are exact
    return (disp[:n, 1].astype(np.int64) // cols), cutoff


def host_slice_rows(inDim: int, slices: int) -> int:
    """Slice rows for a REQUESTED slice count, as plan.hip derives them (ceil(inDim / S)); 0 = one slice here (the CPU test has
    no device whose heuristic it could ask)."""
    return inDim if slices == 0 else -(-inDim // slices)


_LAYOUTS = {}


def fp16_layout(oracle_cpu, family, outDim, inDim, seed=1234, mult=1.0):
    key = (family, outDim, inDim, seed, mult)
    if key not in _LAYOUTS:
        W = family_w(family, outDim, inDim, seed, mult)
        b, s, p, oob = oracle_cpu.convert_fp16(W)
        assert oob == 0
        _LAYOUTS[key] = {"q4": False, "W": W, "buckets": b.view(np.uint16), "stats": s, "probes": p, "inDim": inDim, "outDim": outDim,
                         "percentLoad": 16, "expertRows": inDim * 16}
    return _LAYOUTS[key]


def q4_layout(family, outDim=4096, inDim=4096, seed=31):
    from oracle import q4_layout as ql
    key = ("q4", family, outDim, inDim, seed)
    if key not in _LAYOUTS:
        W = family_w(family, outDim, inDim, seed)
        L = ql.convert(np.ascontiguousarray(W.T))
        _LAYOUTS[key] = {"q4": True, "W": W, "buckets": L["buckets"].view(np.uint16), "stats": L["bucket.stats"], "probes": L["probes"],
                         "outliers": L["outliers"], "inDim": inDim, "outDim": outDim, "percentLoad": 8, "expertRows": inDim * 8}
    return _LAYOUTS[key]


def model_kw(layout):
    return {"stats": layout["stats"], "outliers": layout.get("outliers"), "expertRows": layout["expertRows"]} if layout["q4"] else \
           {"expertRows": layout["expertRows"]}


def layout_bound(layout, expert=0, percentLoad=None):
    if layout["q4"]:
        return fr.rank_bound(layout["stats"], layout["inDim"], 8, expert, q4=True)
    return fr.rank_bound(layout["buckets"], layout["inDim"], percentLoad or layout["percentLoad"], expert)


# family -> (weight family, keywords of family_v)
FP16_FAMILIES = {
    "gauss": ("gauss", {}),
    "structured": ("structured", {}),
    "structured_heavy": ("structured", {"heavy": True}),
    "channel": ("channel", {}),
    "channel_v0": ("channel", {"zero_channel": True}),
    "lone_v0": ("lone", {"zero_channel": True}),
    "subnormal": ("subnormal", {}),
    "large": ("large", {}),
    "flat": ("flat", {"positive": True}),
}


def family_case(oracle_cpu, family, shape=(256, 4096), mult=1.0):
    wf, kw = FP16_FAMILIES[family]
    return fp16_layout(oracle_cpu, wf, *shape, mult=mult), family_v(shape[1], seed=42, **kw)


def run_case(oracle_cpu, layout, v, effort, sliceRows, expNo=0, **mut):
    rows, _ = select(oracle_cpu, v, layout, effort, expNo)
    rb = layout_bound(layout, expNo)
    model = fr.error_model(v, layout["buckets"], rows, layout["outDim"], rb, sliceRows, **model_kw(layout))
    got = emulate(v, layout["buckets"], rows, layout["outDim"], mut.pop("rankBound", rb), sliceRows, **model_kw(layout), **mut)
    return model, got


def family_stats(oracle_cpu, family, shape=(256, 4096)):
    """Per (effort, slices): the emulation's (ratio, |mean z|, rms z), and the family's bars."""
    lay, v = family_case(oracle_cpu, family, shape)
    res = {}
    for effort in EFFORTS:
        for slices in SLICES:
            model, got = run_case(oracle_cpu, lay, v, effort, host_slice_rows(shape[1], slices))
            res[(effort, slices)] = (fr.z_stats(got, model), model, got)
    return res


def family_bars(stats) -> tuple[float, float]:
    """(bar on |mean z|, bar on rms z): twice the largest value the emulation reaches over the family's cases."""
    return 2.0 * max(abs(s[1]) for s in stats), 2.0 * max(s[2] for s in stats)


def rms_limit(n_out: int) -> float:
    """rms of n_out values of at most unit variance: 1, plus four standard errors of an rms (1 / sqrt(2 n))."""
    return 1.0 + 4.0 / np.sqrt(2.0 * n_out)


def mean_limit(model) -> float:
    """|mean z| the scheme itself allows: six standard errors of a mean of values of at most unit variance, plus the bias of
    floor(x + 0.5).  x is an f32: at magnitude 2^e its fraction has 23 - e bits, it is an exact half with probability 2^-(23-e),
    and every such tie goes UP by half a step -- an expected +2^(e-24) steps per product, which is 2^-24 |p|, the same figure as
    the product's f32 rounding bound (``rnd`` of the model).  So the mean may sit above zero by the mean of rnd / sigma."""
    ok = model["sigma"] > 0
    return 6.0 / np.sqrt(max(1, int(ok.sum()))) + float((model["rnd"][ok] / model["sigma"][ok]).mean())


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("family", list(FP16_FAMILIES))
def test_emulation_meets_the_model(oracle_cpu, family):
    res = family_stats(oracle_cpu, family)
    zs = [r[0] for r in res.values()]
    bar_mean, bar_rms = family_bars(zs)
    n_out = 256
    for (effort, slices), ((ratio, mz, rz), model, got) in res.items():
        scale = float(np.abs(model["f64"]).max())
        print(f"{family:17s} effort {effort:4.2f} slices {slices:2d}: err/env {ratio:.3f}  mean z {mz:+.4f}  rms z {rz:.4f}  "
              f"max err/max|out| {float(np.abs(got - model['f64']).max()) / scale:.2e}")
        assert ratio <= 1.0, (family, effort, slices, ratio)
        assert rz <= rms_limit(n_out) and abs(mz) <= mean_limit(model), (family, effort, slices, mz, rz)
        assert abs(mz) <= bar_mean / 2 and rz <= bar_rms / 2
    print(f"{family:17s} bars: |mean z| <= {bar_mean:.4f}, rms z <= {bar_rms:.4f}")


def test_emulation_meets_the_model_ragged_and_q4(oracle_cpu):
    """(1024, 4500): a ragged last slice; Q4 4096 x 4096 with its outlier table."""
    lay = fp16_layout(oracle_cpu, "structured", 1024, 4500)
    v = family_v(4500, heavy=True)
    for slices in (8, 64):
        model, got = run_case(oracle_cpu, lay, v, 0.25, host_slice_rows(4500, slices))
        assert model["slices"][-1][1] - model["slices"][-1][0] < host_slice_rows(4500, slices)      # ragged
        ratio, mz, rz = fr.z_stats(got, model)
        print(f"fp16 1024x4500 slices {slices}: err/env {ratio:.3f} mean z {mz:+.4f} rms z {rz:.4f}")
        assert ratio <= 1.0 and rz <= rms_limit(1024) and abs(mz) <= mean_limit(model)
    layq = q4_layout("structured")
    vq = family_v(4096, heavy=True)
    for slices in (0, 8):
        model, got = run_case(oracle_cpu, layq, vq, 0.25, host_slice_rows(4096, slices))
        ratio, mz, rz = fr.z_stats(got, model)
        print(f"q4 4096x4096 slices {slices}: err/env {ratio:.3f} mean z {mz:+.4f} rms z {rz:.4f}")
        assert ratio <= 1.0 and rz <= rms_limit(4096) and abs(mz) <= mean_limit(model)


MUTATIONS = ["trunc", "expert0_bound", "stale_bound", "dropped_row", "whole_input_grid", "coarser_by_8"]


@pytest.mark.parametrize("family,mutation", [(f, m) for f in ("gauss", "structured_heavy", "channel_v0") for m in MUTATIONS] +
                         [("flat", "expert0_bound"), ("flat", "stale_bound")])
def test_bars_reject_mutations(oracle_cpu, family, mutation):
    """Each documented way of getting the scale wrong must leave the envelope or a statistical bar.

    ``trunc`` is floor(x) where floor(x + 0.5) is due: every product low by half a step on average.  (Truncation TOWARDS ZERO is
    sign-symmetric: it leaves the mean alone and exactly doubles the rounding's standard deviation, which is where the rms bar
    sits; no bar of this kind sees it reliably, and it is not asserted.)

    The two wrong BOUNDS need a word.  A bound too large by 64 makes the grid 64 times coarser: every family shows it (expert 0 of
    a stack being the x64 matrix, its bound used for the x1 expert; weights that shrank under a stale bound are the same case).  A
    bound too SMALL by 64 -- expert 0's used for a x64 expert, or left stale after the weights grew x64 -- makes the grid FINER and
    the result more accurate, until a slice's integer sum leaves int32: that needs an output within 1/32 of the bound L, which of
    these families only ``flat`` reaches (every output is L/16).  So that direction is asserted on ``flat``, where the wrapped
    accumulator leaves the envelope by orders of magnitude; on the other families it is asserted that the bars CANNOT see it."""
    shape = (256, 4096)
    lay, v = family_case(oracle_cpu, family, shape)
    bar_mean, bar_rms = family_bars([r[0] for r in family_stats(oracle_cpu, family).values()])
    effort, slices = 0.25, 8
    B = host_slice_rows(shape[1], slices)
    harmless = False
    if mutation == "trunc":
        model, got = run_case(oracle_cpu, lay, v, effort, B, trunc=True)
    elif mutation == "expert0_bound" and family != "flat":      # stack (x64, x1): the x1 expert multiplied on expert 0's grid
        big, _ = family_case(oracle_cpu, family, shape, mult=64.0)
        model, got = run_case(oracle_cpu, lay, v, effort, B, rankBound=layout_bound(big))
    elif mutation in ("expert0_bound", "stale_bound"):          # the x64 matrix on the x1 matrix's bound
        big, _ = family_case(oracle_cpu, family, shape, mult=64.0)
        model, got = run_case(oracle_cpu, big, v, 1.0, B, rankBound=layout_bound(lay))
        harmless = family != "flat"
    elif mutation == "dropped_row":
        rows, _ = select(oracle_cpu, v, lay, effort)
        means = np.abs(lay["stats"].view(np.float16).reshape(-1, 4)[rows, 3].astype(np.float32))
        drop = int(np.argsort(means, kind="stable")[means.size // 2])                                 # a kept row of median mean
        rb = layout_bound(lay)
        model = fr.error_model(v, lay["buckets"], rows, shape[0], rb, B, **model_kw(lay))
        got = emulate(v, lay["buckets"], np.delete(rows, drop), shape[0], rb, B, **model_kw(lay))
    elif mutation == "whole_input_grid":
        model, got = run_case(oracle_cpu, lay, v, effort, B, whole_input_grid=True)
    else:                                         # one slice, where the whole input's grid is due: a grid coarser by 2^3
        model, got = run_case(oracle_cpu, lay, v, effort, shape[1], kshift=3)
    ratio, mz, rz = fr.z_stats(got, model)
    print(f"{family} {mutation}: err/env {ratio:.3g} mean z {mz:+.4g} rms z {rz:.4g} (bars {bar_mean:.4f} {bar_rms:.4f})")
    rejected = ratio > 1.0 or abs(mz) > bar_mean or rz > bar_rms
    assert rejected != harmless, (family, mutation, ratio, mz, rz)
    if mutation in ("expert0_bound", "stale_bound") and not harmless:
        assert ratio > 1.0                        # (a wrong bound leaves the hard envelope, not only a statistical bar)


def test_rank_bound_against_a_second_formulation(oracle_cpu):
    """rank_bound against loops over the dense matrix's own definition: FP16, the bucket rows of rank r are the r-th largest |w| of
    every bucket, so the rank's maximum is found without the layout's row order; Q4 from the stats."""
    for family in ("gauss", "structured", "channel", "subnormal"):
        lay = fp16_layout(oracle_cpu, family, 256, 4096)
        b = lay["buckets"].reshape(16, 4096, 16)                                   # [rank][input][column]
        for pl in (16, 8, 3):
            total = np.float32(0)
            for r in range(pl):
                m = np.float32(0)
                for col in range(16):
                    m = max(m, np.float32(np.abs(b[r, :, col].view(np.float16)).max()))
                total = np.float32(total + m)
            got = fr.rank_bound(lay["buckets"][:4096 * pl], 4096, pl)
            assert np.float32(got).tobytes() == total.tobytes(), (family, pl)
    two = np.concatenate([fp16_layout(oracle_cpu, "gauss", 256, 4096)["buckets"], fp16_layout(oracle_cpu, "structured", 256, 4096)["buckets"]])
    assert fr.rank_bound(two, 4096, 16, 1) == fr.rank_bound(fp16_layout(oracle_cpu, "structured", 256, 4096)["buckets"], 4096, 16)
    rng = np.random.default_rng(3)
    st = np.abs(rng.normal(0, 0.02, size=(2 * 512 * 8, 2))).astype(np.float32)
    for e in range(2):
        total = np.float32(0)
        for r in range(8):
            total = np.float32(total + max(st[(e * 512 + j) * 8 + r, 1] for j in range(512)))
        assert fr.rank_bound(st, 512, 8, e, q4=True).tobytes() == total.tobytes()


def test_product_f64_against_the_dense_matrix(oracle_cpu):
    """At effort 1 with every rank loaded the selected rows are the whole matrix: product_f64 is W (position bits included) times v."""
    lay = fp16_layout(oracle_cpu, "structured", 256, 4096)
    v = family_v(4096, heavy=True)
    rows = np.arange(4096 * 16)
    got = fr.product_f64(v, lay["buckets"], rows, 256)
    b = lay["buckets"].reshape(16, 4096, 16)
    want = np.zeros(256)
    for r in range(16):
        for col in range(16):
            w = b[r, :, col]
            np.add.at(want, col * 16 + (w & 15), v.astype(np.float64) * w.view(np.float16).astype(np.float64))
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # the position bits perturb a weight by less than 2^-6 of itself: the dense product is close, not equal
    dense = lay["W"].astype(np.float64) @ v.astype(np.float64)
    assert np.abs(got - dense).max() <= 2.0 ** -6 * (np.abs(lay["W"].astype(np.float64)) @ np.abs(v.astype(np.float64))).max()


def test_grid_exponent_and_clamps():
    assert fr.grid_exponent(0.0) == 0
    assert fr.grid_exponent(1.0) == 29 and fr.grid_exponent(1.999) == 29 and fr.grid_exponent(2.0) == 28
    assert fr.grid_exponent(2.0 * (1 - 5e-6)) == 28 and fr.grid_exponent(2.0 * (1 - 5e-6), coarser_near_pow2=False) == 29
    assert fr.grid_exponent(2.0 ** -70) == 99 and fr.grid_exponent(2.0 ** -71) == 100 and fr.grid_exponent(2.0 ** -90) == 100
    assert fr.grid_exponent(2.0 ** 127) == -98                 # the largest finite f32 exponent: the lower clamp, -100, is out of reach
    for L in (3.7e-12, 0.9, 513.0, 7e20):
        k = fr.grid_exponent(L)
        assert 2.0 ** 29 <= 2.0 ** k * L < 2.0 ** 30


# ------------------------------------------------------------------------------------------------ cosine
COSINE_SIZES = (1, 63, 64, 65, 1023, 1025, 4096, 14336)


def cosine_pairs(n: int, seed: int = 9):
    """(name, a, b): equal, opposite, orthogonal (by construction, exactly: disjoint supports, or for n = 1 a zero), heavy-tailed,
    and one zero vector."""
    rng = np.random.default_rng(seed + n)
    a = rng.standard_normal(n).astype(np.float32)
    h1 = (rng.standard_normal(n) * np.exp(2.0 * rng.standard_normal(n))).astype(np.float32)
    h2 = (h1 * (1 + 0.1 * rng.standard_normal(n)) + 0.1 * rng.standard_normal(n)).astype(np.float32)
    pairs = [("equal", a, a.copy()), ("opposite", a, -a), ("heavy", h1, h2), ("zero", a, np.zeros(n, np.float32))]
    if n > 1:
        lo, hi = a.copy(), a.copy()
        lo[n // 2:] = 0
        hi[:n // 2] = 0
        pairs.append(("orthogonal", lo, hi))
    return pairs


def cosine_f32_plain(a, b) -> np.float32:
    d = ma = mb = np.float32(0)
    for x, y in zip(a, b):
        d = np.float32(d + np.float32(x * y))
        ma = np.float32(ma + np.float32(x * x))
        mb = np.float32(mb + np.float32(y * y))
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float32(d / np.float32(np.sqrt(ma) * np.sqrt(mb)))


@pytest.mark.parametrize("n", COSINE_SIZES)
def test_cosine_bar_holds_a_plain_f32_evaluation(n):
    for name, a, b in cosine_pairs(n):
        want, got = fr.cosine_f64(a, b), float(cosine_f32_plain(a, b))
        if name == "zero":
            assert np.isnan(want) and np.isnan(got)             # aux.metal:311: 0 / (sqrt(|a|^2) * sqrt(0)) = 0 / 0
            continue
        bar = fr.cosine_bar(a, b)
        assert abs(got - want) <= bar / 2, (n, name, got, want, bar)
        assert bar <= 2.1 * (n + 4) * fr.U                      # the bar is no looser than gamma_n on each side of the quotient


def test_structured_generators_have_the_stated_structure():
    """The numpy restatements of decode.structured_matrix / structured_norm_weights: overall std, heavy tails, channel spread, unit rms."""
    W = family_w("structured", 256, 4096).astype(np.float64)
    assert abs(W.std() / 0.02 - 1.0) < 0.01
    ch = np.sqrt((W * W).mean(axis=0))
    assert ch.max() / np.median(ch) > 5.0                        # log-normal channel scales, sigma 0.7
    assert np.abs(W).max() / W.std() > 20.0                      # heavy tails
    w = structured_norm_w(4096).astype(np.float64)
    assert abs(np.sqrt((w * w).mean()) - 1.0) < 0.01 and w.min() > 0 and w.max() > 4.0
