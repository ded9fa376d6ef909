"""The inputs that walk block_find_cutoff (effort_amd/csrc/cutoff_device.h) through its branches, as data.
TEST INFRASTRUCTURE: numpy only (no torch, no project code beyond tests/cutoff_model.py), so that the CPU test
(tests/test_cutoff_cases_cpu.py: the model against the oracle, and WHICH branches the table reaches) and the GPU test
(tests/test_gpu_cutoff_paths.py: every instantiation of the search against the oracle) read ONE table.

A case is (name, family, v f32[4096], probes f16[4096], extra): ``extra`` are efforts of its own on top of ``EFFORTS``.  Inputs are
finite: NaN and Inf are out of contract (the reference's min / max on them is unspecified).  Every constructed case asserts the cells
-- ``cells(v, probes)``: the bf16 patterns of the 4096 probe products, the model's ``vp`` -- it aims for, so a builder that misses its
boundary fails here, on the CPU.

Families (``CAPS``: the table sizes kCutoffBinsPerThread x 128 / 256 / 512 / 1024 threads give):
  degenerate   all-zero input (a -0.0 among the zeros), one nonzero product, all products equal, all probes zero, every product above
               the reference's 1000 clamp, subnormal f32 inputs and products, products up to ~1e38
  span         per table size: smallest nonzero to largest cell cap - 2, cap - 1 (the table exactly full) and cap (one cell too many: a
               ballot pass) apart, with and without exact zeros among the values
  window       per table size: the smallest nonzero value on kCutoffWindowBase and one cell below it; the largest on the window's last
               cell and one cell beyond it (zeros among the values: they count into the pad dwords)
  wide         ~100 octaves of range (ballot passes; five and more at high efforts even with 8192 cells), two levels ~100 octaves apart
               with the effort on the upper level's count (the loop ends inside its first ballot pass), and a long descent from ~1e38
               to a tie (bounds in adjacent cells only after more than 60 rounds)
  kinds        gauss, heavy, zeros, few, tiny, ties: two seeds each, for the exits
"""
from collections import namedtuple

import numpy as np

from tests.cutoff_model import CAPS, WINDOW_BASE, cells, frompat

Case = namedtuple("Case", "name family v probes extra")

EFFORTS = (0.0, 0.02, 0.1, 0.25, 0.5, 0.9, 1.0)
BOUNDARY_QS = (1, 2, 4093, 4094)       # m = 4096 - q within 2 of either end of the count range: the k <= 0 and k > 4096 guards decide
FAMILIES = ("degenerate", "span", "window", "wide", "kinds")
# |v| within the twelve decades tests/test_gpu_parity.py::test_cutoff_across_input_scales multiplies at (a heavy-tailed unit input times
# 1e-9 .. 3.1e3): cases whose largest input lies inside have their product checked on the GPU, the others their selection only
PRODUCT_SCALES = (1e-9, 3.1e3 * 64.0)


def effort_to_q(effort: float) -> int:
    """q = Int(Double(4095) * (1 - effort)) (bucketMul.swift:39), as the oracle and the host layer compute it."""
    return int(4095.0 * (1.0 - float(effort)))


def effort_for_q(q: int) -> float:
    """An effort whose quantile is exactly ``q``: 1 - q / 4095 where that rounds to q, else the step above it
    (tests/edge_shapes.py::boundary_efforts builds the same two)."""
    for e in (1.0 - q / 4095.0, 1.0 - (q + 1e-6) / 4095.0):
        if effort_to_q(e) == q:
            return e
    raise AssertionError(q)


BOUNDARY_EFFORTS = tuple(effort_for_q(q) for q in BOUNDARY_QS)


def efforts(case) -> tuple:
    return EFFORTS + BOUNDARY_EFFORTS + tuple(case.extra)


def product_checked(case) -> bool:
    top = float(np.abs(case.v).max())
    return PRODUCT_SCALES[0] <= top <= PRODUCT_SCALES[1]


# ---- today's kinds (tests/test_cutoff_trajectory_model.py runs them at 40 seeds) ------------------------------------------------
def kind_inputs(seed, kind):
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(4096).astype(np.float32)
    pr = (rng.standard_normal(4096) * 0.02).astype(np.float16)
    if kind == "heavy":
        v = (v * np.exp(2.0 * rng.standard_normal(4096))).astype(np.float32)
    elif kind == "zeros":
        v[rng.integers(0, 4096, 1500)] = 0
        pr[rng.integers(0, 4096, 300)] = 0
    elif kind == "wide":                                   # > 64 octaves of range: ballot rounds before the table
        v = (v * np.exp2(rng.integers(-60, 40, 4096).astype(np.float32))).astype(np.float32)
    elif kind == "few":                                    # few distinct values: the count == effort / counts exits
        v = rng.choice(np.array([0.5, 1.0, 2.0, 3.0], np.float32), 4096)
        pr = rng.choice(np.array([0.01, 0.02], np.float16), 4096)
    elif kind == "tiny":
        v = (v * 1e-9).astype(np.float32)
    elif kind == "ties":                                   # three mantissa bits, one probe: a few cells per octave, hundreds of values each --
        u = v.view(np.uint32) & np.uint32(0xFFF00000)      #  the counts step over every rank, the bounds end in adjacent cells
        v = (u.view(np.float32) * np.float32(1.0 if seed % 2 == 0 else 0.01)).astype(np.float32)      # (odd seeds: a cutoff below 128)
        pr = np.full(4096, 0.02, np.float16)
    else:
        assert kind == "gauss", kind
    return v, pr.view(np.uint16)


# ---- vectors with chosen cells -----------------------------------------------------------------------------------------------
PROBE = np.float16(2.0 ** -6)            # exact in f16 and in bf16: the product's bits are the scaled input's


def vector_of_cells(want, rng):
    """(v, probes u16) whose probe products fall into exactly the cells ``want`` (0: an exact zero input), signs mixed."""
    want = np.asarray(want, np.int64)
    assert want.shape == (4096,) and (want >= 0).all() and (want < 0x7F80).all()
    x = (want.astype(np.uint32) << 16).view(np.float32).astype(np.float64)          # the bf16 value at the centre of each cell
    v = (x / (1e5 * float(PROBE))).astype(np.float32)
    v *= rng.choice(np.array([-1.0, 1.0], np.float32), 4096)
    pr = np.full(4096, PROBE, np.float16).view(np.uint16)
    assert np.isfinite(v).all() and (cells(v, pr) == want).all()
    return v, pr


def spread(lo, hi, rng, zeros=0):
    """4096 cells uniform over [lo, hi] with both ends present and ``zeros`` exact zeros among them."""
    c = rng.integers(lo, hi + 1, 4096)
    idx = rng.permutation(4096)
    c[idx[0]], c[idx[1]] = lo, hi
    c[idx[2:2 + zeros]] = 0
    return c


def _degenerate():
    rng = np.random.default_rng(101)
    probes = (rng.standard_normal(4096) * 0.02).astype(np.float16)
    gauss = rng.standard_normal(4096).astype(np.float32)
    out = []
    v = np.zeros(4096, np.float32)
    v[5] = -0.0
    assert np.signbit(v[5]) and not cells(v, probes.view(np.uint16)).any()
    out.append(("all-zero", v, probes))
    v = np.zeros(4096, np.float32)
    v[1234] = 0.7
    assert (cells(v, probes.view(np.uint16)) > 0).sum() == 1
    out.append(("one-nonzero", v, probes))
    v = np.where(np.arange(4096) % 2, -0.5, 0.5).astype(np.float32)
    p = np.full(4096, 0.02, np.float16)
    assert np.unique(cells(v, p.view(np.uint16))).size == 1 and cells(v, p.view(np.uint16))[0] > 0
    out.append(("all-equal", v, p))
    p = np.zeros(4096, np.float16)
    p[::3] = -0.0                                                     # (a Q4 diagonal removed as outliers)
    assert not cells(gauss, p.view(np.uint16)).any()
    out.append(("probes-zero", gauss, p))
    v = (rng.uniform(1.0, 50.0, 4096) * rng.choice([-1.0, 1.0], 4096)).astype(np.float32)
    p = rng.uniform(0.02, 0.04, 4096).astype(np.float16)
    assert (frompat(cells(v, p.view(np.uint16)).min()) > 1000.0)      # min(.., 1000) clamps minBound
    out.append(("above-1000", v, p))
    # |v| ~ 1e-41: subnormal f32 inputs; 1e5 * v is normal again, and half the probes take the product back below 2^-126
    v = (rng.standard_normal(4096) * 1e-41).astype(np.float32)
    p = np.where(np.arange(4096) % 2, 0.02, 1e-3).astype(np.float16)
    c = cells(v, p.view(np.uint16))
    assert (np.abs(v) < np.finfo(np.float32).tiny).all() and ((c > 0) & (c < 128)).sum() > 1000 and (c >= 128).sum() > 1000
    out.append(("subnormal", v, p))
    # products up to ~1e38: sixteen inputs of ~1e33 under probes of 1.0 over a Gaussian rest
    v = gauss.copy()
    p = probes.copy()
    big = rng.permutation(4096)[:16]
    v[big] = (rng.uniform(0.3, 1.0, 16) * 1e33 * rng.choice([-1.0, 1.0], 16)).astype(np.float32)
    p[big] = np.float16(1.0)
    t = np.float32(1e5) * v
    c = cells(v, p.view(np.uint16))
    assert np.isfinite(t).all() and np.isfinite(t * p.astype(np.float32)).all() and c.max() < 0x7F80 and frompat(c.max()) > 5e37
    out.append(("near-max", v, p))
    return [Case(n, "degenerate", np.ascontiguousarray(v, np.float32), np.ascontiguousarray(p).view(np.uint16), ()) for n, v, p in out]


def _span():
    out = []
    for cap in CAPS:
        for d in (cap - 2, cap - 1, cap):
            for zeros in (0, 600):
                rng = np.random.default_rng([202, cap, d, zeros])
                lo = WINDOW_BASE - 300 if zeros else WINDOW_BASE + 40
                v, pr = vector_of_cells(spread(lo, lo + d, rng, zeros), rng)
                c = cells(v, pr)
                assert c.max() - c[c > 0].min() == d and (c == 0).sum() == zeros
                out.append(Case(f"span-{cap}-{'full' if d == cap - 1 else 'under' if d < cap else 'over'}{'-zeros' if zeros else ''}", "span", v, pr, ()))
    return out


def _window():
    out = []
    for cap in CAPS:
        last = WINDOW_BASE + cap - 1
        for name, lo, hi in (("min-on-base", WINDOW_BASE, WINDOW_BASE + cap // 2), ("min-below-base", WINDOW_BASE - 1, WINDOW_BASE + cap // 2),
                             ("max-on-last", WINDOW_BASE + cap // 2, last), ("max-beyond-last", WINDOW_BASE + cap // 2, last + 1)):
            rng = np.random.default_rng([303, cap, lo, hi])
            v, pr = vector_of_cells(spread(lo, hi, rng, 300), rng)
            c = cells(v, pr)
            assert c[c > 0].min() == lo and c.max() == hi and (c == 0).sum() == 300
            out.append(Case(f"window-{cap}-{name}", "window", v, pr, ()))
    return out


TWO_LEVEL_UPPER = 1000                   # values on the upper of the two levels
LATE_TAIL_TOP = (127 + 120) << 7         # the cell of 2^120 ~ 1.3e36 (the scaled input, 64 times that, stays finite)


def _wide():
    out = [Case(f"wide-{seed}", "wide", *kind_inputs(seed, "wide"), ()) for seed in (0, 1)]
    rng = np.random.default_rng(404)
    hi = (127 + 30) << 7
    c = np.full(4096, hi - 100 * 128)
    c[rng.permutation(4096)[:TWO_LEVEL_UPPER]] = hi
    v, pr = vector_of_cells(c, rng)
    assert (cells(v, pr) == hi).sum() == TWO_LEVEL_UPPER
    out.append(Case("two-level", "wide", v, pr, (effort_for_q(4096 - TWO_LEVEL_UPPER),)))
    # a few values at 2^120 over two crowded neighbouring cells 64 octaves below: the upper bound halves its way down for ~64 rounds
    # before the bracket closes on the tie between the two
    tie = (127 + 56) << 7
    c = np.full(4096, tie)
    idx = rng.permutation(4096)
    c[idx[:8]] = LATE_TAIL_TOP
    c[idx[8:2008]] = tie + 1
    v, pr = vector_of_cells(c, rng)
    out.append(Case("late-tail", "wide", v, pr, ()))
    return out


def _kinds():
    return [Case(f"{kind}-{seed}", "kinds", *kind_inputs(seed, kind), ()) for kind in ("gauss", "heavy", "zeros", "few", "tiny", "ties") for seed in (0, 1)]


_TABLE = []


def table():
    """Every case, built once (the arrays are shared: leave them unchanged)."""
    if not _TABLE:
        _TABLE.extend(_degenerate() + _span() + _window() + _wide() + _kinds())
        assert len({c.name for c in _TABLE}) == len(_TABLE)
        for c in _TABLE:
            assert c.v.dtype == np.float32 and c.v.shape == (4096,) and c.probes.dtype == np.uint16 and c.probes.shape == (4096,)
            assert np.isfinite(c.v).all() and np.isfinite(c.probes.view(np.float16).astype(np.float32)).all(), c.name
            c.v.setflags(write=False)
            c.probes.setflags(write=False)
    return list(_TABLE)
