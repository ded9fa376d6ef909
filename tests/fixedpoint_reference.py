"""Float64 reference and error model of bucketMul's fixed-point sums.  TEST INFRASTRUCTURE: numpy only, no project code.

What the multiply documents (csrc/bucket_mul.hip, "Fixed-point scale of this workgroup's tile"; include/effort_hip.h):

  * the inputs are cut into row slices of B inputs, slice s = [s*B, min((s+1)*B, inDim)); one workgroup sums one slice's
    products of one column tile;
  * with L_s = (sum over the slice of |v_j|) * rankBound[e] the workgroup takes the power of two 2^k_s with 2^k_s * L_s < 2^30
    (k_s = 29 - floor(log2 L_s), kept inside [-100, 100]; 0 where L_s = 0);
  * FP16: v_j * 2^k_s is exact, its product with float(w) -- the position bits left in w -- is rounded ONCE to f32 and
    then to the integer grid by floor(x + 0.5); Q4: the row's one magnitude v_j * mean is rounded once to f32, scaled
    (exact) and rounded to the nearest integer, and added or subtracted per nibble;
  * the integers are summed exactly (int32; the bound keeps every partial sum inside it);
  * a slice's sum goes back to f32 (one rounding: |sum| < 2^30 has more than 24 bits), times 2^-k_s (exact), Q4 adds the
    slice's share of the outlier products, themselves an f32 sum; the S slices' f32 values are added in f32.

``product_f64`` is the exact product; ``envelope`` the worst case of that scheme per output, ``sigma`` the standard deviation of
its error were the grid roundings independent and uniform.  The selection of rows is NOT derived here: it is integer work the
suite pins bit-exact elsewhere, the tests take it from the oracle's find_cutoff / prepare_dispatch.

Layouts (bucketMul.metal:100-106, bucketMulQ4.metal:76-81, convert.swift):
  FP16  bucket row  e*expertRows + rank*inDim + j,  word x:  out[x*16 + (w & 15)] += v_j * float(w)
  Q4    bucket row  e*expertRows + j*8 + sub,       word x, nibble n at bits 4q (q = 0 lowest):
                    out[x*32 + (n & 7) + (3 - q)*8] += (n & 8) ? -v_j*mean : v_j*mean,   mean = stats[row][1]
        outliers    f32 [n, 4]: out[o[2]] += v[o[1]] * o[0]   (bucketMulQ4.metal:13-21)
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24            # unit roundoff of f32 (round to nearest)
TINY = 2.0 ** -150        # half the smallest f32 subnormal: the absolute error of an f32 rounding that underflows
K_MIN, K_MAX = -100, 100  # the kernel's clamp of k


# ------------------------------------------------------------------------------------------------ products
def _u16(a) -> np.ndarray:
    a = np.ascontiguousarray(a)
    if a.dtype in (np.float16, np.int16):
        a = a.view(np.uint16)
    assert a.dtype == np.uint16, a.dtype
    return a.reshape(-1, a.shape[-1])


def _row_inputs(rows: np.ndarray, inDim: int, expertRows: int, q4: bool) -> np.ndarray:
    local = np.asarray(rows, np.int64) % expertRows
    return local // 8 if q4 else local % inDim


def _products(v64: np.ndarray, buckets: np.ndarray, rows: np.ndarray, j: np.ndarray, means):
    """(output index, exact product) of every element of the bucket rows ``rows`` (inputs ``j``): two [n, k] arrays."""
    w = buckets[rows]                                                   # [n, cols] u16
    cols = w.shape[1]
    x = np.arange(cols, dtype=np.int64)
    if means is None:                                                    # FP16: the position bits stay in the multiplied value
        o = x[None, :] * 16 + (w & 15)
        p = v64[j][:, None] * w.view(np.float16).astype(np.float64)
        return o, p
    d = v64[j] * means[rows]                                             # exact in f64: two f32 factors
    o = np.empty((w.shape[0], cols, 4), np.int64)
    p = np.empty((w.shape[0], cols, 4), np.float64)
    for q in range(4):
        n = (w >> (4 * q)) & 15
        o[:, :, q] = x[None, :] * 32 + (n & 7) + (3 - q) * 8
        p[:, :, q] = np.where(n & 8, -d[:, None], d[:, None])
    return o.reshape(w.shape[0], -1), p.reshape(w.shape[0], -1)


def _means(stats) -> np.ndarray | None:
    return None if stats is None else np.ascontiguousarray(stats, dtype=np.float32).reshape(-1, 2)[:, 1].astype(np.float64)


def _outlier_terms(v64, outliers, outDim):
    """(output index, exact product) per outlier."""
    if outliers is None or not len(outliers):
        return np.zeros(0, np.int64), np.zeros(0, np.float64)
    ol = np.asarray(outliers, np.float32).reshape(-1, 4)
    return ol[:, 2].astype(np.int64), v64[ol[:, 1].astype(np.int64)] * ol[:, 0].astype(np.float64)


def product_f64(v, buckets, rows, outDim: int, *, stats=None, outliers=None, expertRows: int | None = None) -> np.ndarray:
    """The exact sum over the selected bucket rows ``rows`` (indices into ``buckets``, the expert's offset included) of
    v_j * float(w), in float64.  ``stats`` (f32 [rows, 2]) makes it the Q4 product, ``outliers`` adds the Q4 outlier table.
    Every term is exact in float64 (24 x 11 or 24 x 24 bits); their sum is a float64 sum of at most 2^17 terms per output,
    2^-36 of the sum of magnitudes at worst: nine orders below what it is compared against."""
    v64 = np.asarray(v, np.float32).astype(np.float64)
    b = _u16(buckets)
    rows = np.asarray(rows, np.int64)
    means = _means(stats)
    expertRows = expertRows or b.shape[0]
    j = _row_inputs(rows, v64.shape[0], expertRows, means is not None)
    out = np.zeros(outDim, np.float64)
    for c0 in range(0, rows.shape[0], 8192):
        o, p = _products(v64, b, rows[c0:c0 + 8192], j[c0:c0 + 8192], means)
        out += np.bincount(o.ravel(), weights=p.ravel(), minlength=outDim)[:outDim]
    oo, po = _outlier_terms(v64, outliers, outDim)
    if oo.size:
        out += np.bincount(oo, weights=po, minlength=outDim)[:outDim]
    return out


# ------------------------------------------------------------------------------------------------ the bound of registration
def rank_bound(layout, inDim: int, percentLoad: int, expert: int = 0, q4: bool = False) -> np.float32:
    """rankBound[expert] as registration defines it: the sum over ranks of that rank's largest |w| over the inputs (FP16:
    ``layout`` = buckets, the position bits included; Q4: ``layout`` = stats f32 [rows, 2], the largest |row mean|, eight
    ranks), the maxima exact, the sum in f32 in rank order."""
    total = np.float32(0.0)
    if q4:
        mean = np.abs(np.ascontiguousarray(layout, dtype=np.float32).reshape(-1, 2)[:, 1])
        mean = mean[expert * inDim * 8:(expert + 1) * inDim * 8].reshape(inDim, 8)              # row = j*8 + rank
        for r in range(8):
            total = np.float32(total + mean[:, r].max())
        return total
    b = _u16(layout)
    rows = inDim * percentLoad
    mag = np.abs(b[expert * rows:(expert + 1) * rows].view(np.float16).astype(np.float32)).max(axis=1)   # per bucket row
    for r in range(percentLoad):
        total = np.float32(total + mag[r * inDim:(r + 1) * inDim].max())                        # row = rank*inDim + j
    return total


# ------------------------------------------------------------------------------------------------ the grid
def slice_bounds(inDim: int, sliceRows: int):
    return [(j0, min(j0 + sliceRows, inDim)) for j0 in range(0, inDim, sliceRows)]


def grid_exponent(L: float, coarser_near_pow2: bool = True) -> int:
    """k of a slice whose bound is L: 29 - floor(log2 L) inside [-100, 100], 0 for L = 0.  The kernel sums |v_j| in f32 in its
    own order, so within 1e-5 (relative) below a power of two its L may land on either side: there the COARSER grid is taken
    (the one with the larger roundings)."""
    if not L > 0.0:
        return 0
    m, e = np.frexp(L)                                                   # L = m * 2^e, 0.5 <= m < 1: floor(log2 L) = e - 1
    E = int(e) - 1
    if coarser_near_pow2 and L * (1.0 + 1e-5) >= 2.0 ** (E + 1):
        E += 1
    return int(max(K_MIN, min(K_MAX, 29 - E)))


def slice_exponents(v, rankBound: float, sliceRows: int):
    """[(j0, j1, L_s, k_s)] per slice, L_s in float64."""
    a = np.abs(np.asarray(v, np.float32).astype(np.float64))
    res = []
    for j0, j1 in slice_bounds(a.shape[0], sliceRows):
        L = float(a[j0:j1].sum()) * float(rankBound)
        res.append((j0, j1, L, grid_exponent(L)))
    return res


# ------------------------------------------------------------------------------------------------ the error model
def error_model(v, buckets, rows, outDim: int, rankBound: float, sliceRows: int, *, stats=None, outliers=None,
                expertRows: int | None = None) -> dict:
    """Everything ``envelope`` and ``sigma`` need, per output: see their docstrings.  Also returns the exact product (``f64``), the
    slices' (j0, j1, L, k) and the kept rows per slice (``counts``: what effort_debug_slice_counts reports)."""
    v64 = np.asarray(v, np.float32).astype(np.float64)
    b = _u16(buckets)
    rows = np.asarray(rows, np.int64)
    means = _means(stats)
    q4 = means is not None
    expertRows = expertRows or b.shape[0]
    j = _row_inputs(rows, v64.shape[0], expertRows, q4)
    sl = slice_exponents(v64, rankBound, sliceRows)
    S = len(sl)
    f64 = np.zeros(outDim)
    grid = np.zeros(outDim)            # sum_s m_so * (2^-k_s / 2 + TINY)
    rnd = np.zeros(outDim)             # sum over products of 2^-24 |p|
    mag = np.zeros(outDim)             # sum_s |P_so|
    var = np.zeros(outDim)             # sum_s m_so * 2^(-2 k_s) / 12
    counts = []
    which = j // sliceRows
    for s, (j0, j1, L, k) in enumerate(sl):
        sel = np.nonzero(which == s)[0]
        counts.append(int(sel.size))
        if not sel.size:
            continue
        P = np.zeros(outDim)
        A = np.zeros(outDim)
        M = np.zeros(outDim)
        for c0 in range(0, sel.size, 8192):
            idx = sel[c0:c0 + 8192]
            o, p = _products(v64, b, rows[idx], j[idx], means)
            o = o.ravel()
            p = p.ravel()
            P += np.bincount(o, weights=p, minlength=outDim)[:outDim]
            A += np.bincount(o, weights=np.abs(p), minlength=outDim)[:outDim]
            M += np.bincount(o, minlength=outDim)[:outDim]
        h = 2.0 ** -k
        f64 += P
        grid += M * (0.5 * h + TINY)
        rnd += U * A
        mag += np.abs(P)
        var += M * (h * h / 12.0)
    oo, po = _outlier_terms(v64, outliers, outDim)
    ol_err = np.zeros(outDim)
    if oo.size:
        so = np.bincount(oo, weights=po, minlength=outDim)[:outDim]
        sa = np.bincount(oo, weights=np.abs(po), minlength=outDim)[:outDim]
        cnt = np.bincount(oo, minlength=outDim)[:outDim]
        f64 += so
        ol_err = (cnt + 8.0) * U * sa * (1.0 + 2.0 ** -10)             # an f32 chain of cnt fused multiply-adds, split over at most 8 waves
        mag += np.abs(so) + ol_err
    local = grid + rnd                                                    # what the integers are off by
    terms = S + (1 if oo.size else 0)                                     # f32 values combined per output
    f32 = terms * U * (mag + local) * (1.0 + 2.0 ** -10) + ol_err
    return {"f64": f64, "envelope": local + f32, "sigma": np.sqrt(var + (rnd + f32) ** 2), "slices": sl, "counts": counts,
            "grid": grid, "rnd": rnd, "f32": rnd + f32}


def envelope(v, buckets, rows, outDim: int, rankBound: float, sliceRows: int, **kw) -> np.ndarray:
    """Per output, the worst-case |kernel - exact| the documented scheme allows.

    Derivation.  Let slice s hold m_so products p_i of output o, k_s its grid exponent (``grid_exponent`` of L_s = sum|v_j| * rankBound,
    the coarser one where L_s sits within 1e-5 of a power of two), h_s = 2^-k_s.
      1. A product is rounded to f32 once: |error| <= 2^-24 |p_i| (or 2^-150 where the rounding underflows).  Summed over the
         products this is 2^-24 * sum|p_i| -- at most m_so * 2^-24 * max|p_i|, the form the design statement gives.
      2. The scaled value is rounded to the integer grid: |error| <= h_s / 2 per product (floor(x + 0.5) and round-to-nearest
         alike).  Scaling by 2^k_s and back is exact.
      3. Integer sums are exact.  So the slice's integer sum is off by at most  g_so = m_so * (h_s/2 + 2^-150) + 2^-24 sum|p_i|.
      4. The slice's sum becomes an f32 (relative 2^-24), Q4 adds the outliers' f32 sum (a chain of c fused multiply-adds split over
         at most eight waves: (c + 8) * 2^-24 * sum|v * value|), and the T = S (+ 1 with outliers) f32 values of an output are added in
         f32 in some order: at most (T - 1) * 2^-24 * sum of their magnitudes.  With A_o = sum_s (|P_so| + g_so) (+ the outlier sum's
         magnitude and error) steps 4 cost at most T * 2^-24 * A_o, taken with a factor 1 + 2^-10 for the second-order terms.
    envelope_o = sum_s g_so + T * 2^-24 * (1 + 2^-10) * A_o + the outlier chain's error."""
    return error_model(v, buckets, rows, outDim, rankBound, sliceRows, **kw)["envelope"]


def sigma(v, buckets, rows, outDim: int, rankBound: float, sliceRows: int, **kw) -> np.ndarray:
    """Per output, the standard deviation of the same error if the grid roundings (step 2 above) are independent and uniform on
    [-h_s/2, h_s/2]: variance sum_s m_so * h_s^2 / 12; the f32 terms (steps 1 and 4) are taken at their bound and added in
    quadrature."""
    return error_model(v, buckets, rows, outDim, rankBound, sliceRows, **kw)["sigma"]


def z_stats(got, model: dict):
    """(max |got - f64| / envelope, mean z, rms z) with z = (got - f64) / sigma over the outputs whose sigma is not 0; an output
    without any product must be exact and counts as ratio 0 (or inf when it is not)."""
    err = np.asarray(got, np.float64) - model["f64"]
    env, sg = model["envelope"], model["sigma"]
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(env > 0, np.abs(err) / env, np.where(err == 0, 0.0, np.inf))
    ok = sg > 0
    z = err[ok] / sg[ok]
    if not z.size:
        return float(ratio.max()), 0.0, 0.0
    return float(ratio.max()), float(z.mean()), float(np.sqrt((z * z).mean()))


# ------------------------------------------------------------------------------------------------ cosine
def cosine_f64(a, b) -> float:
    """dot / (|a| |b|) in float64 (aux.metal:293-312).  A zero vector gives 0/0 = NaN there (the precalc kernel's sums are 0,
    cosineCalc32 divides by sqrt(0) * sqrt(..) = 0): NaN here as well."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    den = np.sqrt(a @ a) * np.sqrt(b @ b)
    return float("nan") if den == 0.0 else float(a @ b / den)


def cosine_bar(a, b) -> float:
    """Bound on |f32 evaluation - cosine_f64| for ANY summation order of the three n-term f32 sums.
    A sum of n f32 products (each rounded, then n - 1 rounded additions) is off by at most gamma_n * sum|terms|, gamma_n =
    n u / (1 - n u), u = 2^-24.  For the squares sum|terms| is the sum itself: relative gamma_n; a square root halves a relative
    error and adds u; the product of the roots adds u; the quotient adds u.  The dot product is off by gamma_n * sum|a_i b_i| <=
    gamma_n |a||b| (Cauchy-Schwarz), i.e. gamma_n in units of the result's scale.  With |cos| <= 1:
        |error| <= gamma_n  (dot)  +  (gamma_n/2 + gamma_n/2 + 4u) (denominator, relative, times |cos| <= 1),
    taken with a factor 1.01 for the second-order terms."""
    a = np.asarray(a, np.float32).astype(np.float64)
    b = np.asarray(b, np.float32).astype(np.float64)
    n = a.shape[0]
    g = n * U / (1.0 - n * U)
    den = np.sqrt(a @ a) * np.sqrt(b @ b)
    if not den > 0:
        return 0.0
    dot_err = g * float(np.abs(a * b).sum() / den)                     # <= gamma_n (Cauchy-Schwarz); 0 for disjoint supports
    den_err = (g + 4.0 * U) * min(1.0, abs(float(a @ b / den)) + dot_err)
    return 1.01 * (dot_err + den_err)
