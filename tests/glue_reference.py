"""Plain numpy float64 references of the decode glue (effort_amd/csrc/decode.hip) and of the dense GEMV (csrc/gemv.hip).

Every function restates the OPERATION, not a kernel: no tiles, passes, clamps or summation orders.  The specification fixes a few
float32 rounding points (the launcher's logf, ``Float(freq)`` of createFreqsCis2, the f32 angle, the one f32 add of the residual, the
f16 input of basicMul); exactly those are mirrored, everything else is float64.  Importable without a GPU."""
import math

import numpy as np


def f16_to_f64(a) -> np.ndarray:
    """f16 values (dtype float16, or their bits as uint16 / int16) widened to float64."""
    a = np.asarray(a)
    if a.dtype != np.float16:
        a = a.view(np.float16)
    return a.astype(np.float64)


# ---------------------------------------------------------------- rope
def rope_freqs(headDim: int, ropeBase: float) -> np.ndarray:
    """freq_j, j = 0 .. headDim/2 - 1, as float32: logBase = f32(log(f32(ropeBase))), freq_j = f32(exp(f64(logBase) * (-j / half)))."""
    half = headDim // 2
    logBase = np.float32(math.log(float(np.float32(ropeBase))))
    j = np.arange(half, dtype=np.float64)
    return np.exp(np.float64(logBase) * (-j / half)).astype(np.float32)


def rope_angles(pos: int, headDim: int, ropeBase: float) -> np.ndarray:
    """angle_j = f32(f32(pos) * freq_j): the f32 product is the specification's rounding point, not an approximation of it."""
    return (np.float32(pos) * rope_freqs(headDim, ropeBase)).astype(np.float32)


def rope(x, pos: int, ropeBase: float, angles=None) -> np.ndarray:
    """Rotate-half rope of x [heads, headDim] at position pos; float64 out.  ``angles`` overrides the [headDim / 2] angles."""
    x = np.asarray(x, dtype=np.float64)
    heads, headDim = x.shape
    half = headDim // 2
    a = np.asarray(rope_angles(pos, headDim, ropeBase) if angles is None else angles, dtype=np.float64)
    c, s = np.cos(a), np.sin(a)
    lo, hi = x[:, :half], x[:, half:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=1)


# ---------------------------------------------------------------- attention
def attention(q, K, V) -> np.ndarray:
    """softmax(q . k_t / sqrt(headDim)) over the T rows of K, V [T, heads, headDim]; q [heads, headDim]; out [heads * headDim]."""
    q, K, V = (np.asarray(a, dtype=np.float64) for a in (q, K, V))
    headDim = q.shape[1]
    sc = np.einsum("hd,thd->ht", q, K) / math.sqrt(headDim)
    e = np.exp(sc - sc.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    return np.einsum("ht,thd->hd", p, V).reshape(-1)


def rope_attention(xq, xk, xv, kRows, vRows, pos: int, numHeads: int, numHeadsKV: int, headDim: int, ropeBase: float, angles=None):
    """One decode step's attention.  xq [numHeads * headDim], xk / xv [numHeadsKV * headDim], kRows / vRows = cache rows 0 .. pos-1 as
    given, [pos, numHeads, headDim].  Row pos is the newly roped k and the new v, KV head y feeding query heads y*rep .. y*rep+rep-1.
    Returns (out [numHeads * headDim], k row [numHeads, headDim], v row [numHeads, headDim]), all float64."""
    rep = numHeads // numHeadsKV
    q = rope(np.asarray(xq).reshape(numHeads, headDim), pos, ropeBase, angles)
    kNew = rope(np.repeat(np.asarray(xk).reshape(numHeadsKV, headDim), rep, axis=0), pos, ropeBase, angles)
    vNew = np.repeat(np.asarray(xv, dtype=np.float64).reshape(numHeadsKV, headDim), rep, axis=0)
    K = np.concatenate([np.asarray(kRows, dtype=np.float64).reshape(pos, numHeads, headDim), kNew[None]], axis=0)
    V = np.concatenate([np.asarray(vRows, dtype=np.float64).reshape(pos, numHeads, headDim), vNew[None]], axis=0)
    return attention(q, K, V), kNew, vNew


# ---------------------------------------------------------------- the norm and the element-wise glue
def add_rmsnorm_mul(h, delta, w):
    """x = f32(h + delta) (one f32 add: what is stored back to h; x = h without a delta); out = x / sqrt(mean(x^2) + 1e-5) * w in
    float64.  w: f16.  Returns (x float32, out float64)."""
    x = np.asarray(h, dtype=np.float32)
    if delta is not None:
        x = (x + np.asarray(delta, dtype=np.float32)).astype(np.float32)
    x64 = x.astype(np.float64)
    return x, x64 / math.sqrt(float(np.mean(x64 * x64)) + 1e-5) * f16_to_f64(w)


def silu_mul(x1, x3) -> np.ndarray:
    x1, x3 = np.asarray(x1, dtype=np.float64), np.asarray(x3, dtype=np.float64)
    return x3 * x1 / (1.0 + np.exp(-x1))


def fetch_row(table, rowId: int) -> np.ndarray:
    """Row rowId of the f16 table [rows, n], widened to f32 (exact)."""
    t = np.asarray(table)
    if t.dtype != np.float16:
        t = t.view(np.float16)
    return t[rowId].astype(np.float32)


def argmax(logits) -> int:
    """Index of the largest non-NaN logit, the lowest index on ties; 0 when every logit is NaN."""
    x = np.asarray(logits, dtype=np.float64)
    ok = ~np.isnan(x)
    if not ok.any():
        return 0
    return int(np.flatnonzero(ok & (x == x[ok].max()))[0])


def mix2(f0, f1, val) -> np.ndarray:
    f0, f1, val = (np.asarray(a, dtype=np.float64) for a in (f0, f1, val))
    return f0 * val[0] + f1 * val[1]


def mix2_add(h, f0, f1, val) -> np.ndarray:
    return np.asarray(h, dtype=np.float64) + mix2(f0, f1, val)


def top2_softmax(gate):
    """The two largest logits (the first index on ties; one logit alone is picked twice) and the softmax of the two.
    Returns (idx [2] int64, val [2] float64)."""
    g = np.asarray(gate, dtype=np.float64)
    order = np.argsort(-g, kind="stable")
    i0 = int(order[0])
    i1 = int(order[1]) if g.size > 1 else i0
    e = np.exp(np.array([0.0, g[i1] - g[i0]]))
    return np.array([i0, i1], dtype=np.int64), e / e.sum()


# ---------------------------------------------------------------- dense
def dense(W, v, rows: int = 1024) -> np.ndarray:
    """basicMul: f16->f64(W) @ f64(f16(v)); W f16 [outDim, inDim] (converted a block of rows at a time: the result does not depend on it)."""
    W = np.asarray(W)
    if W.dtype != np.float16:
        W = W.view(np.float16)
    vh = np.asarray(v, dtype=np.float32).astype(np.float16).astype(np.float64)
    return np.concatenate([W[r:r + rows].astype(np.float64) @ vh for r in range(0, W.shape[0], rows)])
