"""The float64 references of tests/glue_reference.py, checked without a GPU:

  * each reference against an independent formulation (torch float64 softmax / einsum, a complex rotation, a loop), 1e-12 relative;
  * the margin check: for every case of the GPU tables (tests/test_gpu_glue.py, the dense shapes of tests/test_gpu_parity.py) a plain
    numpy float32 restatement of the same formula sits within HALF of the bar the GPU test uses -- a bar a correct f32 evaluation
    could not meet would say nothing about a kernel.  An input that fails this gets another scale, the bar stays;
  * the bars see a one-token error: corrupted references are rejected by the very comparison functions the GPU tests use."""
import math

import numpy as np
import pytest
import torch

from tests import glue_reference as ref
from tests import test_gpu_glue as T
from tests.test_gpu_parity import DENSE_BAND, DENSE_F64_SHAPES, dense_close
from tests.util import make_v, make_w

F64 = 1e-12


def rel(a, b) -> float:
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


# ---------------------------------------------------------------- the references against independent formulations
@pytest.mark.parametrize("headDim", T.HEAD_DIMS)
def test_rope_is_a_complex_rotation(headDim):
    rng = np.random.default_rng(headDim)
    x = rng.standard_normal((3, headDim))
    half = headDim // 2
    for pos in (0, 1, 77, 8191):
        ang = ref.rope_angles(pos, headDim, T.ROPE_BASE).astype(np.float64)
        z = (x[:, :half] + 1j * x[:, half:]) * np.exp(1j * ang)                   # (lo, hi) is one complex number per frequency
        assert rel(ref.rope(x, pos, T.ROPE_BASE), np.concatenate([z.real, z.imag], axis=1)) <= F64
    # the rounding points: logf, Float(freq), the f32 product
    f = ref.rope_freqs(headDim, T.ROPE_BASE)
    assert f.dtype == np.float32 and f[0] == 1.0 and ref.rope_angles(8191, headDim, T.ROPE_BASE).dtype == np.float32
    logBase = np.float32(math.log(1e6))
    assert all(f[j] == np.float32(math.exp(float(logBase) * (-j / half))) for j in range(half))
    assert abs(float(f[half - 1]) * 1e6 ** (1.0 - 1.0 / half) - 1.0) < 2e-6       # base^(-j / half)


@pytest.mark.parametrize("numHeads,numHeadsKV,headDim,pos", [(4, 2, 64, 0), (4, 1, 128, 33), (2, 2, 256, 257), (12, 6, 64, 65)])
def test_attention_is_the_torch_restatement(numHeads, numHeadsKV, headDim, pos):
    """The float64 version of test_gpu_decode.torch_reference's attention: repeat_interleave, rope by cos / sin with a rotated copy,
    torch.softmax, einsum."""
    case = T.attention_case(numHeads, numHeadsKV, headDim, pos)
    t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))                # noqa: E731
    half, rep = headDim // 2, numHeads // numHeadsKV
    ang = t(ref.rope_angles(pos, headDim, T.ROPE_BASE))

    def rope(x):
        c, s = torch.cos(ang).repeat(2), torch.sin(ang).repeat(2)
        return x * c + torch.cat([-x[:, half:], x[:, :half]], dim=1) * s
    xk = t(case.xk).view(numHeadsKV, headDim).repeat_interleave(rep, 0)
    xv = t(case.xv).view(numHeadsKV, headDim).repeat_interleave(rep, 0)
    K = torch.cat([t(case.kRows), rope(xk)[None]])
    V = torch.cat([t(case.vRows), xv[None]])
    q = rope(t(case.xq).view(numHeads, headDim))
    p = torch.softmax(torch.einsum("hd,thd->ht", q, K) / math.sqrt(headDim), dim=1)
    att = torch.einsum("ht,thd->hd", p, V).reshape(-1)
    assert rel(case.out, att.numpy()) <= F64 and rel(case.kNew, rope(xk).numpy()) <= F64
    assert np.array_equal(case.vNew, xv.numpy())


def test_elementwise_references_against_loops():
    rng = np.random.default_rng(5)
    n = 37
    h, d = rng.standard_normal(n, dtype=np.float32), rng.standard_normal(n, dtype=np.float32)
    w = (1 + 0.1 * rng.standard_normal(n)).astype(np.float16)
    x, out = ref.add_rmsnorm_mul(h, d, w)
    xs = [np.float32(np.float32(a) + np.float32(b)) for a, b in zip(h, d)]
    ms = sum(float(a) ** 2 for a in xs) / n
    assert x.tolist() == [float(a) for a in xs]
    assert rel(out, [float(a) / math.sqrt(ms + 1e-5) * float(b) for a, b in zip(xs, w)]) <= F64
    x0, out0 = ref.add_rmsnorm_mul(h, None, w)
    assert x0.tobytes() == h.tobytes() and rel(out0, ref.add_rmsnorm_mul(h, np.zeros(n, np.float32), w)[1]) <= F64
    x1, x3 = T.silu_case(257)
    sig = [1.0 / (1.0 + math.exp(-float(a))) for a in x1]                          # x3 * x1 * sigmoid(x1)
    assert rel(ref.silu_mul(x1, x3), [float(b) * float(a) * s for a, b, s in zip(x1, x3, sig)]) <= F64
    val = np.array([0.25, 0.75])
    f0, f1 = rng.standard_normal(n), rng.standard_normal(n)
    assert rel(ref.mix2(f0, f1, val), [a * 0.25 + b * 0.75 for a, b in zip(f0, f1)]) <= F64
    assert rel(ref.mix2_add(h, f0, f1, val), [float(c) + (a * 0.25 + b * 0.75) for a, b, c in zip(f0, f1, h)]) <= F64
    table = rng.standard_normal((5, 16)).astype(np.float16)
    assert ref.fetch_row(table, 4).dtype == np.float32 and ref.fetch_row(table.view(np.uint16), 4).tolist() == [float(a) for a in table[4]]


def test_argmax_and_top2_references():
    nan = float("nan")
    assert ref.argmax([1.0, 3.0, 3.0, nan]) == 1 and ref.argmax([nan, nan]) == 0 and ref.argmax([nan, -np.inf, -np.inf]) == 1
    assert ref.argmax([-0.0, 0.0]) == 0 and ref.argmax([5.0]) == 0
    from effort_amd.sampling import topk_reference
    rng = np.random.default_rng(3)
    for n in (1, 5, 1000):
        x = rng.standard_normal(n).astype(np.float32)
        x[rng.random(n) < 0.2] = np.nan
        wi = topk_reference(x, 1)[0]
        assert ref.argmax(x) == (int(wi[0]) if wi.size else 0)
    idx, val = ref.top2_softmax([0.5])
    assert idx.tolist() == [0, 0] and val.tolist() == [0.5, 0.5]
    idx, val = ref.top2_softmax([1.0, 3.0, 3.0, 2.0, 3.0])
    assert idx.tolist() == [1, 2] and val.tolist() == [0.5, 0.5]
    idx, val = ref.top2_softmax([1.0, 4.0, 3.0, 3.0])
    assert idx.tolist() == [1, 2]
    tv, ti = torch.topk(torch.tensor([1.0, 4.0, 3.0, 3.5], dtype=torch.float64), 2)
    idx, val = ref.top2_softmax([1.0, 4.0, 3.0, 3.5])
    assert idx.tolist() == ti.tolist() and rel(val, torch.softmax(tv, 0).numpy()) <= F64
    for n in (1, 2, 8, 64):                                                        # the GPU test's own expectations of its planted rows
        cases = T.top2_cases(n)
        assert all(c.dtype == np.float32 and (c * 64 == np.round(c * 64)).all() for c in cases)
        if n >= 2:
            assert ref.top2_softmax(cases[1])[0].tolist() == [(n - 1) // 2, n - 1]
        if n >= 8:
            assert ref.top2_softmax(cases[2])[0].tolist() == [5, 1] and ref.top2_softmax(cases[3])[0].tolist() == [2, 4]


def test_dense_reference_is_an_exact_dot_product():
    from fractions import Fraction
    W, v = make_w(5, 48, seed=3), make_v(48, seed=9, heavy=True)
    vh = v.astype(np.float16)
    exact = [float(sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(row, vh))) for row in W]
    assert rel(ref.dense(W, v), exact) <= F64 and rel(ref.dense(W.view(np.uint16), v, rows=2), exact) <= F64


# ---------------------------------------------------------------- the margin check: a correct f32 evaluation meets half of every bar
def rope32(x, pos):
    heads, headDim = x.shape
    half = headDim // 2
    a = ref.rope_angles(pos, headDim, T.ROPE_BASE)
    c, s = np.cos(a), np.sin(a)                                                    # float32 in, float32 out
    lo, hi = x[:, :half], x[:, half:]
    return np.concatenate([lo * c - hi * s, hi * c + lo * s], axis=1)


def attention32(case):
    nh, nkv, hd = case.geom
    rep = nh // nkv
    q = rope32(case.xq.reshape(nh, hd), case.pos)
    kNew = rope32(np.repeat(case.xk.reshape(nkv, hd), rep, axis=0), case.pos)
    vNew = np.repeat(case.xv.reshape(nkv, hd), rep, axis=0)
    K, V = np.concatenate([case.kRows, kNew[None]]), np.concatenate([case.vRows, vNew[None]])
    sc = np.einsum("hd,thd->ht", q, K) * np.float32(1.0 / math.sqrt(hd))
    e = np.exp(sc - sc.max(axis=1, keepdims=True))
    out = np.einsum("ht,thd->hd", e / e.sum(axis=1, keepdims=True), V).reshape(-1)
    assert out.dtype == np.float32 and kNew.dtype == np.float32
    return out, kNew


@pytest.mark.parametrize("headDim", T.HEAD_DIMS)
def test_margin_attention(headDim):
    worst = {"table": [0.0, 0.0, 0.0], "long": [0.0, 0.0, 0.0]}
    for nh, nkv, hd, pos, maxTokens in T.attention_cases(headDim):
        assert pos < maxTokens <= 8192 and maxTokens % 64 == 0
        case = T.attention_case(nh, nkv, hd, pos)
        out, kNew = attention32(case)
        assert T.within_bar(out, case.out, 0.5) and T.within_bar(kNew, case.kNew, 0.5), (nh, nkv, hd, pos)
        eo, ek = T.bar_figures(out, case.out), T.bar_figures(kNew, case.kNew)
        w = worst["long" if pos == T.LONG_POS else "table"]
        w[:] = [max(w[0], eo[0]), max(w[1], ek[0]), max(w[2], 1.0 - eo[1])]
    print(f"attention headDim {headDim}: f32 vs f64 worst (out, k row, 1 - cos): {worst}")


def test_margin_markers_and_sequential_steps():
    for headDim in T.HEAD_DIMS:
        for pos in T.MARKER_POSITIONS:
            case, targets = T.marker_case(headDim, pos)
            assert sorted(set(targets)) == sorted({0, 15, 16, 63, 64, 65, 255, 256, 257, pos - 1, pos})
            want = case.out.reshape(T.MARKER_HEADS, headDim)
            out32 = attention32(case)[0].reshape(T.MARKER_HEADS, headDim)
            for h, t in enumerate(targets):                                        # the closed form the GPU test asserts, at half its bar
                assert (np.abs(want[h] - (t + 1)) <= 1e-9 * (t + 1)).all() and (np.abs(out32[h] - (t + 1)) <= 0.5e-6 * (t + 1)).all(), (headDim, pos, h)
        xs, outs, K, V = T.sequential_case(headDim)
        assert len(xs) == T.SEQ_STEPS[headDim] == K.shape[0] and T.max_tokens(len(xs) - 1) >= len(xs)
        nh, nkv = T.SEQ_GEOMETRY
        for pos in (0, len(xs) - 1):                                               # over the f32-rounded cache a kernel reads back
            c = T.AttnCase(nh, nkv, headDim, pos, *xs[pos], K[:pos].astype(np.float32), V[:pos].astype(np.float32))
            assert T.within_bar(attention32(c)[0], outs[pos], 0.5)


def test_margin_norm_and_silu():
    worst = [0.0, 0.0]
    for with_delta in (True, False):
        for n in T.NORM_NS:
            for scale in T.NORM_SCALES:
                h, delta, w = T.norm_case(n, scale, with_delta)
                x, want = ref.add_rmsnorm_mul(h, delta, w)
                x32 = h + delta if with_delta else h
                out = x32 / np.sqrt(np.mean(x32 * x32) + np.float32(1e-5)) * w.astype(np.float32)
                assert out.dtype == np.float32 and x32.tobytes() == x.tobytes()
                assert T.within_bar(out, want, 0.5), (n, scale, with_delta, T.bar_figures(out, want))
                e = T.bar_figures(out, want)
                worst = [max(worst[0], e[0]), max(worst[1], 1.0 - e[1])]
    print(f"add_rmsnorm_mul: f32 vs f64 worst (err, 1 - cos): {worst}")
    ws = 0.0
    for n in T.SILU_NS:
        x1, x3 = T.silu_case(n)
        assert set(np.float32(T.SILU_PLANTED[:n]).tolist()) <= set(x1.tolist()) and (n == 1 or np.signbit(x1[x1 == 0]).any())
        want = ref.silu_mul(x1, x3)
        with np.errstate(over="ignore"):
            out = x3 * x1 / (np.float32(1.0) + np.exp(-x1))
        assert out.dtype == np.float32 and T.silu_within_bar(out, want, 0.5), n
        ws = max(ws, float((np.abs(out - want) / (2e-6 * np.abs(want) + 2.0 ** -126)).max()))
    print(f"silu_mul: f32 vs f64 worst error over the bar: {ws:.3g}")


@pytest.mark.parametrize("outDim,inDim", DENSE_F64_SHAPES + [(1027, 4112)])
def test_margin_dense(outDim, inDim):
    W, v = make_w(outDim, inDim, seed=3), make_v(inDim, seed=9, heavy=True)
    want = ref.dense(W, v)
    vh = v.astype(np.float16).astype(np.float32)
    out = np.concatenate([W[r:r + 1024].astype(np.float32) @ vh for r in range(0, outDim, 1024)])
    assert out.dtype == np.float32 and dense_close(out, want, 0.5 * DENSE_BAND)
    frac = float((np.abs(out - want) / (DENSE_BAND * np.abs(want).max() + DENSE_BAND * np.abs(want))).max())
    print(f"dense ({outDim}, {inDim}): f32 matmul vs f64, worst error over the band: {frac:.3g}")


# ---------------------------------------------------------------- the bars see a one-token error
def test_bar_rejects_a_dropped_token():
    """Token 64 left out of the sum at pos = 1025 (the first token of a second pass at headDim 128): about 1e-2 of max|want|."""
    nh, nkv, hd, pos = 4, 2, 128, 1025
    case = T.attention_case(nh, nkv, hd, pos)
    keep = np.arange(pos) != 64
    bad, _, _ = ref.rope_attention(case.xq, case.xk, case.xv, case.kRows[keep], case.vRows[keep], pos - 1, nh, nkv, hd, T.ROPE_BASE,
                                   angles=ref.rope_angles(pos, hd, T.ROPE_BASE))
    assert T.within_bar(case.out, case.out) and not T.within_bar(bad, case.out)
    assert T.bar_figures(bad, case.out)[0] > 100 * T.BAR_REL
    nan = case.out.copy()
    nan[3] = np.nan
    assert not T.within_bar(nan, case.out)                                        # one 0 * NaN anywhere fails


def test_bar_rejects_a_shifted_norm_weight():
    for n in (1000, 4097):
        h, delta, w = T.norm_case(n, 1.0, True)
        _, want = ref.add_rmsnorm_mul(h, delta, w)
        _, bad = ref.add_rmsnorm_mul(h, delta, np.roll(w, -1))                    # w[i + 1] for w[i]
        assert not T.within_bar(bad, want)


@pytest.mark.parametrize("headDim", T.HEAD_DIMS)
def test_bar_rejects_a_float64_rope_angle(headDim):
    """Why the rounding point is mirrored: at pos 8191 an angle formed in float64 is off by up to 5e-4 rad from the specified one."""
    nh, nkv, pos = T.LONG_GEOMETRY[0], T.LONG_GEOMETRY[1], T.LONG_POS
    rng = np.random.default_rng(headDim)
    xk = rng.standard_normal(nkv * headDim, dtype=np.float32)
    exact = float(pos) * ref.rope_freqs(headDim, T.ROPE_BASE).astype(np.float64)
    assert np.abs(exact - ref.rope_angles(pos, headDim, T.ROPE_BASE)).max() > 5e-5
    want = ref.rope(np.repeat(xk.reshape(nkv, headDim), nh // nkv, axis=0), pos, T.ROPE_BASE)
    bad = ref.rope(np.repeat(xk.reshape(nkv, headDim), nh // nkv, axis=0), pos, T.ROPE_BASE, angles=exact)
    assert not T.within_bar(bad, want)
