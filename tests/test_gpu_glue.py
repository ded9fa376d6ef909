"""The decode glue kernels (effort_amd/csrc/decode.hip) through the C ABI against the float64 references of tests/glue_reference.py.

Bars, and where each comes from:
  * f32 outputs with no defined summation order (attention, rope, add_rmsnorm_mul): the project's bar of tests/test_gpu_parity.py,
    |got - want| <= 2e-5 * max|want|  and  cos-sim >= 0.999999  (``within_bar``);
  * silu_mul, per element: |got - want| <= 2e-6 * |want| + 2^-126 -- five f32 roundings and an expf of at most 2 ulp stay below
    8 * 2^-24 = 5e-7, times four; 2^-126 (the smallest normal f32) covers the lanes where exp(100) overflows and the quotient is 0;
  * marker cases: 1e-6 relative -- the winning score is 40, the other nTok - 1 tokens carry at most nTok * e^-40 = 4e-15 together;
  * top2_softmax values: 4 ulp (expf, one add, one division, one product); its indices, fetch_row, mix2, mix2_add, the v row, every
    cache row a step does not own, the stored h and all guard elements: bit-exact.

Cache rows at and past the position, and every output buffer, hold NaN before a call: NaN is data here, nothing runs past a buffer; a
single 0 * NaN from a row that should not have been read shows in the result.

What a correct f32 evaluation leaves of these bars (tests/test_glue_reference_cpu.py asserts at most half of each, for every case
of the tables below; plain numpy float32 restatement against the float64 reference, error over max|want|, worst case of each row):

    attention  headDim  64   pos <= 1025   out 1.6e-6   k row 9.8e-8   1 - cos 3.2e-13        pos 8191   out 2.1e-6   k row 4.3e-8
    attention  headDim 128   pos <= 1025   out 1.7e-6   k row 1.0e-7   1 - cos 3.3e-13        pos 8191   out 3.8e-6   k row 1.0e-7
    attention  headDim 256   pos <= 1025   out 2.0e-6   k row 9.6e-8   1 - cos 3.7e-13        pos 8191   out 3.3e-6   k row 6.3e-8
    add_rmsnorm_mul   every n, scale, with and without delta             out 1.3e-7   1 - cos 8.9e-16
    silu_mul          worst element, error over (2e-6 * |want| + 2^-126)     0.11
    dense (tests/test_gpu_parity.py, 1e-5 band): error over the band, numpy f32 matmul
               (8193, 512) 0.016   (8200, 4096) 0.035   (8192, 4112) 0.040   (24, 24592) 0.026   (16, 65536) 0.057   (1027, 4112) 0.040
"""
import ctypes as C
import math

import numpy as np
import pytest

from tests import glue_reference as ref
from tests.util import cos

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BAR_REL, BAR_COS = 2e-5, 0.999999                       # tests/test_gpu_parity.py: ATOL_REL and its cos-sim bar
ROPE_BASE = 1e6

HEAD_DIMS = (64, 128, 256)
GEOMETRIES = ((4, 2), (2, 2), (4, 1))                    # (numHeads, numHeadsKV)
# one below, at and one above every pass boundary of the three head sizes, and both sides of the 256-token softmax stride
POSITIONS = (0, 1, 15, 16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025)
LONG_GEOMETRY, LONG_POS = (2, 1), 8191                   # the last valid slot of the largest cache the ABI takes


def max_tokens(pos: int) -> int:
    return (pos + 1 + 63) // 64 * 64


def attention_cases(headDim: int):
    """(numHeads, numHeadsKV, headDim, pos, maxTokens) of the attention table."""
    cases = [(nh, nkv, headDim, pos, max_tokens(pos)) for nh, nkv in GEOMETRIES for pos in POSITIONS]
    return cases + [(*LONG_GEOMETRY, headDim, LONG_POS, 8192)]


# ---------------------------------------------------------------- the bars
def bar_figures(got, want):
    """(max|got - want| / max|want|, cos-sim) -- NaN when got holds one."""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return float(np.abs(got - want).max() / (np.abs(want).max() + 1e-300)), cos(got, want)


def within_bar(got, want, fraction: float = 1.0) -> bool:
    """The project's f32 bar; ``fraction`` < 1 asks for that part of it (the margin check: 0.5).  A NaN fails."""
    err, c = bar_figures(got, want)
    return bool(err <= fraction * BAR_REL and 1.0 - c <= fraction * (1.0 - BAR_COS))


def silu_within_bar(got, want, fraction: float = 1.0) -> bool:
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool((np.abs(got - want) <= fraction * (2e-6 * np.abs(want) + 2.0 ** -126)).all())


# ---------------------------------------------------------------- inputs (numpy only: the CPU margin check builds the same cases)
class AttnCase:
    """One decode step: inputs as f32, the cache rows 0 .. pos-1 as given, and the float64 reference's answer."""

    def __init__(self, numHeads, numHeadsKV, headDim, pos, xq, xk, xv, kRows, vRows):
        self.geom = (numHeads, numHeadsKV, headDim)
        self.pos, self.xq, self.xk, self.xv, self.kRows, self.vRows = pos, xq, xk, xv, kRows, vRows
        self.out, self.kNew, self.vNew = ref.rope_attention(xq, xk, xv, kRows, vRows, pos, numHeads, numHeadsKV, headDim, ROPE_BASE)


def attention_case(numHeads, numHeadsKV, headDim, pos) -> AttnCase:
    rng = np.random.default_rng([headDim, numHeads, numHeadsKV, pos])
    f = lambda *shape: rng.standard_normal(shape, dtype=np.float32)                     # noqa: E731
    return AttnCase(numHeads, numHeadsKV, headDim, pos, f(numHeads * headDim), f(numHeadsKV * headDim), f(numHeadsKV * headDim),
                    f(pos, numHeads, headDim), f(pos, numHeads, headDim))


MARKER_HEADS, MARKER_HEADS_KV = 12, 6
MARKER_POSITIONS = (300, 1030)


def marker_targets(pos: int):
    """t* of the 12 heads: ten heads each their own, the last KV group (two heads) the newest token."""
    return [0, 15, 16, 63, 64, 65, 255, 256, 257, pos - 1, pos, pos]


def marker_case(headDim: int, pos: int):
    """v row t = t + 1 in every lane (xv: pos + 1); keys zero except head h's row t*_h = c_h * rope(q_h), c_h such that the winning
    score is 40; for t* = pos the key comes through xk = c * xq, the two query heads of that KV group being equal.
    Returns (AttnCase, targets)."""
    nh, nkv = MARKER_HEADS, MARKER_HEADS_KV
    rng = np.random.default_rng([7, headDim, pos])
    xq = rng.standard_normal((nh, headDim), dtype=np.float32)
    xq[nh - 1] = xq[nh - 2]
    targets = marker_targets(pos)
    c = 40.0 * math.sqrt(headDim) / (xq.astype(np.float64) ** 2).sum(axis=1)
    qr = ref.rope(xq, pos, ROPE_BASE)
    kRows = np.zeros((pos, nh, headDim), dtype=np.float32)
    xk = np.zeros((nkv, headDim), dtype=np.float32)
    for h, t in enumerate(targets):
        if t < pos:
            kRows[t, h] = (c[h] * qr[h]).astype(np.float32)
    xk[nkv - 1] = (c[nh - 1] * xq[nh - 1].astype(np.float64)).astype(np.float32)
    vRows = np.broadcast_to(np.arange(1, pos + 1, dtype=np.float32)[:, None, None], (pos, nh, headDim)).copy()
    xv = np.full((nkv, headDim), pos + 1, dtype=np.float32)
    return AttnCase(nh, nkv, headDim, pos, xq.reshape(-1), xk.reshape(-1), xv.reshape(-1), kRows, vRows), targets


SEQ_GEOMETRY = (4, 2)
SEQ_STEPS = {64: 70, 128: 70, 256: 40}
_SEQ = {}


def sequential_case(headDim: int):
    """Per-step inputs and the reference's outputs over its own growing float64 cache; computed once per head size."""
    if headDim not in _SEQ:
        nh, nkv = SEQ_GEOMETRY
        steps = SEQ_STEPS[headDim]
        rng = np.random.default_rng([11, headDim])
        xs = [tuple(rng.standard_normal(n * headDim, dtype=np.float32) for n in (nh, nkv, nkv)) for _ in range(steps)]
        K, V, outs = np.zeros((0, nh, headDim)), np.zeros((0, nh, headDim)), []
        for pos, (xq, xk, xv) in enumerate(xs):
            out, kNew, vNew = ref.rope_attention(xq, xk, xv, K, V, pos, nh, nkv, headDim, ROPE_BASE)
            K, V = np.concatenate([K, kNew[None]]), np.concatenate([V, vNew[None]])
            outs.append(out)
        _SEQ[headDim] = (xs, outs, K, V)
    return _SEQ[headDim]


NORM_NS = (1, 63, 64, 1000, 1024, 1025, 4095, 4096, 4097, 5120, 16384)      # both sides of the register / loop switch at 4096
NORM_SCALES = (1e-3, 1.0, 1e3)                                               # at 1e-3 the epsilon is as large as the mean square


def norm_case(n: int, scale: float, with_delta: bool):
    """(h f32, delta f32 or None, w f16)."""
    rng = np.random.default_rng([13, n, int(round(math.log10(scale))) + 10, int(with_delta)])
    h = (rng.standard_normal(n, dtype=np.float32) * np.float32(scale)).astype(np.float32)
    delta = (rng.standard_normal(n, dtype=np.float32) * np.float32(0.5 * scale)).astype(np.float32) if with_delta else None
    w = (1.0 + 0.1 * rng.standard_normal(n)).astype(np.float16)
    return h, delta, w


SILU_NS = (1, 255, 256, 257, 14336)
SILU_PLANTED = (0.0, -0.0, 1e-30, -1e-30, 20.0, -20.0, 87.0, -87.0, -100.0)


def silu_case(n: int):
    """x1 ~ N(0, 3) with the planted values spread over it (as many as fit), x3 ~ N(0, 1)."""
    rng = np.random.default_rng([17, n])
    x1 = (rng.standard_normal(n, dtype=np.float32) * np.float32(3.0)).astype(np.float32)
    x3 = rng.standard_normal(n, dtype=np.float32)
    where = np.linspace(0, n - 1, len(SILU_PLANTED)).astype(np.int64) if n >= len(SILU_PLANTED) else np.arange(n)
    x1[where] = np.array(SILU_PLANTED, dtype=np.float32)[:where.size]
    if n > 300:                                                                # ... and each once more in the last block's ragged tail
        x1[n - len(SILU_PLANTED):] = np.array(SILU_PLANTED, dtype=np.float32)
    return x1, x3


# ---------------------------------------------------------------- GPU plumbing
@pytest.fixture(scope="module")
def gpu(hip_lib_built):
    import effort_amd
    import torch
    torch.cuda.set_device(0)
    g = effort_amd.gpu()
    g._bind_stream()
    return g


def lib():
    from effort_amd import _lib
    return _lib.lib()


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def nans(*shape):
    import torch
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def decode_status(g) -> int:
    st = C.c_int(0)
    g.check(lib().effort_decode_status(g.ctx, C.byref(st)), "decode_status")
    return int(st.value)


def launch_step(g, xq, xk, xv, kc, vc, posd, out, geom, maxTokens, fused):
    """One decode step's attention on device buffers: the fused launch, or rope_kv then attention."""
    nh, nkv, hd = geom
    rope = C.c_float(ROPE_BASE)
    if fused:
        g.check(lib().effort_rope_attention(g.ctx, P(xq), P(xk), P(xv), P(kc), P(vc), P(posd), P(out), nh, nkv, hd, maxTokens, rope), "rope_attention")
    else:
        q = nans(nh * hd)
        g.check(lib().effort_rope_kv(g.ctx, P(xq), P(xk), P(xv), P(q), P(kc), P(vc), P(posd), nh, nkv, hd, maxTokens, rope), "rope_kv")
        g.check(lib().effort_attention(g.ctx, P(q), P(kc), P(vc), P(posd), P(out), nh, hd, maxTokens), "attention")


def run_case(g, case: AttnCase, maxTokens: int, fused: bool):
    """The case on fresh buffers, every cache row >= pos and the output NaN beforehand.  Asserts everything that is exact (the v row,
    every other cache row, pos, the status word) and returns (out, k row pos) for the caller's bar."""
    import torch
    nh, nkv, hd = case.geom
    pos = case.pos
    rows = lambda a: np.concatenate([a, np.full((maxTokens - pos, nh, hd), np.nan, dtype=np.float32)])       # noqa: E731
    kc, vc = dev(rows(case.kRows)), dev(rows(case.vRows))
    kc0, vc0 = kc.clone(), vc.clone()
    out = nans(nh * hd)
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    launch_step(g, dev(case.xq), dev(case.xk), dev(case.xv), kc, vc, posd, out, case.geom, maxTokens, fused)
    g.eval()
    tag = (case.geom, pos, "fused" if fused else "two launches")
    assert int(posd.item()) == pos, tag
    for now, before in ((kc, kc0), (vc, vc0)):                                  # every row but pos: bit for bit, NaN rows included
        a, b = now.view(torch.int32), before.view(torch.int32)
        assert torch.equal(a[:pos], b[:pos]) and torch.equal(a[pos + 1:], b[pos + 1:]), tag
    vGot = vc[pos].cpu().numpy()
    assert vGot.view(np.int32).tolist() == case.vNew.astype(np.float32).view(np.int32).tolist(), tag
    return out.cpu().numpy(), kc[pos].cpu().numpy()


# ---------------------------------------------------------------- attention and rope
@pytest.mark.parametrize("headDim", HEAD_DIMS)
def test_attention_matches_float64(gpu, headDim):
    gpu._bind_stream()
    decode_status(gpu)                                                          # (clears whatever an earlier test left)
    worst = {}
    for nh, nkv, hd, pos, maxTokens in attention_cases(headDim):
        case = attention_case(nh, nkv, hd, pos)
        for fused in (True, False):
            out, kRow = run_case(gpu, case, maxTokens, fused)
            eo, ek = bar_figures(out, case.out), bar_figures(kRow, case.kNew)
            key = ("fused" if fused else "two", "long" if pos == LONG_POS else "table")
            worst[key] = tuple(max(a, b) for a, b in zip(worst.get(key, (0.0, 0.0, 0.0)), (eo[0], ek[0], 1.0 - eo[1])))
            assert within_bar(out, case.out), (nh, nkv, hd, pos, fused, eo)
            assert within_bar(kRow, case.kNew), (nh, nkv, hd, pos, fused, ek)
    print(f"headDim {headDim}: worst (out err, k row err, 1 - cos) per path: {worst}")
    assert decode_status(gpu) == 0


@pytest.mark.parametrize("headDim", HEAD_DIMS)
def test_attention_marker_tokens(gpu, headDim):
    """Every head's softmax sits on ONE token, another one per head: out == t* + 1.  A token that is dropped, clamped onto its
    neighbour or read from another head's row is off by at least 1 here, where random data would only shift a little."""
    gpu._bind_stream()
    decode_status(gpu)
    for pos in MARKER_POSITIONS:
        case, targets = marker_case(headDim, pos)
        for fused in (True, False):
            out, _ = run_case(gpu, case, max_tokens(pos), fused)
            out = out.reshape(MARKER_HEADS, headDim).astype(np.float64)
            for h, t in enumerate(targets):
                assert (np.abs(out[h] - (t + 1)) <= 1e-6 * (t + 1)).all(), (headDim, pos, fused, h, t, out[h, :4].tolist())
    assert decode_status(gpu) == 0


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-launch"])
@pytest.mark.parametrize("headDim", HEAD_DIMS)
def test_attention_sequential_steps(gpu, headDim, fused):
    """Steps 0 .. n-1 on one cache that starts as NaN: the kernel's own cache writes feed the next step; the position is written
    from the host between calls.  Each step's out against the reference's own growing cache."""
    import torch
    gpu._bind_stream()
    decode_status(gpu)
    nh, nkv = SEQ_GEOMETRY
    xs, outs, K, V = sequential_case(headDim)
    steps = len(xs)
    maxTokens = max_tokens(steps - 1)
    kc, vc = nans(maxTokens, nh, headDim), nans(maxTokens, nh, headDim)
    posd = torch.zeros(1, dtype=torch.int32, device=DEV)
    got = []
    for pos, (xq, xk, xv) in enumerate(xs):
        posd.fill_(pos)
        out = nans(nh * headDim)
        launch_step(gpu, dev(xq), dev(xk), dev(xv), kc, vc, posd, out, (nh, nkv, headDim), maxTokens, fused)
        got.append(out)
    gpu.eval()
    for pos, (out, want) in enumerate(zip(got, outs)):
        assert within_bar(out.cpu().numpy(), want), (headDim, fused, pos, bar_figures(out.cpu().numpy(), want))
    assert within_bar(kc[:steps].cpu().numpy(), K) and within_bar(vc[:steps].cpu().numpy(), V)
    assert bool(torch.isnan(kc[steps:]).all()) and bool(torch.isnan(vc[steps:]).all())
    assert int(posd.item()) == steps - 1 and decode_status(gpu) == 0


# ---------------------------------------------------------------- add_rmsnorm_mul
GUARD = 8


@pytest.mark.parametrize("with_delta", [True, False], ids=["delta", "no-delta"])
def test_add_rmsnorm_mul_matches_float64(gpu, with_delta):
    import torch
    gpu._bind_stream()
    runs = []
    for n in NORM_NS:
        for scale in NORM_SCALES:
            h, delta, w = norm_case(n, scale, with_delta)
            hd = torch.full((n + GUARD,), 777.0, device=DEV)
            hd[:n] = dev(h)
            out = torch.full((n + GUARD,), -555.0, device=DEV)
            out[:n] = float("nan")
            dd, wd = dev(delta) if with_delta else None, dev(w.view(np.int16))
            gpu.check(lib().effort_add_rmsnorm_mul(gpu.ctx, P(hd), P(dd), P(wd), P(out), n), "rmsnorm")
            runs.append((n, scale, h, delta, w, hd, out))
    gpu.eval()
    worst = 0.0
    for n, scale, h, delta, w, hd, out in runs:
        x, want = ref.add_rmsnorm_mul(h, delta, w)
        hGot, oGot = hd.cpu().numpy(), out.cpu().numpy()
        assert hGot[:n].view(np.int32).tolist() == x.view(np.int32).tolist(), (n, scale)        # f32(h + delta); untouched without a delta
        assert (hGot[n:] == 777.0).all() and (oGot[n:] == -555.0).all(), (n, scale)
        worst = max(worst, bar_figures(oGot[:n], want)[0])
        assert within_bar(oGot[:n], want), (n, scale, bar_figures(oGot[:n], want))
    print(f"add_rmsnorm_mul delta={with_delta}: worst err / max|want| {worst:.3g}")


# ---------------------------------------------------------------- silu_mul
def test_silu_mul_matches_float64(gpu):
    import torch
    gpu._bind_stream()
    runs = []
    for n in SILU_NS:
        x1, x3 = silu_case(n)
        out = torch.full((n + GUARD,), -555.0, device=DEV)
        out[:n] = float("nan")
        x1d, x3d = dev(x1), dev(x3)
        gpu.check(lib().effort_silu_mul(gpu.ctx, P(x1d), P(x3d), P(out), n), "silu")
        runs.append((n, x1, x3, out))
    gpu.eval()
    for n, x1, x3, out in runs:
        want = ref.silu_mul(x1, x3)
        got = out.cpu().numpy()
        assert (got[n:] == -555.0).all(), n
        bad = np.flatnonzero(~(np.abs(got[:n] - want) <= 2e-6 * np.abs(want) + 2.0 ** -126))
        assert silu_within_bar(got[:n], want), (n, [(float(x1[i]), float(x3[i]), float(got[i]), float(want[i])) for i in bad[:4]])


# ---------------------------------------------------------------- the exact kernels
def test_fetch_row_is_exact(gpu):
    import torch
    gpu._bind_stream()
    rng = np.random.default_rng(19)
    for n in (4096, 1000):
        table = (rng.standard_normal((300, n)) * 0.05).astype(np.float16)
        td = dev(table.view(np.int16))
        for rowId in (0, 1, 299):
            out = torch.full((n + GUARD,), -555.0, device=DEV)
            out[:n] = float("nan")
            idd = torch.tensor([rowId], dtype=torch.int32, device=DEV)
            gpu.check(lib().effort_fetch_row(gpu.ctx, P(td), P(idd), P(out), n), "fetch_row")
            gpu.eval()
            got = out.cpu().numpy()
            assert got[:n].view(np.int32).tolist() == ref.fetch_row(table, rowId).view(np.int32).tolist(), (n, rowId)
            assert (got[n:] == -555.0).all(), (n, rowId)


@pytest.mark.parametrize("n", [1, 1000, 4096])
def test_mix2_and_mix2_add_are_the_f32_expression(gpu, n):
    """Two products, one add, then one add into h, each rounded to f32 (the build does not contract them into an fma)."""
    import torch
    gpu._bind_stream()
    rng = np.random.default_rng([23, n])
    h, f0, f1 = (rng.standard_normal(n, dtype=np.float32) * np.float32(s) for s in (3.0, 1.0, 0.5))
    val = np.array([0.6180339, 0.3819661], dtype=np.float32)
    mix = (f0 * val[0] + f1 * val[1]).astype(np.float32)
    mixed = (h + mix).astype(np.float32)
    out = torch.full((n + GUARD,), -555.0, device=DEV)
    hd = torch.full((n + GUARD,), 777.0, device=DEV)
    hd[:n] = dev(h)
    f0d, f1d, vd = dev(f0), dev(f1), dev(val)
    gpu.check(lib().effort_mix2(gpu.ctx, P(f0d), P(f1d), P(vd), P(out), n), "mix2")
    gpu.check(lib().effort_mix2_add(gpu.ctx, P(hd), P(f0d), P(f1d), P(vd), n), "mix2_add")
    gpu.eval()
    oGot, hGot = out.cpu().numpy(), hd.cpu().numpy()
    assert oGot[:n].view(np.int32).tolist() == mix.view(np.int32).tolist()
    assert hGot[:n].view(np.int32).tolist() == mixed.view(np.int32).tolist()
    assert (oGot[n:] == -555.0).all() and (hGot[n:] == 777.0).all()
    assert np.abs(oGot[:n] - ref.mix2(f0, f1, val)).max() <= 4e-7 * np.abs(mix).max() + 1e-30          # (and the f32 expression is the float64 one to three roundings)
    assert np.abs(hGot[:n] - ref.mix2_add(h, f0, f1, val)).max() <= 4e-7 * (np.abs(h).max() + np.abs(mix).max())


def top2_cases(n: int):
    """Gate logits on a grid of 1/64 (differences are exact in f32: the softmax's only roundings are the kernel's own): one random
    row, and rows with planted ties for the first and for the second place."""
    rng = np.random.default_rng([29, n])
    base = (np.round(rng.standard_normal(n) * 64.0) / 64.0).astype(np.float32)
    cases = [base]
    if n >= 2:
        tie = base.copy()
        tie[[(n - 1) // 2, n - 1]] = base.max() + 1.0                            # two winners: the first index, then the second
        cases.append(tie)
    if n >= 8:
        second = base.copy()
        second[5] = base.max() + 2.0
        second[[1, 3, 6]] = base.max() + 1.0                                     # three runners-up: the first of them
        three = base.copy()
        three[[2, 4, 7]] = base.max() + 0.5                                      # three winners: the first two
        cases += [second, three]
    return cases


@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_top2_softmax_matches_float64(gpu, n):
    import torch
    gpu._bind_stream()
    for k, gate in enumerate(top2_cases(n)):
        idx = torch.full((2,), -1, dtype=torch.int32, device=DEV)
        val = nans(2)
        gd = dev(gate)
        gpu.check(lib().effort_top2_softmax(gpu.ctx, P(gd), n, P(idx), P(val)), "top2")
        gpu.eval()
        wantIdx, wantVal = ref.top2_softmax(gate)
        got = val.cpu().numpy()
        assert idx.cpu().tolist() == wantIdx.tolist(), (n, k)
        ulp = np.spacing(wantVal.astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - wantVal) <= 4 * ulp).all(), (n, k, got.tolist(), wantVal.tolist())
        if n == 1:
            assert idx.cpu().tolist() == [0, 0] and got.tolist() == [0.5, 0.5]
        if k == 1:
            assert idx.cpu().tolist() == [(n - 1) // 2, n - 1] and got.tolist() == [0.5, 0.5]
        if k == 2:
            assert idx.cpu().tolist() == [5, 1]
        if k == 3:
            assert idx.cpu().tolist() == [2, 4]
