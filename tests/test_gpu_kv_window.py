"""Sliding-window attention over the rolling f16 KV cache [ringRows][numHeadsKV][headDim], token t in row t % ringRows
(effort_amd/csrc/kv_window.hip, ``Decoder(kv_cache="f16", window=W)``).  The writers are held to the bits of the f16 writers, both
attentions to the float64 reference ``glue_reference.attention`` over the halves the ring HOLDS for the tokens of the window, at the
project's f32 bar (``within_bar``), and -- below the window -- to the bits of the kernels on the plain f16 cache.  Every ring row outside
a call's window is f16 NaN, every row a writer must not touch keeps a sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import BAR_REL, DEV, ROPE_BASE, P, bar_figures, decode_status, dev, gpu, lib, nans, within_bar  # noqa: F401
from tests.test_gpu_kv16 import SENTINEL, block_call, split_call, want_of, write

pytestmark = pytest.mark.gpu
SHAPES = [(8, 2, 128), (4, 4, 64), (8, 1, 256)]          # (numHeads, numHeadsKV, headDim)


def lo_of(pos, window):
    return max(0, pos + 1 - window)


def ring_of(rows, first, ringRows):
    """A ring that holds ``rows`` [n][nkv][hd] (float16), the tokens first .. first + n - 1, and NaN in every other row."""
    ring = torch.full((ringRows,) + rows.shape[1:], float("nan"), dtype=torch.float16, device=DEV)
    ring[[t % ringRows for t in range(first, first + len(rows))]] = dev(rows)
    return ring


def halves(rng, n, nkv, hd):
    return rng.standard_normal((n, nkv, hd), dtype=np.float32).astype(np.float16)


# ---------------------------------------------------------------- 1. the writers, bit for bit
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_ring_writers_store_the_f16_writers_halves_at_the_ring_row(gpu, nh, nkv, hd):
    ringRows, rng, rope = 96, np.random.default_rng([81, nh, nkv, hd]), C.c_float(ROPE_BASE)
    for where in (0, 95, 96, 2 * 96 + 5, (0, 64), (93, 17), (96 * 3 - 1, 2), "past"):
        token = not isinstance(where, tuple)
        rows = 1 if token else where[1]
        xs = [dev(rng.standard_normal((rows, n * hd), dtype=np.float32)) for n in (nh, nkv, nkv)]
        q, (kr, vr) = nans(rows, nh * hd), (torch.full((ringRows, nkv, hd), SENTINEL, dtype=torch.int16, device=DEV) for _ in "kv")
        if token:
            pos, maxPos = (50, 50) if where == "past" else (where, 1 << 20)
            posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
            gpu.check(lib().effort_rope_kv_ring(gpu.ctx, *(P(x) for x in xs), P(q), P(kr), P(vr), P(posd), nh, nkv, hd, ringRows, maxPos, rope), "rope_kv_ring")
        else:
            pos = where[0]
            gpu.check(lib().effort_rope_kv_rows_ring(gpu.ctx, *(P(x) for x in xs), P(q), P(kr), P(vr), *where, nh, nkv, hd, ringRows, rope), "rope_kv_rows_ring")
        gpu.eval()
        if where == "past":                                                       # *pos = maxPos: nothing written, status bit 0
            assert decode_status(gpu) == 1 and bool(torch.isnan(q).all()) and bool((kr == SENTINEL).all()) and bool((vr == SENTINEL).all())
            continue
        q16, k16, v16 = write(gpu, True, xs, where, nh, nkv, hd, 96 * 3 + 8)      # the f16 writers: token t in row t
        assert torch.equal(q.view(torch.int32), q16.view(torch.int32)), (where, "q_out")
        for ring, cache in ((kr, k16), (vr, v16)):
            want = torch.full_like(ring, SENTINEL)
            for t in range(pos, pos + rows):
                want[t % ringRows] = cache[t]
            assert torch.equal(ring, want), (where, "a stored half differs, or a row outside the block was written")
        assert decode_status(gpu) == 0


# ---------------------------------------------------------------- 2. / 3. the windowed split attention
def window_call(gpu, q, K, V, pos, ringRows, window, nh, splits, want):
    """The call at ``pos`` on rings that hold K / V, the tokens lo(pos) .. pos, and NaN elsewhere; held to the bar, returns out."""
    nkv, hd = K.shape[1], K.shape[2]
    kr, vr = (ring_of(x, lo_of(pos, window), ringRows) for x in (K, V))
    S = splits or lib().effort_attention_window_default_splits(gpu.ctx, nkv, window)
    scratch, out = nans(lib().effort_attention_split_scratch_bytes(nh, hd, S) // 4 + 8), nans(nh * hd + 8)
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    gpu.check(lib().effort_attention_window(gpu.ctx, P(dev(q)), P(kr), P(vr), P(posd), P(out), P(scratch), nh, nkv, hd, ringRows, window, splits),
              "attention_window")
    gpu.eval()
    assert bool(torch.isnan(out[nh * hd:]).all()) and bool(torch.isnan(scratch[-8:]).all()), "wrote past out or the scratch"
    got = out[:nh * hd].cpu().numpy()
    assert np.isfinite(got).all(), (pos, splits, "a NaN reached the output: a row outside the window, or a masked key multiplied in")
    assert within_bar(got, want), (pos, splits, bar_figures(got, want))
    return out[:nh * hd]


@pytest.mark.parametrize("ringRows", (130, 193))
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_window_attention_matches_float64(gpu, nh, nkv, hd, ringRows):
    window, rng, worst = 130, np.random.default_rng([82, nh, nkv, hd, ringRows]), 0.0
    q = rng.standard_normal(nh * hd, dtype=np.float32)
    for pos in (0, 63, 64, 129, 130, 131, 191, 192, 193, 259, 386, 100000):
        n = pos + 1 - lo_of(pos, window)
        K, V = halves(rng, n, nkv, hd), halves(rng, n, nkv, hd)
        want = want_of(q, K, V, nh)
        for S in (1, 3, 0):
            out, again = (window_call(gpu, q, K, V, pos, ringRows, window, nh, S, want) for _ in range(2))
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (pos, S, "not repeatable")
            worst = max(worst, bar_figures(out.cpu().numpy(), want)[0])
    print(f"attention_window headDim {hd} heads {nh}/{nkv} ring {ringRows}: worst error over the bar {worst / BAR_REL:.3g}")


@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_below_the_window_the_bits_are_the_f16_kernels(gpu, nh, nkv, hd):
    window, ringRows, rng = 130, 193, np.random.default_rng([83, nh, nkv, hd])
    K, V = halves(rng, 130, nkv, hd), halves(rng, 130, nkv, hd)
    for pos in (0, 65, 129):
        q = rng.standard_normal(nh * hd, dtype=np.float32)
        want = want_of(q, K[:pos + 1], V[:pos + 1], nh)
        for S in (1, 3):
            plain = split_call(gpu, q, K[:pos + 1], V[:pos + 1], 256, nh, S, want)[0]
            ours = window_call(gpu, q, K[:pos + 1], V[:pos + 1], pos, ringRows, window, nh, S, want)
            assert torch.equal(ours.view(torch.int32), plain.view(torch.int32)), (pos, S)
    for rows in (1, 17, 64):
        pos0 = 40                                                                 # pos0 + rows <= window: no key is masked
        q = rng.standard_normal((rows, nh * hd), dtype=np.float32)
        plain = block_call(gpu, q, K[:pos0 + rows], V[:pos0 + rows], pos0, nh)[0]
        ours = block_window_call(gpu, q, K[:pos0 + rows], V[:pos0 + rows], 0, pos0, nh, ringRows, window)
        assert torch.equal(ours.view(torch.int32), plain.view(torch.int32)), rows


# ---------------------------------------------------------------- 4. the windowed block attention against float64
def block_window_call(gpu, q, K, V, first, pos0, nh, ringRows, window):
    """The call for the block q [rows][nh * hd] at pos0 on rings that hold K / V, the tokens first .. pos0 + rows - 1; NaN in every other
    ring row and q row.  Every row is held to the bar against float64 over its own window; returns out [rows][nh * hd]."""
    rows, nkv, hd = len(q), K.shape[1], K.shape[2]
    assert first + len(K) == pos0 + rows and first <= lo_of(pos0, window)
    kr, vr = (ring_of(x, first, ringRows) for x in (K, V))
    qd, out = nans(64, nh * hd), nans(rows * nh * hd + 8)
    qd[:rows] = dev(q)
    gpu.check(lib().effort_attention_block_window(gpu.ctx, P(qd), P(kr), P(vr), pos0, rows, P(out), nh, nkv, hd, ringRows, window), "attention_block_window")
    gpu.eval()
    assert bool(torch.isnan(out[rows * nh * hd:]).all()), "wrote past out[rows]"
    got = out[:rows * nh * hd].view(rows, nh * hd).cpu().numpy()
    assert np.isfinite(got).all(), "a NaN reached a result: a row outside the window, or a masked key multiplied in"
    for r in range(rows):
        a, b = lo_of(pos0 + r, window) - first, pos0 + r + 1 - first
        want = want_of(q[r], K[a:b], V[a:b], nh)
        assert within_bar(got[r], want), (pos0, rows, r, bar_figures(got[r], want))
    return out[:rows * nh * hd].view(rows, nh * hd)


@pytest.mark.parametrize("pos0", (0, 35, 41, 3 * 103 - 7))
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_block_window_attention_matches_float64(gpu, nh, nkv, hd, pos0):
    window, ringRows, rng = 40, 103, np.random.default_rng([84, nh, nkv, hd, pos0])
    for rows in (1, 17, 64):
        first = lo_of(pos0, window)
        K, V = halves(rng, pos0 + rows - first, nkv, hd), halves(rng, pos0 + rows - first, nkv, hd)
        q = rng.standard_normal((rows, nh * hd), dtype=np.float32)
        whole = block_window_call(gpu, q, K, V, first, pos0, nh, ringRows, window)
        for r0 in range(0, rows if rows == 64 else 0, 16):                        # the same rows sent as 4 x 16: equal bits
            f = lo_of(pos0 + r0, window)
            part = block_window_call(gpu, q[r0:r0 + 16], K[f - first:pos0 + r0 + 16 - first], V[f - first:pos0 + r0 + 16 - first], f, pos0 + r0, nh,
                                     ringRows, window)
            assert torch.equal(part.view(torch.int32), whole[r0:r0 + 16].view(torch.int32)), (pos0, r0)


# ---------------------------------------------------------------- 5. through the Decoder
def test_decoder_with_a_window(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    cfg, window, last = small_model.cfg, 24, 150
    tokens = [int(t) for t in np.random.default_rng([85]).integers(0, 512, last + 1)]
    win, plain = Decoder(small_model, maxTokens=200, kv_cache="f16", window=window), Decoder(small_model, maxTokens=200, kv_cache="f16")
    assert tuple(win.kCache[0].shape) == (88, cfg.numHeadsKV, cfg.headDim) and win.kCache[0].dtype == torch.float16
    for d in (win, plain):                                                        # the ring wraps under the block writer, then under the token writer
        d.prefill(tokens[:100], chunk=64, attention="block")
        for t in tokens[100:]:
            d.tokId.fill_(t)
            d.token_step(dense=True)
        assert d.status() == 0
    held = list(range(last + 1 - 88, last + 1))                                   # the tokens the ring holds
    for ring, cache in ((win.kCache[0], plain.kCache[0]), (win.vCache[0], plain.vCache[0])):
        assert torch.equal(ring[[t % 88 for t in held]].view(torch.int16), cache[held].view(torch.int16)), "a layer-0 ring row differs from the plain cache's"
    seen = [t % 88 for t in range(last + 1 - window, last + 1)]                   # the last step's window, in token order
    K, V = (c[-1][seen].cpu().numpy() for c in (win.kCache, win.vCache))
    got, want = win.attnOutput.cpu().numpy(), want_of(win.xq.cpu().numpy(), K, V, cfg.numHeads)
    assert within_bar(got, want), bar_figures(got, want)
    runs = [Decoder(small_model, maxTokens=200, **kw).run(tokens[:40], 60, dense=True, collect_logits=True, prefill=True, prefill_chunk=16,
                                                          prefill_attention="block") for kw in (dict(kv_cache="f16", window=256), dict(kv_cache="f16"))]
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][2].view(torch.int32), runs[1][2].view(torch.int32)), "a window no key leaves changed the bits"
    for bad in (dict(window=24), dict(kv_cache="f32", window=24), dict(kv_cache="f16", window=0), dict(kv_cache="f16", window=32768, maxTokens=40000)):
        with pytest.raises(ValueError):
            Decoder(small_model, **dict(dict(maxTokens=64), **bad))
