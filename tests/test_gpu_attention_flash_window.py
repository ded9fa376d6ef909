"""effort_attention_flash_window (effort_amd/csrc/attention_flash_window.hip, ``Decoder.prefill(attention="flash_window")``): the block
attention over the ROLLING f16 cache with a sliding window, both products on the f16 MFMA.  Held to float64 (``glue_reference.attention``
over the halves the ring holds for each query's window) at the project's UNCHANGED f32 bar ``within_bar``, to the bits of
effort_attention_flash_f16 while the window is not reached, and to its own bits across blocks and ring sizes; every ring row outside the
call's tokens and every q row past the block is NaN."""
import numpy as np
import pytest
import torch

from tests.test_gpu_attention_flash import flash_call, marker_rows
from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import BAR_REL, P, bar_figures, dev, gpu, lib, nans, within_bar  # noqa: F401
from tests.test_gpu_kv16 import want_of
from tests.test_gpu_kv_window import SHAPES, halves, lo_of, ring_of

pytestmark = pytest.mark.gpu


def flash_window_call(gpu, q, K, V, pos0, nh, ringRows, window):
    """The call for the block q [rows][nh * hd] at pos0 on rings that hold K / V, the tokens lo(pos0) .. pos0 + rows - 1, and NaN in every
    other ring row and q row.  Every row is held to the bar against float64 over its own window.  Returns (out [rows][nh * hd], worst
    error / max|want| over the rows)."""
    rows, nkv, hd, first = len(q), K.shape[1], K.shape[2], lo_of(pos0, window)
    assert first + len(K) == pos0 + rows == first + len(V)
    kr, vr = (ring_of(x, first, ringRows) for x in (K, V))
    qd, out = nans(64, nh * hd), nans(rows * nh * hd + 8)
    qd[:rows] = dev(q)
    gpu.check(lib().effort_attention_flash_window(gpu.ctx, P(qd), P(kr), P(vr), pos0, rows, P(out), nh, nkv, hd, ringRows, window), "attention_flash_window")
    gpu.eval()
    assert bool(torch.isnan(out[rows * nh * hd:]).all()), "wrote past out[rows]"
    got, worst = out[:rows * nh * hd].view(rows, nh * hd).cpu().numpy(), 0.0
    assert np.isfinite(got).all(), "a NaN reached a result: a row outside the window, or a masked key multiplied in"
    for r in range(rows):
        a, b = lo_of(pos0 + r, window) - first, pos0 + r + 1 - first
        want = want_of(q[r], K[a:b], V[a:b], nh)
        assert within_bar(got[r], want), (pos0, rows, r, bar_figures(got[r], want))
        worst = max(worst, bar_figures(got[r], want)[0])
    return out[:rows * nh * hd].view(rows, nh * hd), worst


# ---------------------------------------------------------------- 1. against float64
# window 70 is no multiple of the 32-key tile; ring 133 = window + 63 is the least legal one for 64 rows (the wrap falls inside a tile), 160
# is tile-aligned.  pos0 0, 27: below the window; 50: the block straddles its edge; 120: the ring wraps inside the block; 300: the walk
# starts on a wave other than 0; 100000: far past.  q x 2^6 where the plain kernel sits closest to the bar.
@pytest.mark.parametrize("pos0", (0, 27, 50, 120, 300, 100000))
@pytest.mark.parametrize("rows", (1, 17, 64))
@pytest.mark.parametrize("ringRows", (133, 160))
@pytest.mark.parametrize("nh,nkv,hd,mag", [s + (1.0,) for s in SHAPES] + [(8, 2, 128, 2.0 ** 6)])
def test_flash_window_attention_matches_float64(gpu, nh, nkv, hd, mag, ringRows, rows, pos0):
    window, rng = 70, np.random.default_rng([101, nh, nkv, hd, ringRows, rows, pos0])
    n = pos0 + rows - lo_of(pos0, window)
    K, V = halves(rng, n, nkv, hd), halves(rng, n, nkv, hd)
    q = rng.standard_normal((rows, nh * hd), dtype=np.float32) * np.float32(mag)
    worst = flash_window_call(gpu, q, K, V, pos0, nh, ringRows, window)[1]
    print(f"attention_flash_window headDim {hd} heads {nh}/{nkv} ring {ringRows} pos0 {pos0} rows {rows} q x {mag:g}: worst error over the bar {worst / BAR_REL:.3g}")


# ---------------------------------------------------------------- 2. the window not yet reached: the plain kernel's bits
@pytest.mark.parametrize("pos0,rows", [(0, 64), (37, 17), (66, 64)])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_below_the_window_the_bits_are_the_plain_flash_kernels(gpu, nh, nkv, hd, pos0, rows):
    window, ringRows, rng = 130, 193, np.random.default_rng([102, nh, nkv, hd, pos0])
    K, V = halves(rng, pos0 + rows, nkv, hd), halves(rng, pos0 + rows, nkv, hd)
    q = rng.standard_normal((rows, nh * hd), dtype=np.float32)
    plain = flash_call(gpu, q, K, V, pos0, nh)[0]
    ours = flash_window_call(gpu, q, K, V, pos0, nh, ringRows, window)[0]
    assert torch.equal(ours.view(torch.int32), plain.view(torch.int32))


# ---------------------------------------------------------------- 3. the lower edge
@pytest.mark.parametrize("hd", (64, 128, 256))
def test_flash_window_masks_the_key_below_each_querys_bound(gpu, hd):
    """The ring row of token lo(pos0 + r) - 1 -- the newest key query r may NO LONGER see -- is c * q[r], its score with query r 40 (for
    r = 0 that row is the block's last token's, which query 0 may not see either); V row of token t is t + 1 - lo(pos0).  A query that
    sees one key below its bound moves by O(1).  The 64 marked tokens are consecutive: every place of a 32-key tile is a boundary."""
    nh, window, ringRows, pos0, rows, rng = 4, 70, 133, 200, 64, np.random.default_rng([103, hd])
    n = pos0 + rows - lo_of(pos0, window)                                         # 133: the ring is full
    q, K = rng.standard_normal((rows, nh * hd), dtype=np.float32), halves(rng, n, nh, hd)
    mark = marker_rows(q, nh, hd)
    K[:rows - 1], K[n - 1] = mark[1:], mark[0]                                    # token lo(pos0) - 1 + r, r = 1 .. 63; token pos0 + 63 in token pos0 - window's row
    V = np.broadcast_to(np.arange(1, n + 1, dtype=np.float16)[:, None, None], K.shape).copy()
    flash_window_call(gpu, q, K, V, pos0, nh, ringRows, window)


# ---------------------------------------------------------------- 4. a row depends neither on its block nor on the ring's size, bit for bit
def test_flash_window_row_does_not_depend_on_its_block_or_ring(gpu):
    nh, nkv, hd, window, first, rng = 8, 2, 128, 70, 237, np.random.default_rng([104])
    base = lo_of(first, window)                                                   # K / V row i: token base + i
    K, V = halves(rng, first + 64 - base, nkv, hd), halves(rng, first + 64 - base, nkv, hd)
    q = rng.standard_normal((64, nh * hd), dtype=np.float32)                      # row r: the query at absolute position 237 + r
    whole = flash_window_call(gpu, q, K, V, first, nh, 133, window)[0].view(torch.int32)
    for i, (r0, rows) in enumerate([(0, 16), (16, 16), (32, 16), (48, 16), (20, 17), (0, 1), (26, 1), (63, 1)]):
        a, b = lo_of(first + r0, window) - base, first + r0 + rows - base
        part = flash_window_call(gpu, q[r0:r0 + rows], K[a:b], V[a:b], first + r0, nh, (133, 160)[i % 2], window)[0].view(torch.int32)
        assert torch.equal(part, whole[r0:r0 + rows]), (r0, rows)


# ---------------------------------------------------------------- 5. through the Decoder
def test_decoder_prefill_with_flash_window_attention(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    prompt, kw, runs = [int(t) for t in np.random.default_rng([105]).integers(0, 512, 90)], dict(maxTokens=128, kv_cache="f16", window=24), {}
    for attention in ("block", "flash_window"):
        dec = Decoder(small_model, **kw)
        logits = dec.run(prompt, len(prompt), dense=True, collect_logits=True, prefill=True, prefill_attention=attention)[2]
        runs[attention] = (logits, [c.float() for c in dec.kCache + dec.vCache])  # 90 tokens through 88 ring rows: every row is live
    (lb, cb), (lf, cf) = runs["block"], runs["flash_window"]
    err = float((lf - lb).abs().max() / lb.abs().max())
    cerr = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(cf, cb))
    print(f"prefill attention='flash_window' against 'block': logits within {err:.3g} of max|logit|, rings within {cerr:.3g} of their max")
    assert err < 2e-3 and cerr < 2e-3, (err, cerr)
    two, got = Decoder(small_model, **kw), []
    for chunk in (64, 16):
        for c in two.kCache + two.vCache:
            c.fill_(float("nan"))
        two.prefill(prompt, chunk=chunk, attention="flash_window")
        got.append([c.clone().view(torch.int16) for c in two.kCache + two.vCache])
    assert all(torch.equal(a, b) for a, b in zip(*got)) and all(bool(torch.isfinite(c).all()) for c in two.kCache + two.vCache)
    for refused in (Decoder(small_model, maxTokens=128), Decoder(small_model, maxTokens=128, kv_cache="f16")):
        with pytest.raises(ValueError, match="flash_window"):
            refused.prefill(prompt[:40], attention="flash_window")
