"""effort_attention_flash_f16 (effort_amd/csrc/attention_flash16.hip, ``Decoder.prefill(attention="flash")``): the block attention over
the compact f16 cache with both products on the f16 MFMA, q and the probabilities split into two halves each.  Held to float64
(``glue_reference.attention`` over the halves the cache holds) at the project's UNCHANGED f32 bar ``within_bar``; every cache row and q
row the kernel must not read is NaN."""
import numpy as np
import pytest
import torch

from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import BAR_REL, DEV, P, bar_figures, dev, gpu, lib, nans, within_bar  # noqa: F401
from tests.test_gpu_kv16 import want_of

pytestmark = pytest.mark.gpu


def flash_call(gpu, q, K, V, pos0, nh, check=True):
    """The call for the block q [rows][nh * hd] at pos0 on caches that hold K / V [pos0 + rows][nkv][hd] (float16) and NaN in every other
    cache row and q row.  Returns (out [rows][nh * hd], worst error / max|want| over the rows held to the bar against float64)."""
    rows, nkv, hd, maxTokens, caches = len(q), K.shape[1], K.shape[2], (len(K) + 63) // 64 * 64, []
    assert len(K) == pos0 + rows
    for c in (K, V):
        caches.append(torch.full((maxTokens, nkv, hd), float("nan"), dtype=torch.float16, device=DEV))
        caches[-1][:len(c)] = dev(c)
    qd, out = nans(64, nh * hd), nans(rows * nh * hd + 8)
    qd[:rows] = dev(q)
    gpu.check(lib().effort_attention_flash_f16(gpu.ctx, P(qd), P(caches[0]), P(caches[1]), pos0, rows, P(out), nh, nkv, hd, maxTokens), "attention_flash_f16")
    gpu.eval()
    assert bool(torch.isnan(out[rows * nh * hd:]).all()), "wrote past out[rows]"
    got, worst = out[:rows * nh * hd].view(rows, nh * hd).cpu().numpy(), 0.0
    assert np.isfinite(got).all(), "a NaN reached a result: a row that must not be read, or a masked key multiplied in"
    for r in range(rows if check else 0):
        want = want_of(q[r], K[:pos0 + r + 1], V[:pos0 + r + 1], nh)
        assert within_bar(got[r], want), (pos0, rows, r, bar_figures(got[r], want))
        worst = max(worst, bar_figures(got[r], want)[0])
    return out[:rows * nh * hd].view(rows, nh * hd), worst


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("mag", (2.0 ** -6, 1.0, 2.0 ** 6))                       # the per-row exponent of q's pre-scale
@pytest.mark.parametrize("rows", (1, 16, 17, 64))
@pytest.mark.parametrize("pos0", (0, 5, 27, 120, 300))                            # unaligned; across a 32-key tile edge; across the waves' 128-key round
@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 64), (8, 2, 128), (8, 1, 256), (4, 4, 128)])
def test_flash_attention_matches_float64(gpu, nh, nkv, hd, pos0, rows, mag):
    rng = np.random.default_rng([91, nh, nkv, hd, pos0, rows])
    K, V = (rng.standard_normal((pos0 + rows, nkv, hd), dtype=np.float32).astype(np.float16) for _ in "kv")
    q = rng.standard_normal((rows, nh * hd), dtype=np.float32) * np.float32(mag)
    worst = flash_call(gpu, q, K, V, pos0, nh)[1]
    print(f"attention_flash_f16 headDim {hd} heads {nh}/{nkv} pos0 {pos0} rows {rows} q x {mag:g}: worst error over the bar {worst / BAR_REL:.3g}")


# ---------------------------------------------------------------- 2. markers
def marker_rows(q, nh, hd):
    """c * q[r] per head, f16: a key row whose score with query r is 40 in every head (nh == nkv)."""
    qh = q.reshape(len(q), nh, hd).astype(np.float64)
    return (qh * (40.0 * np.sqrt(hd) / (qh ** 2).sum(axis=2))[:, :, None]).astype(np.float16)


@pytest.mark.parametrize("hd", (64, 128, 256))
@pytest.mark.parametrize("pos0,rows", [(0, 64), (27, 17), (120, 64)])
def test_flash_attention_is_causal_inside_the_block(gpu, hd, pos0, rows):
    """Cache row pos0 + r + 1 -- the first key query r may NOT see -- is c * q[r], its score with query r 40; V row t is t + 1.  A query
    that sees one future key moves by O(1)."""
    nh, rng = 4, np.random.default_rng([92, hd, pos0, rows])
    q, K = rng.standard_normal((rows, nh * hd), dtype=np.float32), rng.standard_normal((pos0 + rows, nh, hd), dtype=np.float32).astype(np.float16)
    K[pos0 + 1:pos0 + rows] = marker_rows(q, nh, hd)[:rows - 1]
    V = np.broadcast_to(np.arange(1, pos0 + rows + 1, dtype=np.float16)[:, None, None], K.shape).copy()
    flash_call(gpu, q, K, V, pos0, nh)


@pytest.mark.parametrize("hd", (64, 128, 256))
def test_flash_attention_weighs_one_key_at_every_place_of_a_tile(gpu, hd):
    """Query r (position 64 + r) finds c * q[r] in cache row 32 + r: the 32 places of key tile 1 -- each of a lane's eight keys, both
    halves of the tile -- carry one query's whole weight each; V row t is t + 1, so out[r] must be 33 + r in every d.  A wrong
    transposed read or row assignment moves an element by O(1)."""
    nh, pos0, rows, rng = 4, 64, 32, np.random.default_rng([93, hd])
    q, K = rng.standard_normal((rows, nh * hd), dtype=np.float32), rng.standard_normal((pos0 + rows, nh, hd), dtype=np.float32).astype(np.float16)
    K[32:64] = marker_rows(q, nh, hd)
    V = np.broadcast_to(np.arange(1, pos0 + rows + 1, dtype=np.float16)[:, None, None], K.shape).copy()
    got = flash_call(gpu, q, K, V, pos0, nh)[0].cpu().numpy()
    assert abs(got - np.arange(33, 65)[:, None]).max() < 1e-2, "a query's weight landed on another V row"
    # ... and with V row t = one-hot-like in d (V[t][d] = d + 1 at the marked keys), an element that changes its d shows
    V[32:64] = np.arange(1, hd + 1, dtype=np.float16)[None, None, :]
    got = flash_call(gpu, q, K, V, pos0, nh)[0].view(rows, nh, hd).cpu().numpy()
    assert abs(got - np.arange(1, hd + 1)[None, None, :]).max() < 1e-2 * hd / 64, "an output element landed on another d"


# ---------------------------------------------------------------- 3. a row does not depend on its block, bit for bit
def test_flash_row_does_not_depend_on_its_block(gpu):
    nh, nkv, hd, first, rng = 8, 2, 128, 37, np.random.default_rng([94])
    K, V = (rng.standard_normal((first + 64, nkv, hd), dtype=np.float32).astype(np.float16) for _ in "kv")
    q = rng.standard_normal((64, nh * hd), dtype=np.float32)                      # row r: the query at absolute position 37 + r
    part = lambda r0, rows: flash_call(gpu, q[r0:r0 + rows], K[:first + r0 + rows], V[:first + r0 + rows], first + r0, nh, check=False)[0].view(torch.int32)  # noqa: E731
    whole = flash_call(gpu, q, K, V, first, nh)[0].view(torch.int32)
    for r0, rows in [(r0, 16) for r0 in range(0, 64, 16)] + [(20, 17)] + [(r0, 1) for r0 in (0, 5, 26, 27, 58, 63)]:
        assert torch.equal(part(r0, rows), whole[r0:r0 + rows]), (r0, rows)


# ---------------------------------------------------------------- 4. through the Decoder
def test_decoder_prefill_with_flash_attention(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    prompt = [int(t) for t in np.random.default_rng([95]).integers(0, 512, 41)]
    runs = {}
    for attention in ("block", "flash"):
        dec = Decoder(small_model, maxTokens=64, kv_cache="f16")
        logits = dec.run(prompt, len(prompt), dense=True, collect_logits=True, prefill=True, prefill_attention=attention)[2]
        runs[attention] = (logits, [c[:40].float() for c in dec.kCache + dec.vCache])
    (lb, cb), (lf, cf) = runs["block"], runs["flash"]
    err = float((lf - lb).abs().max() / lb.abs().max())
    cerr = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(cf, cb))
    print(f"prefill attention='flash' against 'block': logits within {err:.3g} of max|logit|, caches within {cerr:.3g} of their max")
    assert err < 2e-3 and cerr < 2e-3, (err, cerr)
    two, got = Decoder(small_model, maxTokens=64, kv_cache="f16"), []
    for chunk in (64, 16):
        for c in two.kCache + two.vCache:
            c.fill_(float("nan"))
        two.prefill(prompt[:40], chunk=chunk, attention="flash")
        got.append([c[:40].clone().view(torch.int16) for c in two.kCache + two.vCache])
        assert all(bool(torch.isnan(c[40:]).all()) for c in two.kCache + two.vCache)
    assert all(torch.equal(a, b) for a, b in zip(*got)) and bool(torch.isfinite(two.kCache[1][:40]).all())
    for refused in (Decoder(small_model, maxTokens=64), Decoder(small_model, maxTokens=64, kv_cache="f16", window=24)):
        with pytest.raises(ValueError, match="flash"):
            refused.prefill(prompt[:40], attention="flash")
