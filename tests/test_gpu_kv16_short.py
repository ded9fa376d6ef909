"""effort_rope_attention_f16 (effort_amd/csrc/kv16_short.hip, ``Decoder(kv_cache="f16", short_attention_below=P)``): the one-launch token
step over the compact f16 KV cache.  The row it writes is held to effort_rope_kv_f16's bits, its output to the float64 reference over
the halves the caches hold AFTER the call, at effort_attention_split_f16's bar; every row it must not touch keeps a sentinel NaN."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import BAR_REL, DEV, ROPE_BASE, P, bar_figures, decode_status, dev, gpu, lib, nans, within_bar  # noqa: F401
from tests.test_gpu_kv16 import SENTINEL, want_of

pytestmark = pytest.mark.gpu
ROWS, MAX_KEYS = 600, 520


def short_call(gpu, xs, kc, vc, pos, nh, nkv, hd):
    out, posd = nans(nh * hd + 8), torch.tensor([pos], dtype=torch.int32, device=DEV)
    gpu.check(lib().effort_rope_attention_f16(gpu.ctx, *(P(x) for x in xs), P(kc), P(vc), P(posd), P(out), nh, nkv, hd, ROWS, MAX_KEYS,
                                              C.c_float(ROPE_BASE)), "rope_attention_f16")
    gpu.eval()
    assert bool(torch.isnan(out[nh * hd:]).all()), "wrote past out"
    return out[:nh * hd]


def step(gpu, rng, K, V, pos, nh, nkv, hd, big=False):
    """One call at ``pos`` on caches holding K / V rows < pos and the sentinel from row pos on.  Checks the written row against
    effort_rope_kv_f16's and every other row against what it held; returns (out, want) over the caches after the call."""
    xq, xk, xv = (rng.standard_normal(n * hd, dtype=np.float32) for n in (nh, nkv, nkv))
    if big:
        xk[hd // 2 - 1] = xv[3] = 7e4                                           # past the largest half: +inf is stored (k: the slowest rope pair)
    xs, before = [dev(x) for x in (xq, xk, xv)], []
    for c in (K, V):
        before.append(torch.full((ROWS, nkv, hd), SENTINEL, dtype=torch.int16, device=DEV))
        before[-1][:pos] = dev(c[:pos]).view(torch.int16)
    kc, vc = (c.clone() for c in before)
    out = short_call(gpu, xs, kc, vc, pos, nh, nkv, hd)
    q, k2, v2 = nans(nh * hd), before[0].clone(), before[1].clone()              # the two-launch writer on a second pair: the row's bits, and q
    posd = torch.tensor([pos], dtype=torch.int32, device=DEV)
    gpu.check(lib().effort_rope_kv_f16(gpu.ctx, *(P(x) for x in xs), P(q), P(k2), P(v2), P(posd), nh, nkv, hd, ROWS, C.c_float(ROPE_BASE)), "rope_kv_f16")
    gpu.eval()
    assert torch.equal(kc, k2) and torch.equal(vc, v2), (pos, "row pos differs from effort_rope_kv_f16's, or another row was written")
    assert not bool((kc[pos] == SENTINEL).any()) and bool((kc[pos + 1:] == SENTINEL).all())
    again = short_call(gpu, xs, kc, vc, pos, nh, nkv, hd)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (pos, "not repeatable")
    Kh, Vh = (c[:pos + 1].view(torch.float16).cpu().numpy() for c in (kc, vc))
    if big:
        return out.cpu().numpy(), Kh, Vh
    return out.cpu().numpy(), want_of(q.cpu().numpy(), Kh, Vh, nh)


@pytest.mark.parametrize("nh,nkv", [(8, 2), (4, 4), (8, 1), (4, 2)])
@pytest.mark.parametrize("hd", (64, 128, 256))
def test_short_attention_f16_matches_float64(gpu, hd, nh, nkv):
    rng, kpp, worst = np.random.default_rng([91, hd, nh, nkv]), 2048 // hd, 0.0
    K, V = (rng.standard_normal((MAX_KEYS, nkv, hd), dtype=np.float32).astype(np.float16) for _ in "kv")
    # a pass edge, the batch asked for before the rotation, a whole batch of passes, the softmax's stride, the last legal position
    for pos in sorted({0, 1, kpp - 1, kpp, 4 * kpp - 1, 4 * kpp, 4 * kpp + 1, 8 * kpp - 1, 8 * kpp, 8 * kpp + 1, 255, 256, 257, MAX_KEYS - 1}):
        got, want = step(gpu, rng, K, V, pos, nh, nkv, hd)
        assert np.isfinite(got).all(), (pos, "a NaN reached the output: the row being written, or a row past pos")
        assert within_bar(got, want), (pos, bar_figures(got, want))
        worst = max(worst, bar_figures(got, want)[0])
    print(f"rope_attention_f16 headDim {hd} heads {nh}/{nkv}: worst error over the bar {worst / BAR_REL:.3g}")
    got, Kh, Vh = step(gpu, rng, K, V, 4 * kpp, nh, nkv, hd, big=True)
    assert np.isinf(Kh[-1]).any() and np.isinf(Vh[-1]).any() and not np.isfinite(got).all()
    assert decode_status(gpu) == 0


def test_short_attention_f16_past_its_limit_writes_nothing(gpu):
    nh, nkv, hd = 8, 2, 128
    xs = [dev(np.ones(n * hd, dtype=np.float32)) for n in (nh, nkv, nkv)]
    kc, vc = (torch.full((ROWS, nkv, hd), SENTINEL, dtype=torch.int16, device=DEV) for _ in "kv")
    out = short_call(gpu, xs, kc, vc, MAX_KEYS, nh, nkv, hd)
    assert bool(torch.isnan(out).all()) and bool((kc == SENTINEL).all()) and bool((vc == SENTINEL).all())
    assert decode_status(gpu) == 1


@pytest.mark.parametrize("window", (None, 48))
@pytest.mark.parametrize("how", (dict(dense=True), dict(effort=1.0)))
def test_decoder_with_short_attention(small_model, how, window):  # noqa: F811
    """Teacher-forced, 64 steps, at the settings the project's 2e-3 is defined for: the dense path and effort 1.0 (at effort 0.25 the
    multiply's row selection is discontinuous in its input: no attention path is within 2e-3 of another, tests/test_gpu_attention_split.py)."""
    from effort_amd.decode import Decoder
    ids = [int(t) for t in np.random.default_rng([92]).integers(0, 512, 64)]
    plain, short = (Decoder(small_model, maxTokens=96, kv_cache="f16", window=window, **opt) for opt in ({}, dict(short_attention_below=40)))
    want, got = (d.run(ids, 64, forced=True, collect_logits=True, **how)[2] for d in (plain, short))
    err = float(((got - want).abs().amax(1) / want.abs().amax(1)).max())
    print(f"short_attention_below=40, window {window}, {how}: logits within {err:.3g} of max|logit| of the decoder without it")
    assert err <= 2e-3, err
    assert torch.equal(short.kCache[0].view(torch.int16), plain.kCache[0].view(torch.int16))
    assert torch.equal(short.vCache[0].view(torch.int16), plain.vCache[0].view(torch.int16))
    assert short.status() == 0
    assert len(plain._graphs) == 1 and len(short._graphs) == 2 and sum("short" in key for key in short._graphs) == 1


def test_decoder_refuses_a_short_attention_it_cannot_serve(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    for bad in (dict(kv_cache="f32"), dict(short_attention_below=0), dict(maxTokens=4096, short_attention_below=2049), dict(window=39)):
        with pytest.raises(ValueError):
            Decoder(small_model, **dict(dict(maxTokens=96, kv_cache="f16", short_attention_below=40), **bad))
    with pytest.raises(ValueError):
        Decoder(small_model, maxTokens=96, kv_cache="f16").token_step(short=True)
