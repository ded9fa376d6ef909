"""The compact f16 KV cache [maxTokens][numHeadsKV][headDim] (effort_amd/csrc/kv16.hip, the f16 instantiation of attention_block.hip,
``Decoder(kv_cache="f16")``).  The writers are held to the f32 writers' bits; both attentions to the float64 reference
``glue_reference.attention`` over the f16 values the cache HOLDS, at the project's f32 bar (``within_bar``: |got - want| <= 2e-5 *
max|want|, cos-sim >= 0.999999) -- the kernels' arithmetic is f32 on exactly representable inputs, so the bar applies unchanged.  Every
cache row a kernel must not read is f16 NaN, every row a writer must not touch keeps a sentinel."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_reference as ref
from tests.test_gpu_decode import small_model, torch_reference  # noqa: F401  (small_model: the fixture)
from tests.test_gpu_glue import BAR_REL, DEV, ROPE_BASE, P, bar_figures, decode_status, dev, gpu, lib, nans, within_bar  # noqa: F401

pytestmark = pytest.mark.gpu
SENTINEL = 0x7E55                                        # an f16 NaN no conversion produces


# ---------------------------------------------------------------- 1. the writers, bit for bit
def write(gpu, f16, xs, where, nh, nkv, hd, maxTokens):
    """One writer call on fresh caches.  ``where``: a position (token form) or (pos0, rows).  Returns (q_out, kCache, vCache)."""
    token = not isinstance(where, tuple)
    q = nans(1 if token else where[1], nh * hd)
    shape = (maxTokens, nkv, hd) if f16 else (maxTokens, nh, hd)
    kc, vc = (torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV) if f16 else nans(*shape) for _ in "kv")
    posd = torch.tensor([where if token else 0], dtype=torch.int32, device=DEV)
    name = "effort_rope_kv" + ("" if token else "_rows") + ("_f16" if f16 else "")
    gpu.check(getattr(lib(), name)(gpu.ctx, *(P(x) for x in xs), P(q), P(kc), P(vc), *((P(posd),) if token else where), nh, nkv, hd, maxTokens,
                                   C.c_float(ROPE_BASE)), name)
    gpu.eval()
    return q, kc, vc


@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 128), (4, 4, 64), (8, 1, 256)])
def test_writers_store_half_rn_of_the_f32_writers_values(gpu, nh, nkv, hd):
    maxTokens, rng = 96, np.random.default_rng([71, nh, nkv, hd])
    for where in (0, 1, 77, maxTokens - 1, maxTokens) + tuple((pos0, rows) for rows in (1, 17, 64) for pos0 in (0, 5)):
        rows = where[1] if isinstance(where, tuple) else 1
        xq, xk, xv = (rng.standard_normal((rows, n * hd), dtype=np.float32) for n in (nh, nkv, nkv))
        xk[0, hd // 2 - 1] = xv[0, 3] = 7e4                                       # past the largest half (k: the slowest rope pair, angle < 1e-4): +inf is stored
        xs = [dev(x) for x in (xq, xk, xv)]
        q16, k16, v16 = write(gpu, True, xs, where, nh, nkv, hd, maxTokens)
        if where == maxTokens:                                                    # a step past the cache: nothing written, status bit 0
            assert decode_status(gpu) == 1 and bool(torch.isnan(q16).all()) and bool((k16 == SENTINEL).all()) and bool((v16 == SENTINEL).all())
            continue
        q32, k32, v32 = write(gpu, False, xs, where, nh, nkv, hd, maxTokens)
        live = slice(where[0], where[0] + rows) if isinstance(where, tuple) else slice(where, where + 1)
        assert torch.equal(q16.view(torch.int32), q32.view(torch.int32)), (where, "q_out")
        for c16, c32 in ((k16, k32), (v16, v32)):
            want = torch.full_like(c16, SENTINEL)
            want[live] = c32[live, ::nh // nkv].half().view(torch.int16)
            assert torch.equal(c16, want), (where, "a stored half differs, or a row outside the block was written")
        assert bool(torch.isinf(k16[live].view(torch.float16)).any()) and bool(torch.isinf(v16[live].view(torch.float16)).any())
        assert decode_status(gpu) == 0


# ---------------------------------------------------------------- 2. / 3. the split decode attention against float64
def want_of(q, K, V, nh):
    rep = nh // K.shape[1]
    return ref.attention(q.reshape(nh, -1), np.repeat(K.astype(np.float64), rep, axis=1), np.repeat(V.astype(np.float64), rep, axis=1))


def split_call(gpu, q, K, V, maxTokens, nh, splits, want):
    """The call at position len(K) - 1 on caches that hold K / V [n][nkv][hd] (float16) and NaN in every other row, held to the bar
    against ``want``; returns (out, error / max|want|)."""
    nkv, hd, caches = K.shape[1], K.shape[2], []
    for rows in (K, V):
        caches.append(torch.full((maxTokens, nkv, hd), float("nan"), dtype=torch.float16, device=DEV))
        caches[-1][:len(rows)] = dev(rows)
    S = splits or lib().effort_attention_split_default_splits(gpu.ctx, nkv, maxTokens)
    scratch, out = nans(lib().effort_attention_split_scratch_bytes(nh, hd, S) // 4 + 8), nans(nh * hd + 8)
    posd = torch.tensor([len(K) - 1], dtype=torch.int32, device=DEV)
    gpu.check(lib().effort_attention_split_f16(gpu.ctx, P(dev(q)), P(caches[0]), P(caches[1]), P(posd), P(out), P(scratch), nh, nkv, hd, maxTokens, splits),
              "attention_split_f16")
    gpu.eval()
    assert bool(torch.isnan(out[nh * hd:]).all()) and bool(torch.isnan(scratch[-8:]).all()), "wrote past out or the scratch"
    got = out[:nh * hd].cpu().numpy()
    assert np.isfinite(got).all(), "a NaN reached the output: a row past pos, or a masked key multiplied in"
    assert within_bar(got, want), bar_figures(got, want)
    return out[:nh * hd], bar_figures(got, want)[0]


@pytest.mark.parametrize("nh,nkv", [(8, 2), (4, 4), (8, 1), (4, 2)])
@pytest.mark.parametrize("hd", (64, 128, 256))
def test_split_attention_f16_matches_float64(gpu, hd, nh, nkv):
    rng = np.random.default_rng([72, hd, nh, nkv])
    q, K, V = (rng.standard_normal(s, dtype=np.float32) for s in ((nh * hd,), (1031, nkv, hd), (1031, nkv, hd)))
    K, V, worst = K.astype(np.float16), V.astype(np.float16), 0.0               # drawn as f32, rounded to f16 by numpy
    for pos in (0, 1, 15, 63, 64, 65, 127, 128, 257, 1030):                       # a tile edge, a split edge, empty trailing splits
        want = want_of(q, K[:pos + 1], V[:pos + 1], nh)
        for S in (1, 3, 8, 0):
            (out, err), (again, _) = (split_call(gpu, q, K[:pos + 1], V[:pos + 1], 1100, nh, S, want) for _ in range(2))
            assert torch.equal(out.view(torch.int32), again.view(torch.int32)), (pos, S, "not repeatable")
            worst = max(worst, err)
    print(f"attention_split_f16 headDim {hd} heads {nh}/{nkv}: worst error over the bar {worst / BAR_REL:.3g}")


def test_split_attention_f16_at_the_cap(gpu):
    nh, nkv, hd, maxTokens = 8, 2, 128, 32768
    rng = np.random.default_rng([73])
    q, K, V = (rng.standard_normal(s, dtype=np.float32) for s in ((nh * hd,), (maxTokens, nkv, hd), (maxTokens, nkv, hd)))
    K, V = K.astype(np.float16), V.astype(np.float16)
    want = want_of(q, K, V, nh)
    for S in (0, 7, 64):
        split_call(gpu, q, K, V, maxTokens, nh, S, want)
    f = lib().effort_attention_split_f16
    assert f(None, None, None, None, None, None, None, nh, nkv, hd, maxTokens + 1, 0) == -2      # judged before the pointers
    assert f(None, None, None, None, None, None, None, nh, nkv, 96, maxTokens, 0) == -2


# ---------------------------------------------------------------- 4. the block attention against float64
def block_call(gpu, q, K, V, pos0, nh):
    """The call for the block q [rows][nh * hd] at pos0 on caches that hold K / V [pos0 + rows][nkv][hd] (float16); NaN in every other
    cache row and q row.  Every row is held to the bar against float64; returns (out [rows][nh * hd], worst error / max|want|)."""
    rows, nkv, hd, maxTokens, caches = len(q), K.shape[1], K.shape[2], (len(K) + 63) // 64 * 64, []
    for c in (K, V):
        caches.append(torch.full((maxTokens, nkv, hd), float("nan"), dtype=torch.float16, device=DEV))
        caches[-1][:len(c)] = dev(c)
    qd, out = nans(64, nh * hd), nans(rows * nh * hd + 8)
    qd[:rows] = dev(q)
    gpu.check(lib().effort_attention_block_f16(gpu.ctx, P(qd), P(caches[0]), P(caches[1]), pos0, rows, P(out), nh, nkv, hd, maxTokens), "attention_block_f16")
    gpu.eval()
    assert bool(torch.isnan(out[rows * nh * hd:]).all()), "wrote past out[rows]"
    got, worst = out[:rows * nh * hd].view(rows, nh * hd).cpu().numpy(), 0.0
    assert np.isfinite(got).all(), "a NaN reached a result: a row that must not be read, or a masked key multiplied in"
    for r in range(rows):
        want = want_of(q[r], K[:pos0 + r + 1], V[:pos0 + r + 1], nh)
        assert within_bar(got[r], want), (pos0, rows, r, bar_figures(got[r], want))
        worst = max(worst, bar_figures(got[r], want)[0])
    return out[:rows * nh * hd].view(rows, nh * hd), worst


@pytest.mark.parametrize("nh,nkv,hd", [(8, 2, 64), (8, 2, 128), (8, 2, 256), (4, 4, 128), (8, 1, 128)])
def test_block_attention_f16_matches_float64(gpu, nh, nkv, hd):
    rng, worst = np.random.default_rng([74, nh, nkv, hd]), 0.0
    K, V = (rng.standard_normal((1064, nkv, hd), dtype=np.float32).astype(np.float16) for _ in "kv")
    for pos0 in (0, 5, 1000):
        for rows in (1, 16, 17, 64):
            q = rng.standard_normal((rows, nh * hd), dtype=np.float32)
            worst = max(worst, block_call(gpu, q, K[:pos0 + rows], V[:pos0 + rows], pos0, nh)[1])
    print(f"attention_block_f16 headDim {hd} heads {nh}/{nkv}: worst error over the bar {worst / BAR_REL:.3g}")


def test_block_attention_f16_weighs_a_marker_key(gpu):
    """KV head g's row 3 + g is c * q of the LAST head of its group in the last query row (score 40), V row t is t + 1: that head answers
    4 + g, the other heads of the group -- other queries -- an ordinary mix.  A head reading another group's rows moves by O(1)."""
    nh, nkv, hd, pos0, rows = 8, 2, 128, 5, 17
    rng = np.random.default_rng([76])
    q, K = rng.standard_normal((rows, nh * hd), dtype=np.float32), rng.standard_normal((pos0 + rows, nkv, hd), dtype=np.float32).astype(np.float16)
    for g in range(nkv):
        qh = q[rows - 1].reshape(nh, hd)[g * (nh // nkv) + nh // nkv - 1].astype(np.float64)
        K[3 + g, g] = (qh * (40.0 * np.sqrt(hd) / (qh ** 2).sum())).astype(np.float16)
    V = np.broadcast_to(np.arange(1, pos0 + rows + 1, dtype=np.float16)[:, None, None], K.shape).copy()
    want = want_of(q[rows - 1], K, V, nh).reshape(nh, hd)
    assert abs(want[3] - 4.0).max() < 1e-3 and abs(want[7] - 5.0).max() < 1e-3 and abs(want[0] - 4.0).max() > 1.0
    block_call(gpu, q, K, V, pos0, nh)


def test_block_attention_f16_row_does_not_depend_on_its_block(gpu):
    nh, nkv, hd, rng = 8, 2, 128, np.random.default_rng([77])
    K, V = (rng.standard_normal((1064, nkv, hd), dtype=np.float32).astype(np.float16) for _ in "kv")
    q = rng.standard_normal((64, nh * hd), dtype=np.float32)                                  # row r: the query at absolute position 1000 + r
    got = [block_call(gpu, q[pos0 - 1000:pos0 - 1000 + rows], K[:pos0 + rows], V[:pos0 + rows], pos0, nh)[0][1010 - pos0].view(torch.int32)
           for pos0, rows in ((1000, 64), (1010, 1), (1003, 17))]
    assert torch.equal(got[0], got[1]) and torch.equal(got[0], got[2])


# ---------------------------------------------------------------- 5. / 6. through the Decoder
def test_decoder_with_f16_caches(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    cfg, steps = small_model.cfg, 12
    prompt = [int(t) for t in np.random.default_rng([79]).integers(0, 512, 40)]
    dec = Decoder(small_model, maxTokens=8256, kv_cache="f16")                   # (past what any f32 entry point accepts)
    assert dec.kCache[0].dtype == torch.float16 and tuple(dec.vCache[1].shape) == (8256, cfg.numHeadsKV, cfg.headDim)
    dec.run(prompt[:7], steps, dense=True)
    K, V = (c[-1][:steps].cpu().numpy() for c in (dec.kCache, dec.vCache))       # the last layer's rows 0 .. the last position
    got, want = dec.attnOutput.cpu().numpy(), want_of(dec.xq.cpu().numpy(), K, V, cfg.numHeads)     # the last step, over the decoder's own caches
    assert within_bar(got, want), bar_figures(got, want)
    assert all(not bool(c[steps:].any()) for c in dec.kCache + dec.vCache), "a cache row past the last position was written"
    two, got = Decoder(small_model, maxTokens=64, kv_cache="f16"), []
    for chunk in (64, 16):
        for c in two.kCache + two.vCache:
            c.fill_(float("nan"))
        two.prefill(prompt, chunk=chunk, attention="block")
        got.append([c[:40].clone().view(torch.int16) for c in two.kCache + two.vCache])
        assert all(bool(torch.isnan(c[40:]).all()) for c in two.kCache + two.vCache)
    assert all(torch.equal(a, b) for a, b in zip(*got)) and bool(torch.isfinite(two.kCache[1][:40]).all())
    with pytest.raises(ValueError):
        two.prefill(prompt, attention="rows")
    with pytest.raises(ValueError):
        two.token_step(split=True)
    for bad in (dict(emulate_world=True, world=2), dict(split_attention_from=0), dict(maxTokens=32769)):
        with pytest.raises(ValueError):
            Decoder(small_model, **dict(dict(maxTokens=64, kv_cache="f16"), **bad))
    plain = Decoder(small_model, maxTokens=16)
    assert plain.kCache[0].dtype == torch.float32 and tuple(plain.kCache[0].shape) == (16, cfg.numHeads, cfg.headDim) and plain.splitScratch is None


def test_dense_path_with_f16_caches_against_the_torch_reference(small_model):  # noqa: F811
    """tests/test_gpu_decode.py::test_dense_path_matches_torch_reference on f16 caches: the reference keeps f32 K / V, so the figure is the
    price of the format."""
    from effort_amd.decode import Decoder
    prompt, steps = [3, 77, 130], 10
    want_ids, want_logits = torch_reference(small_model, prompt, steps)
    ids, _, logits = Decoder(small_model, maxTokens=16, kv_cache="f16").run(prompt, steps, dense=True, collect_logits=True)
    err = float((logits - want_logits).abs().max() / want_logits.abs().max())
    print(f"kv_cache='f16': logits within {err:.3g} of max|logit| of the f32 reference; greedy picks agree at {sum(a == b for a, b in zip(ids, want_ids))} of {steps} steps")
    assert err < 2e-3, err
