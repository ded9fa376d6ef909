"""effort_attention_block (effort_amd/csrc/attention_block.hip): prefill attention in which a block's queries share each K / V tile.

The bar is the project's f32 bar (``within_bar`` of tests/test_gpu_glue.py: |got - want| <= 2e-5 * max|want| and cos-sim >= 0.999999)
against the float64 reference ``glue_reference.attention``.  What a correct f32 evaluation of the scheme -- 16-key tiles, four
round-robin partial states merged at the end -- leaves of it, from a numpy f32 model on N(0, 1) inputs at T = 17 / 1025 / 8192 and
headDim 64 / 128 / 256: worst error 1.6e-6 * max|want|, worst 1 - cos 6.4e-13, under a tenth of the bar.  The measured worst error over
the bar is printed per case.

  1. every row and head against float64, NaN in every place the kernel must not read or write;
  2. causal inside the block: the key right behind each query would win its softmax if it were seen;
  3. a row's bits do not depend on the block it sits in (pos0, rows, its place);
  4. refusals return their codes and write nothing;
  5. through Decoder.prefill / Decoder.run with attention="block".
"""
import math

import numpy as np
import pytest
import torch

from tests import glue_reference as ref
from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import BAR_REL, DEV, P, bar_figures, dev, gpu, lib, nans, within_bar  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
HEAD_DIMS = (64, 128, 256)
HEADS = 4
BLOCKS = ((0, 1), (0, 16), (0, 17), (0, 64), (1, 15), (5, 3), (15, 2), (16, 16), (17, 33), (63, 64), (64, 64), (200, 64), (1000, 40))
LONG = (2, 8128, 64, 8192)                               # heads, pos0, rows, maxTokens: the last row of the largest cache is in use
GUARD = 8


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b) -> bool:
    return bool(torch.equal(bits(a), bits(b)))


def max_tokens(pos0, rows):
    return (pos0 + rows + 63) // 64 * 64


def call(gpu, q, K, V, pos0, rows, heads, headDim, maxTokens):
    """The call with NaN wherever the kernel has no business: q rows >= rows (of 64), cache rows >= pos0 + rows, all of out and a guard
    behind it.  q [rows][heads * headDim], K / V [pos0 + rows][heads][headDim] numpy f32.  Returns out [rows][heads * headDim] (torch)."""
    n = heads * headDim
    qd, kc, vc = nans(64, n), nans(maxTokens, heads, headDim), nans(maxTokens, heads, headDim)
    qd[:rows] = dev(q)
    kc[:pos0 + rows] = dev(K)
    vc[:pos0 + rows] = dev(V)
    k0, v0, q0 = kc.clone(), vc.clone(), qd.clone()
    out = nans(rows * n + GUARD)
    gpu.check(lib().effort_attention_block(gpu.ctx, P(qd), P(kc), P(vc), pos0, rows, P(out), heads, headDim, maxTokens), "attention_block")
    gpu.eval()
    assert bool(torch.isnan(out[rows * n:]).all()), "wrote past out[rows]"
    assert same_bits(kc, k0) and same_bits(vc, v0) and same_bits(qd, q0), "an input was written"
    return out[:rows * n].view(rows, n)


def check_rows(got, q, K, V, pos0, rows, heads, headDim, tag):
    """Every row against ref.attention over cache rows 0 .. pos0 + r; returns the worst error / max|want| of the rows."""
    K64, V64 = K.astype(np.float64), V.astype(np.float64)
    got, worst = got.cpu().numpy(), 0.0
    assert np.isfinite(got).all(), (tag, "a NaN reached a result: a row that must not be read, or a masked key multiplied in")
    for r in range(rows):
        want = ref.attention(q[r].reshape(heads, headDim), K64[:pos0 + r + 1], V64[:pos0 + r + 1])
        worst = max(worst, bar_figures(got[r], want)[0])
        assert within_bar(got[r], want), (tag, r, bar_figures(got[r], want))
    return worst


def random_block(seed, pos0, rows, heads, headDim):
    rng = np.random.default_rng(seed)
    f = lambda *shape: rng.standard_normal(shape, dtype=np.float32)      # noqa: E731
    return f(rows, heads * headDim), f(pos0 + rows, heads, headDim), f(pos0 + rows, heads, headDim)


# ---------------------------------------------------------------- 1. against float64
@pytest.mark.parametrize("headDim", HEAD_DIMS)
def test_block_attention_matches_float64(gpu, headDim):
    for pos0, rows in BLOCKS:
        q, K, V = random_block([51, headDim, pos0, rows], pos0, rows, HEADS, headDim)
        got = call(gpu, q, K, V, pos0, rows, HEADS, headDim, max_tokens(pos0, rows))
        worst = check_rows(got, q, K, V, pos0, rows, HEADS, headDim, (headDim, pos0, rows))
        print(f"attention_block headDim {headDim} pos0 {pos0} rows {rows}: worst error over the bar {worst / BAR_REL:.3g}")


@pytest.mark.parametrize("headDim", HEAD_DIMS)
def test_block_attention_at_the_end_of_the_largest_cache(gpu, headDim):
    heads, pos0, rows, maxTokens = LONG
    q, K, V = random_block([52, headDim], pos0, rows, heads, headDim)
    got = call(gpu, q, K, V, pos0, rows, heads, headDim, maxTokens)
    worst = check_rows(got, q, K, V, pos0, rows, heads, headDim, (headDim, "long"))
    print(f"attention_block headDim {headDim} pos0 {pos0} rows {rows}: worst error over the bar {worst / BAR_REL:.3g}")


# ---------------------------------------------------------------- 2. causal inside the block
@pytest.mark.parametrize("pos0,rows", [(0, 17), (5, 64), (250, 20)])
@pytest.mark.parametrize("headDim", (64, 128))
def test_block_attention_is_causal_inside_the_block(gpu, headDim, pos0, rows):
    """Cache row pos0 + r + 1 -- the first key query r may NOT see -- is c * q[r], its score with query r 40 (marker_case's
    construction); V row t is t + 1.  A query that sees one future key moves by O(1)."""
    q, K, V = random_block([53, headDim, pos0, rows], pos0, rows, HEADS, headDim)
    qh = q.reshape(rows, HEADS, headDim).astype(np.float64)
    c = 40.0 * math.sqrt(headDim) / (qh ** 2).sum(axis=2)                               # [rows][heads]
    for r in range(rows - 1):
        K[pos0 + r + 1] = (c[r][:, None] * qh[r]).astype(np.float32)
    V[:] = np.arange(1, pos0 + rows + 1, dtype=np.float32)[:, None, None]
    got = call(gpu, q, K, V, pos0, rows, HEADS, headDim, max_tokens(pos0, rows))
    worst = check_rows(got, q, K, V, pos0, rows, HEADS, headDim, (headDim, pos0, rows, "markers"))
    print(f"attention_block markers headDim {headDim} pos0 {pos0} rows {rows}: worst error over the bar {worst / BAR_REL:.3g}")


# ---------------------------------------------------------------- 3. a row does not depend on its block
@pytest.mark.parametrize("first", (5, 1000))
@pytest.mark.parametrize("headDim", (64, 128))
def test_a_row_does_not_depend_on_its_block(gpu, headDim, first):
    """64 queries at absolute positions first .. first + 63 as one call, four calls of 16, calls of 7 and 64 calls of 1, all on ONE
    cache: every output row bit-identical across the four."""
    n, maxTokens = HEADS * headDim, max_tokens(first, 64)
    q, K, V = random_block([54, headDim, first], first, 64, HEADS, headDim)
    qd, kc, vc = dev(q), nans(maxTokens, HEADS, headDim), nans(maxTokens, HEADS, headDim)
    kc[:first + 64] = dev(K)
    vc[:first + 64] = dev(V)
    outs = []
    for step in (64, 16, 7, 1):
        out = nans(64, n)
        for r0 in range(0, 64, step):
            rows = min(step, 64 - r0)
            gpu.check(lib().effort_attention_block(gpu.ctx, P(qd[r0]), P(kc), P(vc), first + r0, rows, P(out[r0]), HEADS, headDim, maxTokens),
                      "attention_block")
        gpu.eval()
        outs.append(out)
    assert bool(torch.isfinite(outs[0]).all())
    for step, other in zip((16, 7, 1), outs[1:]):
        differ = [r for r in range(64) if not same_bits(outs[0][r], other[r])]
        assert not differ, (headDim, first, f"rows {differ} of the single call differ from calls of {step}")


# ---------------------------------------------------------------- 4. refusals
def test_block_attention_refusals_write_nothing(gpu):
    headDim, maxTokens = 64, 64
    n = HEADS * headDim
    q, kc, vc, out = dev(np.ones((64, n), dtype=np.float32)), nans(maxTokens, HEADS, headDim), nans(maxTokens, HEADS, headDim), nans(64 * n)
    f = lib().effort_attention_block
    assert f(gpu.ctx, None, P(kc), P(vc), 0, 4, P(out), HEADS, headDim, maxTokens) == -1            # a null argument
    assert f(gpu.ctx, P(q), None, P(vc), 0, 4, P(out), HEADS, headDim, maxTokens) == -1
    assert f(gpu.ctx, P(q), P(kc), None, 0, 4, P(out), HEADS, headDim, maxTokens) == -1
    assert f(gpu.ctx, P(q), P(kc), P(vc), 0, 4, None, HEADS, headDim, maxTokens) == -1
    assert f(None, P(q), P(kc), P(vc), 0, 4, P(out), HEADS, headDim, maxTokens) == -1
    for rows in (0, 65, -1):
        assert f(gpu.ctx, P(q), P(kc), P(vc), 0, rows, P(out), HEADS, headDim, maxTokens) == -1
    assert f(gpu.ctx, P(q), P(kc), P(vc), -1, 4, P(out), HEADS, headDim, maxTokens) == -1
    assert f(gpu.ctx, P(q), P(kc), P(vc), 61, 4, P(out), HEADS, headDim, maxTokens) == -1           # pos0 + rows > maxTokens
    assert f(gpu.ctx, P(q), P(kc), P(vc), 64, 1, P(out), HEADS, headDim, maxTokens) == -1
    for hd in (96, 32, 512):
        assert f(gpu.ctx, P(q), P(kc), P(vc), 0, 4, P(out), HEADS, hd, maxTokens) == -2
    assert f(gpu.ctx, P(q), P(kc), P(vc), 0, 4, P(out), HEADS, headDim, 8193) == -2
    gpu.eval()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(kc).all()) and bool(torch.isnan(vc).all())


# ---------------------------------------------------------------- 5. through the Decoder
PROMPT_SEED = 0          # tests/test_gpu_prefill.py: the seed whose token-by-token dense run keeps the compared steps' top-1 / top-2 gap above 4e-3
STEPS, MAXTOK = 12, 32


def prompt_of(seed):
    return [int(t) for t in np.random.default_rng([41, seed]).integers(0, 512, 7)]


def caches(dec, rows):
    return [(dec.kCache[n][:rows].clone(), dec.vCache[n][:rows].clone()) for n in range(len(dec.kCache))]


def poison(dec):
    for c in dec.kCache + dec.vCache:
        c.fill_(float("nan"))


def rel(a, b) -> float:
    return float((a - b).abs().max() / b.abs().max())


def test_decoder_prefill_with_block_attention(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=MAXTOK)
    prompt = prompt_of(PROMPT_SEED)
    dec.prefill(prompt[:6])
    rows_kv = caches(dec, 6)
    poison(dec)
    dec.prefill(prompt[:6], attention="block")
    assert int(dec.pos[0]) == 6
    block_kv = caches(dec, 6)
    for which in (0, 1):
        assert same_bits(block_kv[0][which], rows_kv[0][which]), "layer 0: nothing before its K / V passes through attention"
        assert rel(block_kv[1][which], rows_kv[1][which]) < 2e-3, which


def test_decoder_prefill_block_attention_does_not_depend_on_the_chunk(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=64)
    prompt = [int(t) for t in np.random.default_rng([42, 0]).integers(0, 512, 40)]
    got = []
    for chunk in (64, 16, 5):
        poison(dec)
        dec.prefill(prompt, chunk=chunk, attention="block")
        got.append(caches(dec, 40))
        assert all(bool(torch.isfinite(t).all()) for pair in got[-1] for t in pair)
        assert all(bool(torch.isnan(c[40:]).all()) for c in dec.kCache + dec.vCache), "a cache row beyond the prompt was written"
    for other in got[1:]:
        for (k0, v0), (k1, v1) in zip(got[0], other):
            assert same_bits(k0, k1) and same_bits(v0, v1)
    poison(dec)
    dec.prefill(prompt)
    for (k0, v0), (k1, v1) in zip(got[0], caches(dec, 40)):
        assert rel(k0, k1) < 2e-3 and rel(v0, v1) < 2e-3


def test_run_with_block_attention_matches_the_token_loop(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=MAXTOK)
    prompt = prompt_of(PROMPT_SEED)
    P1 = len(prompt) - 1
    ids, _, logits = dec.run(prompt, STEPS, dense=True, collect_logits=True)
    ids_b, _, logits_b = dec.run(prompt, STEPS, dense=True, prefill=True, prefill_attention="block", collect_logits=True)
    err = rel(logits_b, logits[P1:])
    print(f"logits after a block-attention prefill against the token loop: {err:.3g} of max|logit|")
    assert err < 2e-3, err
    assert ids_b[:P1] == [-1] * P1 and ids_b[P1:] == ids[P1:]
