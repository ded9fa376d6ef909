"""Prompt prefill on the GPU (effort_amd/csrc/prefill.hip, the block glue in effort_amd/csrc/decode.hip, Decoder.prefill).

  1. effort_dense_gemm_rows against the float64 reference of basicMul (tests/glue_reference.py: dense), row by row, at the bar the
     in-tree GEMV meets with the same exact f16 products and f32 sums: ``dense_close`` with DENSE_BAND = 1e-5.  An MFMA step sums 32
     exact products into an f32 accumulator -- f32 additions in some order, like the GEMV's fma chains --, so the same band applies;
     the measured worst error over the band is printed per shape.
  2. A row's bits do not depend on the number of rows or on its position in the block.
  3. The block forms of the glue write, per row, the bits of the single-token entry points (which tests/test_gpu_glue.py pins to
     float64 references).
  4. End to end: prefill + decode against the token-by-token dense loop on test_gpu_decode's small model.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_reference as ref
from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import DEV, ROPE_BASE, P, dev, gpu, lib, nans, within_bar  # noqa: F401  (gpu: the fixture)
from tests.test_gpu_parity import DENSE_BAND, dense_close
from tests.util import make_v, make_w

pytestmark = pytest.mark.gpu
MAX_ROWS = 64
SENTINEL = -555.0


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b) -> bool:
    return bool(torch.equal(bits(a), bits(b)))


# ---------------------------------------------------------------- 0. prefill leaves the captured token step's scratch alone
def test_prefill_after_a_captured_step_on_the_rocblas_backend(small_model):  # noqa: F811
    """The FIRST test of this module, and no module before it calls the block multiply: its scratch is allocated HERE, after the step
    was captured.  Under the rocBLAS dense backend the captured step holds the address of the context's f16 copy of v
    (effort_dense_gemv); the block multiply keeps f16(x) in a buffer of its own, so growing it frees nothing a graph points to.
    Sequence: capture and run the dense step, then ``run(prefill=True)`` on the same graph -- its steps must give what the token loop
    gave (the decode tests' 2e-3 bar: rocBLAS sums in another order than the block kernel; same greedy tokens), and the token loop,
    replayed once more after the prefill, must give its own bits again."""
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=MAXTOK)
    prompt = prompt_of(PROMPT_SEED)
    P1 = len(prompt) - 1
    dec.g.set_dense_backend(True)
    try:
        ids, _, logits = dec.run(prompt, STEPS, dense=True, collect_logits=True)
        ids_p, _, logits_p = dec.run(prompt, STEPS, dense=True, prefill=True, collect_logits=True)
        ids_again, _, logits_again = dec.run(prompt, STEPS, dense=True, collect_logits=True)
    finally:
        dec.g.set_dense_backend(False)
    assert len(dec._graphs) == 1
    err = float((logits_p - logits[P1:]).abs().max() / logits[P1:].abs().max())
    print(f"rocBLAS backend, logits after prefill against the token loop: {err:.3g} of max|logit|")
    assert err < 2e-3, err
    assert ids_p[:P1] == [-1] * P1 and ids_p[P1:] == ids[P1:]
    assert ids_again == ids and same_bits(logits_again, logits)


# ---------------------------------------------------------------- 1. the block multiply against float64
# (outDim, inDim, rows) and what each reaches.  The kernel's template parameters are the token tiles NT = ceil(rows / 16) and the cache
# policy of the weight stream (nt above 64 MiB): every (NT, policy) pair occurs.  Its k split (pf_split, a function of the shape):
# stages = ceil(inDim / 256); groups = ceil(outDim / 64) workgroups of 64 rows; splits wanted = min(ceil(256 / groups), 16, stages);
# per = ceil(stages / wanted) stages per split; splits = ceil(stages / per).  One split writes out itself, more go through the partial
# sums and reduce_splits_kernel; a split of more than one stage runs the double-buffered loop.
GEMM_SHAPES = [
    (17, 32, 16),         # 1 stage, 1 split, written directly; the stage holds 32 live elements of 256; ragged 16-row tile (row 16 alone in wave 1), NT 1 full
    (24, 64, 1),          # 1 stage, 1 split; one live token column; waves 2 and 3 of the group own no row
    (1024, 4096, 5),      # the wk / wv shape: 16 stages, 16 groups -> per 1, 16 splits (the cap): every split is one stage (no loop), reduce over 16
    (4096, 4096, 17),     # 16 stages, 64 groups -> per 4, 4 even splits: loop + reduce; NT 2, the second token tile with one live column
    (512, 14336, 64),     # the longest K: 56 stages, 8 groups -> per 4, 14 even splits; all four token tiles full (NT 4)
    (8200, 4096, 16),     # above 64 MiB: the nt weight stream, NT 1; 129 groups -> per 8, 2 splits; the last group holds 8 rows (8200 = 128 * 64 + 8)
    (40, 96, 33),         # NT 3 with one live column in the third tile; 1 stage with 96 live elements (a chunk and a half), 1 split
    (16, 1056, 48),       # NT 3 full; 5 stages, 1 group -> per 1, 5 splits; the last stage holds 32 live elements (1056 = 4 * 256 + 32)
    (16400, 512, 3),      # ONE split over several stages: 257 groups -> 1 split of 2 stages: the double-buffered loop writes out itself, no reduce; last group 16 rows
    (64, 11008, 20),      # an UNEVEN last split: 43 stages, 1 group -> per 3, 15 splits, the last one clipped to 1 stage (s1 = min(s0 + per, stages)); NT 2
    (8200, 4096, 17),     # nt, NT 2
    (8200, 4096, 33),     # nt, NT 3
    (8200, 4096, 64),     # nt, NT 4
]
EDGE_ROWS_ONLY = {(8200, 4096, 17), (8200, 4096, 33), (8200, 4096, 64)}      # 0.15 s of float64 per row: first and last row of every token tile
_W, _X, _WANT = {}, {}, {}


def gemm_inputs(outDim, inDim):
    """W f16 (numpy and device) and 64 heavy-tailed rows, shared by the cases of a matrix shape; left unchanged."""
    key = (outDim, inDim)
    if key not in _W:
        W = make_w(outDim, inDim, seed=3)
        _W[key] = (W, dev(W.view(np.int16)))
        _X[key] = np.stack([make_v(inDim, seed=100 + r, heavy=True) for r in range(MAX_ROWS)])
        _WANT[key] = {}
    return _W[key] + (_X[key],)


def want_row(outDim, inDim, r):
    """glue_reference.dense of row r, computed once."""
    W, _, X = gemm_inputs(outDim, inDim)
    if r not in _WANT[(outDim, inDim)]:
        _WANT[(outDim, inDim)][r] = ref.dense(W, X[r])
    return _WANT[(outDim, inDim)][r]


def gemm_rows(gpu, Wd, x_rows, rows, outDim, inDim, beyond=float("nan"), alloc_rows=MAX_ROWS):
    """The call on a NaN-filled out with a sentinel tail; x rows at and beyond ``rows`` hold ``beyond``.  Returns out f32 [rows][outDim]."""
    x = torch.full((alloc_rows, inDim), beyond, dtype=torch.float32, device=DEV)
    x[:rows] = dev(np.ascontiguousarray(x_rows, dtype=np.float32))
    out = nans(rows * outDim + 8)
    out[rows * outDim:] = SENTINEL
    gpu.check(lib().effort_dense_gemm_rows(gpu.ctx, P(Wd), P(x), P(out), inDim, outDim, rows), "dense_gemm_rows")
    gpu.eval()
    assert bool((out[rows * outDim:] == SENTINEL).all()), "wrote past rows * outDim"
    return out[:rows * outDim].view(rows, outDim)


@pytest.mark.parametrize("outDim,inDim,rows", GEMM_SHAPES)
def test_block_multiply_matches_float64(gpu, outDim, inDim, rows):
    W, Wd, X = gemm_inputs(outDim, inDim)
    out = gemm_rows(gpu, Wd, X[:rows], rows, outDim, inDim)
    assert bool(torch.isfinite(out).all()), "a NaN row of x beyond `rows` (or of out) reached a result"
    other = gemm_rows(gpu, Wd, X[:rows], rows, outDim, inDim, beyond=1.0)
    assert same_bits(out, other), "x rows beyond `rows` changed the result"
    got = out.cpu().numpy()
    worst = 0.0
    check = range(rows) if (outDim, inDim, rows) not in EDGE_ROWS_ONLY else sorted({r for t in range(0, rows, 16) for r in (t, min(t + 15, rows - 1))})
    for r in check:
        want = want_row(outDim, inDim, r)
        band = DENSE_BAND * np.abs(want).max() + DENSE_BAND * np.abs(want)
        worst = max(worst, float((np.abs(got[r] - want) / band).max()))
        assert dense_close(got[r], want, DENSE_BAND), (r, float(np.abs(got[r] - want).max() / np.abs(want).max()))
    print(f"dense_gemm_rows ({outDim}, {inDim}, {rows}): worst error over the 1e-5 band {worst:.3g}")


def test_block_multiply_refuses_with_nothing_written(gpu):
    """A refused call (shape, rows) leaves out alone: the caller's fallback finds it as it was."""
    _, Wd, X = gemm_inputs(24, 64)
    x, out = dev(X[:2].copy()), nans(2 * 24)
    assert lib().effort_dense_gemm_rows(gpu.ctx, P(Wd), P(x), P(out), 48, 24, 2) == -2
    assert lib().effort_dense_gemm_rows(gpu.ctx, P(Wd), P(x), P(out), 64, 24, 65) == -1
    assert lib().effort_dense_gemm_rows(gpu.ctx, P(Wd), P(x), None, 64, 24, 2) == -1
    gpu.eval()
    assert bool(torch.isnan(out).all())


# ---------------------------------------------------------------- 2. row independence, bit for bit
def test_rows_do_not_depend_on_the_block(gpu):
    outDim, inDim = 512, 14336
    _, Wd, X = gemm_inputs(outDim, inDim)
    full = gemm_rows(gpu, Wd, X, 64, outDim, inDim)
    for r in (0, 15, 16, 63):
        alone = gemm_rows(gpu, Wd, X[r:r + 1], 1, outDim, inDim)
        assert same_bits(full[r], alone[0]), f"row {r} of 64 against the row alone"
        five = np.stack([X[40], X[41], X[42], X[r], X[43]])
        placed = gemm_rows(gpu, Wd, five, 5, outDim, inDim)
        assert same_bits(full[r], placed[3]), f"row {r} of 64 against position 3 of 5"


# ---------------------------------------------------------------- 3. the block glue equals the single-token entry points
HEADS, HEADS_KV, MAX_TOKENS = 8, 2, 32
GLUE = [(hd, pos0, rows) for hd in (64, 128) for pos0 in (0, 5) for rows in (1, 3, 17)]
GLUE.append((256, 5, 3))                                             # headDim 256: the one head size at which attention has a single value phase


def rnd(seed, *shape):
    return dev(np.random.default_rng(seed).standard_normal(shape, dtype=np.float32))


def pos_dev(pos):
    return torch.tensor([pos], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("rows", (1, 3, 17))
def test_fetch_rows_is_fetch_row(gpu, rows):
    n, vocab = 1000, 50
    rng = np.random.default_rng([21, rows])
    table = dev(rng.standard_normal((vocab, n), dtype=np.float32).astype(np.float16).view(np.int16))
    ids = torch.from_numpy(rng.integers(0, vocab, rows).astype(np.int32)).to(DEV)
    out = nans(rows * n + 8)
    gpu.check(lib().effort_fetch_rows(gpu.ctx, P(table), P(ids), P(out), n, rows), "fetch_rows")
    one = nans(rows, n)
    for r in range(rows):
        gpu.check(lib().effort_fetch_row(gpu.ctx, P(table), P(ids[r:r + 1]), P(one[r]), n), "fetch_row")
    gpu.eval()
    assert same_bits(out[:rows * n].view(rows, n), one) and bool(torch.isnan(out[rows * n:]).all())


@pytest.mark.parametrize("with_delta", (False, True))
@pytest.mark.parametrize("rows", (1, 3, 17))
@pytest.mark.parametrize("n", (1000, 4096, 5120))                    # both sides of the kernel's register / loop switch at 4096
def test_add_rmsnorm_mul_rows_is_add_rmsnorm_mul(gpu, n, rows, with_delta):
    h0, delta = rnd([22, n, rows], rows, n), (rnd([23, n, rows], rows, n) * 0.5 if with_delta else None)
    w = dev((1.0 + 0.1 * np.random.default_rng([24, n]).standard_normal(n)).astype(np.float16).view(np.int16))
    h = torch.cat([h0.reshape(-1), nans(8)])
    out = nans(rows * n + 8)
    gpu.check(lib().effort_add_rmsnorm_mul_rows(gpu.ctx, P(h), P(delta), P(w), P(out), n, rows), "add_rmsnorm_mul_rows")
    h1, out1 = h0.clone(), nans(rows, n)
    for r in range(rows):
        gpu.check(lib().effort_add_rmsnorm_mul(gpu.ctx, P(h1[r]), P(delta[r]) if with_delta else None, P(w), P(out1[r]), n), "add_rmsnorm_mul")
    gpu.eval()
    assert same_bits(out[:rows * n].view(rows, n), out1) and same_bits(h[:rows * n].view(rows, n), h1)
    assert bool(torch.isnan(out[rows * n:]).all()) and bool(torch.isnan(h[rows * n:]).all())
    assert with_delta or same_bits(h1, h0)


@pytest.mark.parametrize("headDim,pos0,rows", GLUE)
def test_rope_kv_rows_is_rope_kv(gpu, headDim, pos0, rows):
    q, kv = HEADS * headDim, HEADS_KV * headDim
    xq, xk, xv = rnd([25, headDim, pos0, rows], rows, q), rnd([26, headDim, pos0, rows], rows, kv), rnd([27, headDim, pos0, rows], rows, kv)
    rope = C.c_float(ROPE_BASE)
    qo, kc, vc = nans(rows * q + 8), nans(MAX_TOKENS, HEADS, headDim), nans(MAX_TOKENS, HEADS, headDim)
    gpu.check(lib().effort_rope_kv_rows(gpu.ctx, P(xq), P(xk), P(xv), P(qo), P(kc), P(vc), pos0, rows, HEADS, HEADS_KV, headDim, MAX_TOKENS, rope), "rope_kv_rows")
    qo1, kc1, vc1 = nans(rows, q), nans(MAX_TOKENS, HEADS, headDim), nans(MAX_TOKENS, HEADS, headDim)
    for r in range(rows):
        gpu.check(lib().effort_rope_kv(gpu.ctx, P(xq[r]), P(xk[r]), P(xv[r]), P(qo1[r]), P(kc1), P(vc1), P(pos_dev(pos0 + r)), HEADS, HEADS_KV, headDim,
                                       MAX_TOKENS, rope), "rope_kv")
    gpu.eval()
    assert same_bits(qo[:rows * q].view(rows, q), qo1) and bool(torch.isnan(qo[rows * q:]).all())
    assert same_bits(kc, kc1) and same_bits(vc, vc1)                  # the written rows AND the NaN poison everywhere else (same NaN bits)
    own = torch.zeros(MAX_TOKENS, dtype=torch.bool, device=DEV)
    own[pos0:pos0 + rows] = True
    for cache in (kc, vc):
        assert bool(torch.isfinite(cache[own]).all()) and bool(torch.isnan(cache[~own]).all())


@pytest.mark.parametrize("headDim,pos0,rows", GLUE)
def test_attention_rows_is_attention_and_is_causal(gpu, headDim, pos0, rows):
    q = HEADS * headDim
    xq = rnd([28, headDim, pos0, rows], rows, q)
    kc, vc = rnd([29, headDim, pos0, rows], MAX_TOKENS, HEADS, headDim), rnd([30, headDim, pos0, rows], MAX_TOKENS, HEADS, headDim)
    kc[pos0 + rows:] = float("nan")                                   # rows beyond the block: never read by anyone
    vc[pos0 + rows:] = float("nan")
    out = nans(rows * q + 8)
    gpu.check(lib().effort_attention_rows(gpu.ctx, P(xq), P(kc), P(vc), pos0, rows, P(out), HEADS, headDim, MAX_TOKENS), "attention_rows")
    one = nans(rows, q)
    for r in range(rows):
        k1, v1 = kc.clone(), vc.clone()
        k1[pos0 + r + 1:] = float("nan")                              # the single-token call sees nothing beyond its own position
        v1[pos0 + r + 1:] = float("nan")
        gpu.check(lib().effort_attention(gpu.ctx, P(xq[r]), P(k1), P(v1), P(pos_dev(pos0 + r)), P(one[r]), HEADS, headDim, MAX_TOKENS), "attention")
    gpu.eval()
    got = out[:rows * q].view(rows, q)
    assert bool(torch.isfinite(got).all()), "a query of the block read a cache row beyond its own position"
    assert same_bits(got, one) and bool(torch.isnan(out[rows * q:]).all())


def test_block_glue_refusals_enqueue_nothing(gpu):
    kc, x = nans(MAX_TOKENS, HEADS, 64), rnd(31, 4, HEADS * 64)
    rope = C.c_float(ROPE_BASE)
    assert lib().effort_rope_kv_rows(gpu.ctx, P(x), P(x), P(x), P(x), P(kc), P(kc), 30, 3, HEADS, HEADS, 64, MAX_TOKENS, rope) == -1
    assert lib().effort_rope_kv_rows(gpu.ctx, P(x), P(x), P(x), P(x), P(kc), P(kc), -1, 3, HEADS, HEADS, 64, MAX_TOKENS, rope) == -1
    assert lib().effort_attention_rows(gpu.ctx, P(x), P(kc), P(kc), 30, 3, P(x), HEADS, 64, MAX_TOKENS) == -1
    gpu.eval()
    assert bool(torch.isnan(kc).all())


# ---------------------------------------------------------------- 4. end to end
PROMPT_SEED = 0          # the first seed whose token-by-token dense run keeps every compared step's top-1 / top-2 gap above 4e-3 * max|logit|
STEPS, MAXTOK = 12, 32


def prompt_of(seed):
    return [int(t) for t in np.random.default_rng([41, seed]).integers(0, 512, 7)]


def min_gap(logits):
    """Smallest (top-1 - top-2) / max|logit| over the steps."""
    top = torch.topk(logits, 2, dim=1).values
    return float(((top[:, 0] - top[:, 1]) / logits.abs().amax(dim=1)).min())


def caches(dec, rows=6):
    return [(dec.kCache[n][:rows].clone(), dec.vCache[n][:rows].clone()) for n in range(len(dec.kCache))]


@pytest.fixture(scope="module")
def token_run(small_model):  # noqa: F811
    """The token-by-token dense run: how the prompt is ingested without prefill.  Computed once."""
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=MAXTOK)
    prompt = prompt_of(PROMPT_SEED)
    ids, _, logits = dec.run(prompt, STEPS, dense=True, collect_logits=True)
    return dec, prompt, ids, logits, caches(dec)


def test_prefill_then_decode_matches_the_token_loop(token_run):
    dec, prompt, ids, logits, kv = token_run
    P1 = len(prompt) - 1
    gap = min_gap(logits[P1:])
    print(f"smallest top-1 / top-2 gap of the compared steps: {gap:.3g} of max|logit|")
    assert gap > 4e-3, "PROMPT_SEED no longer qualifies: the greedy comparison needs a decided reference run"
    ids_p, _, logits_p = dec.run(prompt, STEPS, dense=True, prefill=True, collect_logits=True)
    assert tuple(logits_p.shape) == (STEPS - P1, logits.shape[1]) and dec.last_prefill_s > 0
    err = float((logits_p - logits[P1:]).abs().max() / logits[P1:].abs().max())
    print(f"logits after prefill against the token loop: {err:.3g} of max|logit|")
    assert err < 2e-3, err
    assert ids_p[:P1] == [-1] * P1 and ids_p[P1:] == ids[P1:]


def test_prefill_caches_match_the_token_loop(token_run):
    dec, prompt, _, _, kv = token_run
    dec.prefill(prompt[:6])
    assert int(dec.pos[0]) == 6
    got = caches(dec)
    for which in (0, 1):                                             # K, V of layer 0: the norm is bit-identical, only the multiply's order differs
        assert within_bar(got[0][which].cpu().numpy(), kv[0][which].cpu().numpy()), which
        a, b = got[1][which], kv[1][which]
        assert float((a - b).abs().max() / b.abs().max()) < 2e-3, which


def test_prefill_does_not_depend_on_the_chunk(token_run):
    dec, prompt, _, _, _ = token_run
    got = []
    for chunk in (1, 4, 64):
        for n in range(len(dec.kCache)):
            dec.kCache[n].fill_(float("nan"))
            dec.vCache[n].fill_(float("nan"))
        dec.prefill(prompt[:6], chunk=chunk)
        got.append(caches(dec))
        assert all(bool(torch.isfinite(t).all()) for pair in got[-1] for t in pair)
        assert all(bool(torch.isnan(c[6:]).all()) for c in dec.kCache + dec.vCache), "a cache row beyond the prompt was written"
    for other in got[1:]:
        for (k0, v0), (k1, v1) in zip(got[0], other):
            assert same_bits(k0, k1) and same_bits(v0, v1)


def test_effort_decode_after_a_prefill(token_run):
    dec, prompt, ids, _, _ = token_run
    ids_e, dt, _ = dec.run(prompt, STEPS, effort=0.25, prefill=True)             # run raises on a device status
    assert ids_e[:6] == [-1] * 6 and len(ids_e) == STEPS and all(0 <= t < 512 for t in ids_e[6:])


def test_prefill_on_a_q4_model(hip_lib_built):
    from effort_amd.decode import Decoder, MistralConfig, Model
    cfg = MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=2, numHeads=32, numHeadsKV=8, headDim=128, vocab=512)
    dec = Decoder(Model.random(cfg, seed=5, q4=True), maxTokens=16)
    ids, _, _ = dec.run([3, 77, 130, 9], 6, effort=0.25, prefill=True)          # the cores prefill, the Q4 step follows: no status
    assert ids[:3] == [-1] * 3 and all(0 <= t < 512 for t in ids[3:])
    assert all(bool(torch.isfinite(c[:6]).all()) for c in dec.kCache + dec.vCache)


def test_prefill_refusals_change_nothing(token_run):
    from effort_amd.decode import Decoder, MistralConfig, Model
    dec, prompt, _, _, _ = token_run

    def refused(d, tokens, **kw):
        d.pos.fill_(3)
        for c in d.kCache + d.vCache:
            c.fill_(7.0)
        with pytest.raises(ValueError):
            d.prefill(tokens, **kw)
        torch.cuda.synchronize()
        assert int(d.pos[0]) == 3 and all(bool((c == 7.0).all()) for c in d.kCache + d.vCache)

    refused(dec, list(range(MAXTOK + 1)))
    refused(dec, prompt, pos0=MAXTOK - 3)
    small = dict(stateDim=4096, hiddenDim=4096, numLayers=1, numHeads=32, numHeadsKV=8, headDim=128, vocab=64)
    refused(Decoder(Model.random(MistralConfig(**small), seed=1, keep_cores=False), maxTokens=8), [1, 2, 3])
    refused(Decoder(Model.random(MistralConfig(numExperts=2, **small), seed=1), maxTokens=8), [1, 2, 3])
