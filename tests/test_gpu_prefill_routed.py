"""Mixtral prompt prefill on the GPU: the routed block multiply (effort_amd/csrc/prefill.hip), the block forms of the routing and the
mix (effort_amd/csrc/decode.hip) and ``Decoder.prefill(..., ffn="routed")``.

  1. effort_dense_gemm_rows_routed against effort_dense_gemm_rows on the picked expert's matrix, BIT FOR BIT per assignment -- which
     hands the float64 pin of tests/test_gpu_prefill.py on to the routed kernel without a tolerance of its own.  The experts nobody picked
     hold NaN: every output finite shows that they contribute nothing.
  2. An assignment's bits do not depend on the block it sits in, its position or who else picked its expert.
  3. Refusals enqueue nothing.
  4., 5. effort_moe_route_rows / effort_mix2_add_rows are effort_moe_route / effort_mix2_add per row, bit for bit.
  6. End to end on a small three-layer Mixtral model against the token-by-token dense loop.
"""
import numpy as np
import pytest
import torch

from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import DEV, P, dev, gpu, lib, nans, within_bar  # noqa: F401  (gpu: the fixture)
from tests.test_gpu_prefill import SENTINEL, caches, min_gap, same_bits

pytestmark = pytest.mark.gpu
MAX_ROWS = 64
BAD = 0xFFFFFFFF


# ---------------------------------------------------------------- 1. the routed multiply is the block multiply on the picked expert
def routing(kind, E, rows, seed):
    """idx2 [rows][2] as int64 (entries may exceed int32: stored as uint32 bit patterns)."""
    rng = np.random.default_rng([61, seed, E, rows])
    if kind == "pair01":
        return np.tile([0, 1], (rows, 1))
    if kind == "round_robin":                      # assignment a picks expert a % E: 2 * rows / E columns each
        return (np.arange(2 * rows) % E).reshape(rows, 2)
    if kind == "skewed":                           # expert 0 takes slot 0 of the first 17 tokens (exactly 17 columns), the rest go to 1 and 2
        idx = np.empty((rows, 2), dtype=np.int64)
        idx[:, 0] = np.where(np.arange(rows) < 17, 0, 1)
        idx[:, 1] = 2
        return idx
    if kind == "random":                           # two different experts per token, as a routing gives them
        return np.stack([rng.permutation(E)[:2] for _ in range(rows)])
    if kind == "pair25":
        return np.tile([2, 5], (rows, 1))
    if kind == "pair11":
        return np.tile([1, 1], (rows, 1))
    if kind == "clamped":                          # entries past the last expert: clamped to E - 1
        idx = np.stack([rng.permutation(E - 1)[:2] for _ in range(rows)])
        idx[0, 1], idx[2, 0], idx[4, 1] = BAD, E, E + 7
        return idx
    raise AssertionError(kind)


# (outDim, inDim, E, rows, routing) and what each reaches
ROUTED_CASES = [
    (17, 32, 2, 1, "pair01"),            # smallest: one stage of 32 live elements, ragged row tile
    (24, 64, 8, 16, "round_robin"),      # six or more experts with 4 columns each
    (40, 96, 3, 33, "skewed"),           # expert 0 gets exactly 17 columns: a second token tile with one live column
    (80, 288, 4, 17, "random"),          # two stages, the second with 32 live elements
    (64, 1056, 8, 64, "random"),         # 5 splits + reduce
    (64, 1056, 8, 64, "pair25"),         # 64 columns on two experts, six NaN experts unread
    (64, 1056, 2, 64, "pair11"),         # 128 assignments on one expert: the second walk
    (64, 1056, 4, 5, "clamped"),         # entries 0xFFFFFFFF and E: clamped to E - 1
    (8200, 4096, 2, 16, "random"),       # one expert above 64 MiB: the nt stream
    (4096, 4096, 8, 64, "random"),       # a production-sized stack, 268 MB
]
_STACKS = {}


def stack_of(outDim, inDim, E):
    """f16 [E][outDim][inDim] on the device, made there; shared by the cases of a shape and left unchanged."""
    key = (outDim, inDim, E)
    if key not in _STACKS:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(outDim * 31 + inDim * 7 + E)
        _STACKS[key] = (torch.randn((E, outDim, inDim), generator=gen, device=DEV) * 0.02).to(torch.float16)
    return _STACKS[key]


def inputs_of(inDim, n, seed):
    """n heavy-tailed rows."""
    gen = torch.Generator(device=DEV)
    gen.manual_seed(1000 + seed)
    return torch.randn((n, inDim), generator=gen, device=DEV) * torch.exp(0.5 * torch.randn((n, inDim), generator=gen, device=DEV))


def idx_dev(idx, alloc_rows):
    """idx2 as the device sees it: uint32 bit patterns in an int32 tensor; entries at and beyond the live rows hold 0xFFFFFFFF."""
    full = np.full((alloc_rows, 2), BAD, dtype=np.int64)
    full[:idx.shape[0]] = idx
    return dev(full.astype(np.uint32).view(np.int32))


def routed(gpu, W, idx, x_live, xPerSlot, outDim, inDim, rows, beyond=float("nan")):
    """The call on a NaN-filled out with a sentinel tail; x rows and idx2 entries beyond the live ones hold ``beyond`` / 0xFFFFFFFF.
    Returns out f32 [rows][2][outDim]."""
    E = int(W.shape[0])
    live = (2 if xPerSlot else 1) * rows
    x = torch.full((2 * MAX_ROWS, inDim), beyond, dtype=torch.float32, device=DEV)
    x[:live] = x_live[:live]
    out = nans(2 * rows * outDim + 8)
    out[2 * rows * outDim:] = SENTINEL
    gpu.check(lib().effort_dense_gemm_rows_routed(gpu.ctx, P(W), E, P(idx_dev(idx, MAX_ROWS)), P(x), xPerSlot, P(out), inDim, outDim, rows),
              "dense_gemm_rows_routed")
    gpu.eval()
    assert bool((out[2 * rows * outDim:] == SENTINEL).all()), "wrote past 2 * rows * outDim"
    return out[:2 * rows * outDim].view(rows, 2, outDim)


def by_the_block_multiply(gpu, W, idx, x_live, xPerSlot, outDim, inDim, rows):
    """The same products through effort_dense_gemm_rows on W[e], with expert e's gathered input rows, at most 64 per call."""
    E = int(W.shape[0])
    picked = np.minimum(idx.reshape(-1), E - 1)
    want = nans(2 * rows, outDim)
    for e in sorted(set(picked.tolist())):
        a = np.nonzero(picked == e)[0]
        for c0 in range(0, len(a), MAX_ROWS):
            part = a[c0:c0 + MAX_ROWS]
            src = torch.from_numpy(part if xPerSlot else part // 2).to(DEV)
            xin = x_live[src].contiguous()
            o = nans(len(part), outDim)
            gpu.check(lib().effort_dense_gemm_rows(gpu.ctx, P(W[e]), P(xin), P(o), inDim, outDim, len(part)), "dense_gemm_rows")
            want[torch.from_numpy(part).to(DEV)] = o
    gpu.eval()
    return want.view(rows, 2, outDim)


@pytest.mark.parametrize("xPerSlot", (0, 1))
@pytest.mark.parametrize("outDim,inDim,E,rows,kind", ROUTED_CASES)
def test_routed_multiply_is_the_block_multiply_on_the_picked_expert(gpu, outDim, inDim, E, rows, kind, xPerSlot):
    clean = stack_of(outDim, inDim, E)
    idx = routing(kind, E, rows, seed=outDim + inDim)
    picked = set(np.minimum(idx.reshape(-1), E - 1).tolist())
    if kind in ("round_robin", "random") and rows >= 16:
        assert len(picked) >= min(E, 6)
    if kind == "skewed":
        assert int((idx == 0).sum()) == 17
    x = inputs_of(inDim, 2 * rows, seed=rows + xPerSlot)
    want = by_the_block_multiply(gpu, clean, idx, x, xPerSlot, outDim, inDim, rows)
    if len(picked) < E:                                    # the experts nobody picked hold NaN
        W = clean.clone()
        for e in range(E):
            if e not in picked:
                W[e] = float("nan")
    else:
        W = clean
    got = routed(gpu, W, idx, x, xPerSlot, outDim, inDim, rows)
    assert bool(torch.isfinite(got).all()), "an expert nobody picked, an x row or an idx2 entry beyond `rows` reached a result"
    assert bool(torch.isfinite(want).all())
    assert same_bits(got, want), f"{int((got != want).sum())} of {got.numel()} elements differ"
    del W


# ---------------------------------------------------------------- 2. independence from the company
def test_an_assignment_does_not_depend_on_the_block(gpu):
    outDim, inDim, E = 64, 1056, 8
    W = stack_of(outDim, inDim, E)
    idx = routing("random", E, 64, seed=5)
    x = inputs_of(inDim, 64, seed=7)
    full = routed(gpu, W, idx, x, 0, outDim, inDim, 64)
    others = routing("random", E, 64, seed=6)
    for r in (0, 15, 16, 40, 63):
        alone = routed(gpu, W, idx[r:r + 1], x[r:r + 1], 0, outDim, inDim, 1)
        assert same_bits(full[r], alone[0]), f"token {r} of 64 against the token alone"
        rows5 = [40, 41, 42, r, 43]
        idx5 = others[rows5].copy()                        # other neighbours, routed otherwise
        idx5[3] = idx[r]
        placed = routed(gpu, W, idx5, x[rows5], 0, outDim, inDim, 5)
        assert same_bits(full[r], placed[3]), f"token {r} of 64 against position 3 of 5"


# ---------------------------------------------------------------- 3. refusals enqueue nothing
def test_refusals_enqueue_nothing(gpu):
    outDim, inDim, E = 24, 64, 8
    W = stack_of(outDim, inDim, E)
    idx = idx_dev(routing("round_robin", E, 16, 0), MAX_ROWS)
    x, out = inputs_of(inDim, 32, 1), nans(2 * 16 * outDim)
    call = lambda W=W, E=E, idx=idx, x=x, per=0, out=out, i=inDim, o=outDim, rows=16: lib().effort_dense_gemm_rows_routed(   # noqa: E731
        gpu.ctx, P(W), E, P(idx), P(x), per, P(out), i, o, rows)
    assert call(rows=0) == -1 and call(rows=65) == -1
    assert call(E=0) == -1 and call(E=65) == -2
    assert call(i=48) == -2
    assert call(per=2) == -1
    assert call(out=None) == -1
    assert call(rows=65, i=48) == -1 and call(i=48, out=None) == -2            # values, then the shape, then the pointers
    assert lib().effort_dense_gemm_rows_routed(None, P(W), E, P(idx), P(x), 0, P(out), inDim, outDim, 16) == -1
    # the two glue entry points: rows, the shape, a null pointer
    n = 64
    h, w, gate = nans(16, n), dev(np.ones(n, np.float16).view(np.int16)), stack_of(1, n, E)[:, 0]
    idx2, val2 = torch.full((16, 2), 1234, dtype=torch.int32, device=DEV), nans(16, 2)
    route = lambda n=n, E=E, idx2=idx2, rows=16: lib().effort_moe_route_rows(gpu.ctx, P(h), P(w), P(gate), n, E, None, P(idx2), P(val2), rows)   # noqa: E731
    assert route(rows=0) == -1 and route(rows=65) == -1 and route(n=40) == -2 and route(E=65) == -2 and route(E=0) == -1 and route(idx2=None) == -1
    assert lib().effort_moe_route_rows(None, P(h), P(w), P(gate), n, E, None, P(idx2), P(val2), 16) == -1
    f = inputs_of(n, 32, 2)
    mix = lambda h=h, n=n, rows=16: lib().effort_mix2_add_rows(gpu.ctx, P(h), P(f), P(val2), n, rows)   # noqa: E731
    assert mix(rows=0) == -1 and mix(rows=65) == -1 and mix(n=0) == -1 and mix(h=None) == -1
    assert lib().effort_mix2_add_rows(None, P(h), P(f), P(val2), n, 16) == -1
    gpu.eval()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(h).all()) and bool(torch.isnan(val2).all()) and bool((idx2 == 1234).all())


# ---------------------------------------------------------------- 4. moe_route_rows is moe_route per row
def route_inputs(n, E, rows):
    from effort_amd.decode import structured_norm_weights
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n * 131 + E * 17 + rows)
    h = torch.randn((rows, n), generator=gen, device=DEV) * torch.exp(torch.randn((rows, n), generator=gen, device=DEV))
    w = structured_norm_weights(n, gen, DEV)
    gate = (torch.randn((E, n), generator=gen, device=DEV) * 0.2).to(torch.float16).contiguous()
    return h, w, gate


@pytest.mark.parametrize("with_logits", (True, False))
@pytest.mark.parametrize("rows", (1, 3, 17))
@pytest.mark.parametrize("n,E", [(16, 2), (992, 8), (4096, 8), (4096, 64), (5120, 2), (5120, 64), (992, 64)])
def test_moe_route_rows_is_moe_route(gpu, n, E, rows, with_logits):
    h, w, gate = route_inputs(n, E, rows)
    run_route_rows(gpu, h, w, gate, n, E, rows, with_logits)


def run_route_rows(gpu, h, w, gate, n, E, rows, with_logits):
    GUARD = 3
    hb = torch.cat([h.reshape(-1), nans(8)])               # nothing past `rows` rows of h is read
    logits = nans(rows + GUARD, E) if with_logits else None
    idx = torch.full((rows + GUARD, 2), 1234, dtype=torch.int32, device=DEV)
    val = nans(rows + GUARD, 2)
    gpu.check(lib().effort_moe_route_rows(gpu.ctx, P(hb), P(w), P(gate), n, E, P(logits), P(idx), P(val), rows), "moe_route_rows")
    logits1, idx1, val1 = nans(rows, E), torch.full((rows, 2), -1, dtype=torch.int32, device=DEV), nans(rows, 2)
    for r in range(rows):
        gpu.check(lib().effort_moe_route(gpu.ctx, P(h[r]), P(w), P(gate), n, E, P(logits1[r]), P(idx1[r]), P(val1[r])), "moe_route")
    gpu.eval()
    assert same_bits(hb[:rows * n].view(rows, n), h), "the state is read, never written"
    assert torch.equal(idx[:rows], idx1) and same_bits(val[:rows], val1)
    assert with_logits is False or same_bits(logits[:rows], logits1)
    assert bool((idx[rows:] == 1234).all()) and bool(torch.isnan(val[rows:]).all()), "rows beyond `rows` were written"
    assert with_logits is False or bool(torch.isnan(logits[rows:]).all())
    assert bool(torch.isfinite(val1).all()) and bool((idx1[:, 0] != idx1[:, 1]).all())
    return idx1, logits1


def test_moe_route_rows_breaks_a_tie_by_the_lowest_index(gpu):
    n, E, rows = 4096, 8, 17
    h, w, gate = route_inputs(n, E, rows)
    h = h.abs()                                            # the norm weights are positive, so every x = h * inv * w is: a gate row of 0.2s gives
    gate[E - 2] = 0.2                                      # the logit 0.2 * sum |f16(x)|, far above a random row's -- twice, in EVERY token
    gate[E - 1] = 0.2
    assert bool((w.float() > 0).all())
    idx, logits = run_route_rows(gpu, h, w, gate, n, E, rows, True)
    assert bool((logits[:, E - 2] == logits[:, E - 1]).all()) and bool((logits[:, E - 2] == logits.amax(dim=1)).all())
    assert idx.tolist() == [[E - 2, E - 1]] * rows


# ---------------------------------------------------------------- 5. mix2_add_rows is mix2_add per row
@pytest.mark.parametrize("rows", (1, 3, 17))
@pytest.mark.parametrize("n", (16, 4096, 5120))
def test_mix2_add_rows_is_mix2_add(gpu, n, rows):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(n + rows)
    h0 = torch.randn((rows, n), generator=gen, device=DEV) * 3.0
    f = torch.randn((rows, 2, n), generator=gen, device=DEV)
    p = torch.rand(rows, generator=gen, device=DEV)
    val = torch.stack([p, 1.0 - p], dim=1).contiguous()
    h = torch.cat([h0.reshape(-1), nans(8)])
    gpu.check(lib().effort_mix2_add_rows(gpu.ctx, P(h), P(f), P(val), n, rows), "mix2_add_rows")
    h1 = h0.clone()
    for r in range(rows):
        gpu.check(lib().effort_mix2_add(gpu.ctx, P(h1[r]), P(f[r][0]), P(f[r][1]), P(val[r]), n), "mix2_add")
    gpu.eval()
    assert same_bits(h[:rows * n].view(rows, n), h1) and bool(torch.isnan(h[rows * n:]).all())
    assert not same_bits(h1, h0)


# ---------------------------------------------------------------- 6. end to end
STEPS, MAXTOK, LAYERS, EXPERTS = 12, 32, 3, 4
MARGIN = 4e-3            # of max|logit|: the margin test_prefill_then_decode_matches_the_token_loop asks of its reference run
SEEDS = range(8)


def prompt_of(seed):
    return [int(t) for t in np.random.default_rng([43, seed]).integers(0, 512, 7)]


def routing_margin(logits):
    """Smallest gap between the 2nd and 3rd largest gate logit over [..., E], in units of that row's max|logit|."""
    top = torch.topk(logits, 3, dim=-1).values
    return float(((top[..., 1] - top[..., 2]) / logits.abs().amax(dim=-1)).min())


def kept_routing(dec, rows=6):
    """(expert pairs as sorted tuples per (layer, token), gate logits [layers - 1][rows][E]) of the last prefilled block."""
    idx = dec.pf_gateIdxs[:LAYERS - 1, :rows].cpu().tolist()
    return [[tuple(sorted(p)) for p in layer] for layer in idx], dec.pf_gateOut[:LAYERS - 1, :rows].clone()


@pytest.fixture(scope="module")
def mixtral(hip_lib_built):
    """The model, ONE decoder, the first qualifying prompt, its token-by-token dense run with the routing of every (layer, token), and
    the routed prefill's caches and routing.  Computed once."""
    from effort_amd import _lib
    from effort_amd.decode import Decoder, MistralConfig, Model
    cfg = MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=LAYERS, numHeads=32, numHeadsKV=8, headDim=128, vocab=512, numExperts=EXPERTS)
    model = Model.random(cfg, seed=11)
    dec = Decoder(model, maxTokens=MAXTOK)
    chosen = None
    for seed in SEEDS:
        prompt = prompt_of(seed)
        dec.prefill(prompt[:6], ffn="routed")
        pairs, gate = kept_routing(dec)
        if routing_margin(gate) > MARGIN:
            chosen = seed
            break
    assert chosen is not None, "no prompt seed qualifies: every one has a routed (layer, token) with an undecided second expert"
    kv_prefill = caches(dec)
    # the token loop, eagerly, with the expert pair of every (token, layer) read off the token step's own top-2 call
    l = _lib.lib()
    real, picks = l.effort_top2_softmax, []

    def spy(*args):
        rc = real(*args)
        picks.append(dec.gateIdxs.clone())
        return rc
    l.effort_top2_softmax = spy
    try:
        dec.reset()
        for t in prompt[:6]:
            dec.tokId.fill_(t)
            dec.token_step(dense=True)
    finally:
        l.effort_top2_softmax = real
    torch.cuda.synchronize()
    assert len(picks) == 6 * LAYERS
    loop_pairs = [[tuple(sorted(picks[t * LAYERS + n].cpu().tolist())) for t in range(6)] for n in range(LAYERS - 1)]
    kv_loop = caches(dec)
    ids, _, logits = dec.run(prompt, STEPS, dense=True, collect_logits=True)
    return dict(dec=dec, seed=chosen, prompt=prompt, pairs=pairs, gate=gate, kv_prefill=kv_prefill, loop_pairs=loop_pairs, kv_loop=kv_loop,
                ids=ids, logits=logits)


def test_routed_prefill_does_not_depend_on_the_chunk(mixtral):
    dec, prompt = mixtral["dec"], mixtral["prompt"]
    for attention in ("rows", "block"):
        got = []
        for chunk in (1, 4, 64):
            for c in dec.kCache + dec.vCache:
                c.fill_(float("nan"))
            dec.prefill(prompt[:6], chunk=chunk, attention=attention, ffn="routed")
            assert int(dec.pos[0]) == 6
            got.append(caches(dec))
            assert all(bool(torch.isfinite(t).all()) for pair in got[-1] for t in pair)
            assert all(bool(torch.isnan(c[6:]).all()) for c in dec.kCache + dec.vCache), "a cache row beyond the prompt was written"
        for other in got[1:]:
            for n, ((k0, v0), (k1, v1)) in enumerate(zip(got[0], other)):
                assert same_bits(k0, k1) and same_bits(v0, v1), (attention, n)
        if attention == "rows":
            for (k0, v0), (k1, v1) in zip(got[0], mixtral["kv_prefill"]):
                assert same_bits(k0, k1) and same_bits(v0, v1)


def test_routed_prefill_caches_match_the_token_loop(mixtral):
    margin = routing_margin(mixtral["gate"])
    print(f"prompt seed {mixtral['seed']}: smallest 2nd / 3rd gate-logit gap of the prefill {margin:.3g} of max|logit|")
    assert margin > MARGIN, "seed no longer qualifies: a routed (layer, token) has an undecided second expert"
    assert mixtral["pairs"] == mixtral["loop_pairs"], "the prefill routed a (layer, token) to other experts than the token loop"
    got, kv = mixtral["kv_prefill"], mixtral["kv_loop"]
    for which in (0, 1):                                             # K, V of layer 0: the norm is bit-identical, only the multiply's order differs
        assert within_bar(got[0][which].cpu().numpy(), kv[0][which].cpu().numpy()), which
        for n in range(1, LAYERS):
            a, b = got[n][which], kv[n][which]
            err = float((a - b).abs().max() / b.abs().max())
            print(f"layer {n} {'KV'[which]}: {err:.3g} of max|cache|")
            assert err < 2e-3, (n, which, err)


def test_run_with_a_routed_prefill_matches_the_token_loop(mixtral):
    dec, prompt, ids, logits = mixtral["dec"], mixtral["prompt"], mixtral["ids"], mixtral["logits"]
    P1 = len(prompt) - 1
    assert routing_margin(mixtral["gate"]) > MARGIN, "seed no longer qualifies: a routed (layer, token) has an undecided second expert"
    gap = min_gap(logits[P1:])
    print(f"smallest top-1 / top-2 gap of the compared steps: {gap:.3g} of max|logit|")
    assert gap > MARGIN, "seed no longer qualifies: the greedy comparison needs a decided reference run"
    ids_p, _, logits_p = dec.run(prompt, STEPS, dense=True, prefill=True, prefill_ffn="routed", collect_logits=True)
    assert tuple(logits_p.shape) == (STEPS - P1, logits.shape[1]) and dec.last_prefill_s > 0
    err = float((logits_p - logits[P1:]).abs().max() / logits[P1:].abs().max())
    print(f"logits after the routed prefill against the token loop: {err:.3g} of max|logit|")
    assert err < 2e-3, err
    assert ids_p[:P1] == [-1] * P1 and ids_p[P1:] == ids[P1:]


@pytest.mark.parametrize("folded", (False, True))
def test_effort_decode_after_a_routed_prefill(mixtral, folded):
    from effort_amd.decode import Decoder
    dec = mixtral["dec"] if not folded else Decoder(mixtral["dec"].model, maxTokens=MAXTOK, fused_glue=True)
    assert dec.fused_glue is folded
    ids_e, _, _ = dec.run(mixtral["prompt"], STEPS, effort=0.25, prefill=True, prefill_ffn="routed")        # run raises on a device status
    assert ids_e[:6] == [-1] * 6 and len(ids_e) == STEPS and all(0 <= t < 512 for t in ids_e[6:])


def test_routed_prefill_refusals_change_nothing(mixtral, small_model):  # noqa: F811
    from effort_amd.decode import Decoder

    def refused(d, tokens, **kw):
        d.pos.fill_(3)
        for c in d.kCache + d.vCache:
            c.fill_(7.0)
        with pytest.raises(ValueError):
            d.prefill(tokens, **kw)
        torch.cuda.synchronize()
        assert int(d.pos[0]) == 3 and all(bool((c == 7.0).all()) for c in d.kCache + d.vCache)

    refused(Decoder(small_model, maxTokens=8), [1, 2, 3], ffn="routed")
    refused(Decoder(small_model, maxTokens=8), [1, 2, 3], ffn="bogus")
    refused(mixtral["dec"], [1, 2, 3], ffn="bogus")
    refused(mixtral["dec"], [1, 2, 3])                                # the default is "dense": a Mixtral model is still refused
