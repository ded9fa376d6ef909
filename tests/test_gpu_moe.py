"""GPU tests of the Mixtral routing path: effort_moe_route against the three calls it replaces (bit for bit), effort_mix2_add against
effort_mix2 + an f32 add, effort_dense_gemv_expert against effort_dense_gemv on the picked expert's matrix, and the decoder with
everything folded (7 launches per layer) against the separate glue kernels (12) and the torch restatement."""
import ctypes as C

import pytest
import torch

from tests.test_gpu_decode import torch_reference
from tests.test_gpu_parity import DEV, ea  # noqa: F401  (ea: module fixture)

pytestmark = pytest.mark.gpu
P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None               # noqa: E731


def _gen(seed):
    gen = torch.Generator(device=DEV)
    gen.manual_seed(seed)
    return gen


def _route_inputs(n, numExperts, seed):
    """h heavy-tailed, norm weights with outlier channels, gate rows randn * 0.2 as f16."""
    from effort_amd.decode import structured_norm_weights
    gen = _gen(seed)
    h = torch.randn(n, generator=gen, device=DEV) * torch.exp(torch.randn(n, generator=gen, device=DEV))
    w = structured_norm_weights(n, gen, DEV)
    gate = (torch.randn((numExperts, n), generator=gen, device=DEV) * 0.2).to(torch.float16).contiguous()
    return h, w, gate


def _chain(ea, h, w, gate):
    """effort_add_rmsnorm_mul(h, NULL, w, x) -> effort_dense_gemv(gate, x) on the in-tree kernel -> effort_top2_softmax."""
    g, lib = ea.gpu(), ea.lib()
    g.set_dense_backend(False)
    g._bind_stream()
    n, E = h.numel(), gate.shape[0]
    x, logits = torch.zeros(n, device=DEV), torch.zeros(E, device=DEV)
    idx, val = torch.full((2,), -1, dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV)
    hc = h.clone()
    g.check(lib.effort_add_rmsnorm_mul(g.ctx, P(hc), None, P(w), P(x), n), "rmsnorm")
    g.check(lib.effort_dense_gemv(g.ctx, P(gate), P(x), P(logits), n, E), "dense_gemv")
    g.check(lib.effort_top2_softmax(g.ctx, P(logits), E, P(idx), P(val)), "top2")
    g.eval()
    assert torch.equal(hc, h)
    return x, logits, idx, val


def _route(ea, h, w, gate, with_logits=True):
    g, lib = ea.gpu(), ea.lib()
    g._bind_stream()
    n, E = h.numel(), gate.shape[0]
    logits = torch.full((E,), float("nan"), device=DEV) if with_logits else None
    idx, val = torch.full((2,), -1, dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV)
    hc = h.clone()
    g.check(lib.effort_moe_route(g.ctx, P(hc), P(w), P(gate), n, E, P(logits), P(idx), P(val)), "moe_route")
    g.eval()
    assert torch.equal(hc, h)                                                    # the state is read, never written
    return logits, idx, val


# (4096, 8): the norm's register path; (4112, 4): its strided path and a masked last 512-chunk; (2048, 20): more rows than waves;
# (512, 1): one expert picked twice
@pytest.mark.parametrize("n,numExperts", [(4096, 8), (4112, 4), (1024, 2), (2048, 20), (512, 1)])
def test_route_equals_the_three_call_chain(ea, n, numExperts):
    """gate_out, idx2 and val2 bit for bit against the chain.  With ONE expert the chain picks expert 0 twice with the weights
    0.5 / 0.5 (the softmax of a logit with itself; tests/test_gpu_glue.py pins top2_softmax to that), and the route reproduces what
    the chain writes."""
    h, w, gate = _route_inputs(n, numExperts, seed=n + numExperts)
    _, want_logits, want_idx, want_val = _chain(ea, h, w, gate)
    logits, idx, val = _route(ea, h, w, gate)
    assert torch.equal(logits, want_logits), (logits, want_logits)
    assert torch.equal(idx, want_idx) and torch.equal(val, want_val), (idx, want_idx, val, want_val)
    assert float(want_logits.abs().max()) > 0 and bool(torch.isfinite(want_logits).all())
    if numExperts == 1:
        assert idx.tolist() == [0, 0] and float(val[0]) + float(val[1]) == 1.0
    else:
        assert idx[0] != idx[1] and abs(float(val.sum()) - 1.0) < 1e-6 and val[0] >= val[1]


def test_route_tie_takes_the_lowest_index_first_and_runs_without_logits(ea):
    n, E = 4096, 8
    h, w, gate = _route_inputs(n, E, seed=77)
    x, _, _, _ = _chain(ea, h, w, gate)
    gate[2] = torch.sign(x).to(torch.float16) * 0.2                              # logit = 0.2 * sum |f16(x)|: far above a random row's
    gate[5] = gate[2]
    _, want_logits, want_idx, want_val = _chain(ea, h, w, gate)
    assert want_logits[2] == want_logits[5] == want_logits.max() and want_idx.tolist() == [2, 5]
    logits, idx, val = _route(ea, h, w, gate)
    assert torch.equal(logits, want_logits) and idx.tolist() == [2, 5] and torch.equal(val, want_val) and val.tolist() == [0.5, 0.5]
    _, idx0, val0 = _route(ea, h, w, gate, with_logits=False)                     # gate_out_dev = NULL
    assert torch.equal(idx0, want_idx) and torch.equal(val0, want_val)


@pytest.mark.parametrize("n,numExperts", [(4100, 8), (16400, 8), (4096, 0), (4096, 65)])
def test_route_refuses_shapes_outside_its_limits(ea, n, numExperts):
    g, lib = ea.gpu(), ea.lib()
    g._bind_stream()
    h, w, gate = _route_inputs(n, max(numExperts, 1), seed=3)
    idx, val = torch.full((2,), 1234, dtype=torch.int32, device=DEV), torch.full((2,), -7.0, device=DEV)
    rc = lib.effort_moe_route(g.ctx, P(h), P(w), P(gate), n, numExperts, None, P(idx), P(val))
    g.eval()
    assert rc in (-1, -2), rc                                                    # EFFORT_ERR_ARG / EFFORT_ERR_SHAPE
    assert idx.tolist() == [1234, 1234] and val.tolist() == [-7.0, -7.0]


@pytest.mark.parametrize("n", [4096, 1000])
def test_mix2_add_equals_mix2_then_add(ea, n):
    g, lib = ea.gpu(), ea.lib()
    g._bind_stream()
    gen = _gen(n)
    h, f0, f1 = (torch.randn(n, generator=gen, device=DEV) * s for s in (3.0, 1.0, 0.5))
    val = torch.tensor([0.6180339, 0.3819661], device=DEV)
    mix = torch.zeros(n, device=DEV)
    g.check(lib.effort_mix2(g.ctx, P(f0), P(f1), P(val), P(mix), n), "mix2")
    guard = torch.full((n + 64,), 5.0, device=DEV)                               # h with a guard band behind it
    guard[:n] = h
    g.check(lib.effort_mix2_add(g.ctx, P(guard), P(f0), P(f1), P(val), n), "mix2_add")
    g.eval()
    assert torch.equal(guard[:n], h + mix)
    assert bool((guard[n:] == 5.0).all())


# (8200, 512): the two-rows-per-wave instantiation (outDim > 8192); (1024, 4112): a masked last chunk
@pytest.mark.parametrize("outDim,inDim", [(1024, 4112), (8200, 512)])
def test_dense_gemv_expert_equals_dense_gemv_on_that_expert(ea, outDim, inDim):
    g, lib = ea.gpu(), ea.lib()
    g.set_dense_backend(False)
    g._bind_stream()
    gen = _gen(outDim)
    W = (torch.randn((3, outDim, inDim), generator=gen, device=DEV) * 0.05).to(torch.float16).contiguous()
    v = torch.randn(inDim, generator=gen, device=DEV)
    for e in (0, 2):
        want, got = torch.zeros(outDim, device=DEV), torch.full((outDim,), float("nan"), device=DEV)
        g.check(lib.effort_dense_gemv(g.ctx, P(W[e]), P(v), P(want), inDim, outDim), "dense_gemv")
        ea.basicMulExpert(v, W, torch.tensor([e], dtype=torch.int32, device=DEV), got)
        g.eval()
        assert torch.equal(got, want), e
    assert float(want.abs().max()) > 0


@pytest.fixture(scope="module")
def mixtral(ea):
    """The model of test_gpu_decode.test_mixtral_routing, its dense run and the torch restatement, shared by the tests below."""
    from effort_amd.decode import Decoder, MistralConfig, Model
    cfg = MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=2, numHeads=32, numHeadsKV=8, headDim=128, vocab=512, numExperts=4)
    model = Model.random(cfg, seed=9)
    prompt, steps = [5, 9], 8
    plain = Decoder(model, maxTokens=16)
    ids, _, logits = plain.run(prompt, steps, dense=True, collect_logits=True)
    return {"model": model, "prompt": prompt, "steps": steps, "plain": plain, "dense_ids": ids, "dense_logits": logits,
            "forced": prompt + ids[len(prompt) - 1:-1]}


def test_dense_mixtral_through_the_expert_gemv_matches_torch(mixtral):
    assert mixtral["plain"].dense_expert_gemv is True                            # (not the index_select gather)
    want_ids, want_logits = torch_reference(mixtral["model"], mixtral["prompt"], mixtral["steps"])
    assert mixtral["dense_ids"] == want_ids
    assert float((mixtral["dense_logits"] - want_logits).abs().max() / want_logits.abs().max()) < 2e-3


@pytest.mark.parametrize("effort", [1.0, 0.25])
def test_folded_mixtral_decoder_matches_the_separate_glue(mixtral, effort):
    """Decoder(fused_glue=True) on a Mixtral model (7 launches per layer) against the default (12): same tokens, logits within the
    project's bar between a folded and a separate loop, 2e-3 * max|logit|; a second run of the folded loop repeats its bits.
    (By construction -- the routing and the prologues sum in the glue kernels' orders -- the two loops should agree bit for bit on
    this model; the test prints whether they did and asserts the bar only.)"""
    from effort_amd.decode import Decoder
    model, forced, steps = mixtral["model"], mixtral["forced"], mixtral["steps"]
    plain = mixtral["plain"]
    folded = Decoder(model, maxTokens=16, fused_glue=True)
    assert folded.fused_glue and not plain.fused_glue and not Decoder(model, maxTokens=16, fused_glue=("norm",)).fused_glue
    ids_p, _, lg_p = plain.run(forced, steps, effort=effort, forced=True, collect_logits=True)
    ids_f, _, lg_f = folded.run(forced, steps, effort=effort, forced=True, collect_logits=True)
    err = float((lg_f - lg_p).abs().max() / lg_p.abs().max())
    print(f"folded vs separate at effort {effort}: rel err {err:.3e}, bit-identical {torch.equal(lg_f, lg_p)}")
    assert ids_f == ids_p
    assert err < 2e-3, err
    ids_2, _, lg_2 = folded.run(forced, steps, effort=effort, forced=True, collect_logits=True)       # replay after reset: same bits
    assert ids_2 == ids_f and torch.equal(lg_2, lg_f)


def test_sharded_and_q4_mixtral_decoders_still_refuse(mixtral):
    from effort_amd.decode import Decoder, MistralConfig, Model
    with pytest.raises(ValueError):                                              # no Q4 Mixtral model can be made, folded or not
        Model.random(MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=1, vocab=512, numExperts=4), seed=9, q4=True)
    with pytest.raises(ValueError):
        Decoder(mixtral["model"], maxTokens=16, fused_glue=True, emulate_world=True, world=2)
