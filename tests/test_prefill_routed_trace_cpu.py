"""The calls ``Decoder.prefill(..., ffn="routed")`` makes on a Mixtral model (effort_amd/decode.py), on a machine without a GPU: the
recorder of tests/test_decode_trace_cpu.py stands in for the C ABI, and the expected sequence is written out here from the description
of a routed block's walk -- fetch; per layer norm (the pending residual added on its way; after a routed FFN nothing is pending) ->
wq, wk, wv -> rope + cache write -> attention -> wo -> norm -> moe_route_rows -> routed w1, routed w3 (both slots read the token's
normed state) -> silu over rows * 2 * hiddenDim -> routed w2 (a gated vector per slot) -> mix2_add_rows on the block's h; the last
layer ends at its cache write -- with the operands by name."""
import json

import pytest

from tests.test_decode_trace_cpu import Recorder, make_model

ROPE = 1e6
MAX_TOKENS = 8
EXPERTS = 4


def decoder(monkeypatch, experts=EXPERTS, **ctor):
    from effort_amd.decode import Decoder
    rec = Recorder().install(monkeypatch)
    dec = Decoder(make_model("fp16", experts), maxTokens=MAX_TOKENS, **ctor)
    return rec, dec


def routed_block_calls(cfg, pos0, rows, chunk, attention="effort_attention_rows", layers=2):
    """What one routed block of ``rows`` tokens at ``pos0`` must record on the stand-in model whose block buffers hold ``chunk`` rows."""
    S, H, q, E = cfg.stateDim, cfg.hiddenDim, cfg.numHeads * cfg.headDim, cfg.numExperts
    kv = cfg.numHeadsKV * cfg.headDim
    gemm = lambda core, x, out, i, o: ["effort_dense_gemm_rows", "ctx", core, x, out, i, o, rows]      # noqa: E731
    calls = [["effort_fetch_rows", "ctx", "tokEmbeddings", "pf_ids", "pf_h", S, rows]]
    for n in range(layers):
        L = f"L{n}."
        calls += [["effort_add_rmsnorm_mul_rows", "ctx", "pf_h", None, L + "attnNorm", "pf_norm", S, rows],
                  gemm(L + "wq.core", "pf_norm", "pf_xq_temp", S, q),
                  gemm(L + "wk.core", "pf_norm", "pf_xk_temp", S, kv),
                  gemm(L + "wv.core", "pf_norm", "pf_xv_temp", S, kv),
                  ["effort_rope_kv_rows", "ctx", "pf_xq_temp", "pf_xk_temp", "pf_xv_temp", "pf_xq", f"kCache[{n}]", f"vCache[{n}]", pos0, rows,
                   cfg.numHeads, cfg.numHeadsKV, cfg.headDim, MAX_TOKENS, ROPE]]
        if n == layers - 1:
            break
        # layer n's rows of the kept routing: a pointer is named by its buffer, and by [buffer, offset in bytes] past its start
        idx2 = ["pf_gateIdxs", n * chunk * 2 * 4] if n else "pf_gateIdxs"
        logits = ["pf_gateOut", n * chunk * E * 4] if n else "pf_gateOut"
        routed = lambda core, x, per_slot, out, i, o: ["effort_dense_gemm_rows_routed", "ctx", core, E, idx2, x, per_slot, out, i, o, rows]   # noqa: E731
        calls += [[attention, "ctx", "pf_xq", f"kCache[{n}]", f"vCache[{n}]", pos0, rows, "pf_attnOutput", cfg.numHeads, cfg.headDim, MAX_TOKENS],
                  gemm(L + "wo.core", "pf_attnOutput", "pf_attnFfnOut", q, S),
                  ["effort_add_rmsnorm_mul_rows", "ctx", "pf_h", "pf_attnFfnOut", L + "ffnNorm", "pf_norm", S, rows],
                  ["effort_moe_route_rows", "ctx", "pf_h", L + "ffnNorm", L + "ffnGate", S, E, logits, idx2, "pf_gateVals", rows],
                  routed(L + "w1.core", "pf_norm", 0, "pf_x1r", S, H),
                  routed(L + "w3.core", "pf_norm", 0, "pf_x3r", S, H),
                  ["effort_silu_mul", "ctx", "pf_x1r", "pf_x3r", "pf_x2r", rows * 2 * H],
                  routed(L + "w2.core", "pf_x2r", 1, "pf_ffnOutR", H, S),
                  ["effort_mix2_add_rows", "ctx", "pf_h", "pf_ffnOutR", "pf_gateVals", S, rows]]
    return calls


def test_routed_prefill_makes_the_routed_block_walk(monkeypatch):
    rec, dec = decoder(monkeypatch)
    assert dec._pf is None and not hasattr(dec, "pf_x1r"), "the block buffers are made by the first prefill, not by the constructor"
    dec._prefill_buffers(2)
    cfg = dec.cfg
    assert tuple(dec.pf_x1r.shape) == (2, 2, cfg.hiddenDim) and tuple(dec.pf_ffnOutR.shape) == (2, 2, cfg.stateDim)
    assert tuple(dec.pf_gateIdxs.shape) == (cfg.numLayers, 2, 2) and tuple(dec.pf_gateOut.shape) == (cfg.numLayers, 2, EXPERTS)
    rec.watch(dec)
    dec.prefill([7, 1, 30, 2, 9], chunk=2, ffn="routed")
    got = json.loads(json.dumps(rec.records))
    want = routed_block_calls(cfg, 0, 2, 2) + routed_block_calls(cfg, 2, 2, 2) + routed_block_calls(cfg, 4, 1, 2)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i} of {len(want)}"
    assert len(got) == len(want)
    assert got[-1][0] == "effort_rope_kv_rows" and got[-1][6:8] == ["kCache[1]", "vCache[1]"]       # the last layer ends at its cache write
    assert "basicMul" not in [r[0] for r in got] and "basicMulExpert" not in [r[0] for r in got]
    assert int(dec.pos[0]) == 5


def test_block_attention_with_the_routed_ffn(monkeypatch):
    rec, dec = decoder(monkeypatch)
    dec._prefill_buffers(3)
    rec.watch(dec)
    dec.prefill([4, 5, 6, 7], pos0=3, chunk=3, attention="block", ffn="routed")
    want = routed_block_calls(dec.cfg, 3, 3, 3, "effort_attention_block") + routed_block_calls(dec.cfg, 6, 1, 3, "effort_attention_block")
    assert json.loads(json.dumps(rec.records)) == want
    assert int(dec.pos[0]) == 7


def test_a_refused_stack_goes_assignment_by_assignment(monkeypatch):
    """EFFORT_ERR_SHAPE from the routed multiply (nothing enqueued) sends THAT stack to basicMulExpert once per assignment: the slot's
    input, the stack, the slot's expert number on the device, the slot's output."""
    rec, dec = decoder(monkeypatch)
    dec._prefill_buffers(2)
    rec.watch(dec)
    lib = rec.lib_module.lib()
    real = lib.effort_dense_gemm_rows_routed

    def refuse_w2(*args):
        rc = real(*args)
        return -2 if rec.records[-1][2] == "L0.w2.core" else rc
    lib.effort_dense_gemm_rows_routed = refuse_w2
    dec.prefill([3, 4], chunk=2, ffn="routed")
    got = json.loads(json.dumps(rec.records))
    i = [r[:3] for r in got].index(["effort_dense_gemm_rows_routed", "ctx", "L0.w2.core"])
    S, H = dec.cfg.stateDim, dec.cfg.hiddenDim
    want = [["basicMulExpert", ["pf_x2r", a * H, H], "L0.w2.core", ["pf_gateIdxs", a, 1], ["pf_ffnOutR", a * S, S]] for a in range(4)]
    assert got[i + 1:i + 5] == want
    assert got[i + 5][0] == "effort_mix2_add_rows" and [r[0] for r in got].count("basicMulExpert") == 4


def test_routed_refusals_come_before_any_call(monkeypatch):
    def refused(match, experts=EXPERTS, spoil=None, ffn="routed", **ctor):
        rec, dec = decoder(monkeypatch, experts, **ctor)
        if spoil:
            spoil(dec)
        dec.pos.fill_(1)
        with pytest.raises(ValueError, match=match):
            dec.prefill([1, 2, 3], chunk=2, ffn=ffn)
        assert rec.records == [] and int(dec.pos[0]) == 1 and dec._pf is None

    refused("ffn='routed' is for Mixtral models", experts=1)
    refused("ffn='routed' is for Mixtral models", experts=1, world=2, emulate_world=True)      # (a sharded decoder is a dense-FFN one)
    refused("needs its f16 core", spoil=lambda dec: setattr(dec.model.layers[0].w3, "core", None))
    refused("expert stacks' cores", spoil=lambda dec: setattr(dec.model.layers[1].w2, "core", dec.model.layers[1].w2.core[0]))
    refused("ffn must be 'dense' or 'routed'", ffn="bogus")
    refused("ffn must be 'dense' or 'routed'", experts=1, ffn="bogus")
    refused("dense-FFN models only", ffn="dense")                                               # the default is today's refusal


def test_run_hands_prefill_ffn_on(monkeypatch):
    import torch

    from tests.test_prefill_trace_cpu import StepGraph
    rec, dec = decoder(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(dec, "_graph", lambda effort, dense, sampled=False: StepGraph(dec, effort, dense, sampled))
    monkeypatch.setattr(dec, "status", lambda: 0)
    dec._prefill_buffers(2)
    rec.watch(dec)
    with pytest.raises(ValueError, match="dense-FFN models only"):
        dec.run([1, 2, 3, 4], 6, dense=True, prefill=True, prefill_chunk=2)
    rec.records.clear()
    ids, _, _ = dec.run([1, 2, 3, 4], 6, dense=True, prefill=True, prefill_chunk=2, prefill_ffn="routed")
    got = json.loads(json.dumps(rec.records))
    want = routed_block_calls(dec.cfg, 0, 2, 2) + routed_block_calls(dec.cfg, 2, 1, 2)
    assert got[:len(want)] == want and got[len(want)][0] == "effort_fetch_row"
    assert ids[:3] == [-1, -1, -1] and len(ids) == 6
