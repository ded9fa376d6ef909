"""The calls ``Decoder.prefill`` makes (effort_amd/decode.py), on a machine without a GPU: the recorder of
tests/test_decode_trace_cpu.py stands in for the C ABI, and the expected sequence is written out here from the description of a
block's walk -- fetch; per layer norm (the pending residual added on its way) -> wq, wk, wv -> rope + cache write -> attention -> wo
-> norm -> w1, w3 -> silu -> w2; the last layer ends at its cache write -- with the operands by name."""
import json

import pytest
import torch

from tests.test_decode_trace_cpu import GOLDEN, Recorder, make_model

ROPE = 1e6
MAX_TOKENS = 8


def decoder(monkeypatch, layout="fp16", experts=1, **ctor):
    from effort_amd.decode import Decoder
    rec = Recorder().install(monkeypatch)
    dec = Decoder(make_model(layout, experts), maxTokens=MAX_TOKENS, **ctor)
    return rec, dec


def block_calls(cfg, pos0, rows, layers=2):
    """What one block of ``rows`` tokens at ``pos0`` must record on the stand-in model."""
    S, H, q = cfg.stateDim, cfg.hiddenDim, cfg.numHeads * cfg.headDim
    kv = cfg.numHeadsKV * cfg.headDim
    gemm = lambda core, x, out, i, o: ["effort_dense_gemm_rows", "ctx", core, x, out, i, o, rows]      # noqa: E731
    calls = [["effort_fetch_rows", "ctx", "tokEmbeddings", "pf_ids", "pf_h", S, rows]]
    delta = None
    for n in range(layers):
        L = f"L{n}."
        calls += [["effort_add_rmsnorm_mul_rows", "ctx", "pf_h", delta, L + "attnNorm", "pf_norm", S, rows],
                  gemm(L + "wq.core", "pf_norm", "pf_xq_temp", S, q),
                  gemm(L + "wk.core", "pf_norm", "pf_xk_temp", S, kv),
                  gemm(L + "wv.core", "pf_norm", "pf_xv_temp", S, kv),
                  ["effort_rope_kv_rows", "ctx", "pf_xq_temp", "pf_xk_temp", "pf_xv_temp", "pf_xq", f"kCache[{n}]", f"vCache[{n}]", pos0, rows,
                   cfg.numHeads, cfg.numHeadsKV, cfg.headDim, MAX_TOKENS, ROPE]]
        if n == layers - 1:
            break
        calls += [["effort_attention_rows", "ctx", "pf_xq", f"kCache[{n}]", f"vCache[{n}]", pos0, rows, "pf_attnOutput", cfg.numHeads, cfg.headDim,
                   MAX_TOKENS],
                  gemm(L + "wo.core", "pf_attnOutput", "pf_attnFfnOut", q, S),
                  ["effort_add_rmsnorm_mul_rows", "ctx", "pf_h", "pf_attnFfnOut", L + "ffnNorm", "pf_norm", S, rows],
                  gemm(L + "w1.core", "pf_norm", "pf_x1", S, H),
                  gemm(L + "w3.core", "pf_norm", "pf_x3", S, H),
                  ["effort_silu_mul", "ctx", "pf_x1", "pf_x3", "pf_x2", rows * H],
                  gemm(L + "w2.core", "pf_x2", "pf_ffnOut", H, S)]
        delta = "pf_ffnOut"
    return calls


def test_prefill_makes_the_block_walk(monkeypatch):
    rec, dec = decoder(monkeypatch)
    assert dec._pf is None and not hasattr(dec, "pf_h"), "the block buffers are made by the first prefill, not by the constructor"
    dec._prefill_buffers(2)
    assert tuple(dec.pf_h.shape) == (2, dec.cfg.stateDim) and tuple(dec.pf_x1.shape) == (2, dec.cfg.hiddenDim)
    rec.watch(dec)
    dec.prefill([7, 1, 30, 2, 9], chunk=2)
    got = json.loads(json.dumps(rec.records))
    want = block_calls(dec.cfg, 0, 2) + block_calls(dec.cfg, 2, 2) + block_calls(dec.cfg, 4, 1)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i} of {len(want)}"
    assert len(got) == len(want)
    assert got[-1][0] == "effort_rope_kv_rows" and got[-1][6:8] == ["kCache[1]", "vCache[1]"]       # the last layer ends at its cache write
    assert [r[8:10] for r in got if r[0] == "effort_rope_kv_rows" and r[6] == "kCache[0]"] == [[0, 2], [2, 2], [4, 1]]
    assert int(dec.pos[0]) == 5
    assert dec.pf_ids.tolist()[:1] == [9]                                                      # the last block's id


def test_prefill_at_a_position_and_a_second_time(monkeypatch):
    rec, dec = decoder(monkeypatch)
    dec._prefill_buffers(3)
    rec.watch(dec)
    dec.prefill([4, 5, 6, 7], pos0=3, chunk=3)
    assert json.loads(json.dumps(rec.records)) == block_calls(dec.cfg, 3, 3) + block_calls(dec.cfg, 6, 1)
    assert int(dec.pos[0]) == 7
    buf = dec.pf_h
    dec.prefill([1], chunk=2)                                                                   # a smaller block: the same buffers
    assert dec.pf_h is buf and int(dec.pos[0]) == 1


def test_a_refused_matrix_goes_row_by_row(monkeypatch):
    """EFFORT_ERR_SHAPE from the block multiply (nothing enqueued) sends THAT matrix to basicMul once per row, views of the block buffers."""
    rec, dec = decoder(monkeypatch)
    dec._prefill_buffers(2)
    rec.watch(dec)
    lib = rec.lib_module.lib()
    real = lib.effort_dense_gemm_rows

    def refuse_wk(*args):
        rc = real(*args)
        return -2 if rec.records[-1][2] == "L0.wk.core" else rc
    lib.effort_dense_gemm_rows = refuse_wk
    dec.prefill([3, 4], chunk=2)
    got = json.loads(json.dumps(rec.records))
    i = [r[:3] for r in got].index(["effort_dense_gemm_rows", "ctx", "L0.wk.core"])
    kv = dec.cfg.numHeadsKV * dec.cfg.headDim
    S = dec.cfg.stateDim
    assert got[i + 1:i + 3] == [["basicMul", ["pf_norm", 0, S], "L0.wk.core", ["pf_xk_temp", 0, kv]],
                                ["basicMul", ["pf_norm", S, S], "L0.wk.core", ["pf_xk_temp", kv, kv]]]
    assert [r[0] for r in got].count("basicMul") == 2


def test_refusals_come_before_any_call(monkeypatch):
    def refused(match, tokens=(1, 2, 3), layout="fp16", experts=1, spoil=None, pos0=0, chunk=2, **ctor):
        rec, dec = decoder(monkeypatch, layout, experts, **ctor)
        if spoil:
            spoil(dec)
        dec.pos.fill_(1)
        with pytest.raises(ValueError, match=match):
            dec.prefill(list(tokens), pos0=pos0, chunk=chunk)
        assert rec.records == [] and int(dec.pos[0]) == 1 and dec._pf is None

    refused("dense-FFN models only", experts=4)
    refused("column-sharded", world=2, emulate_world=True)
    refused("needs its f16 core", spoil=lambda dec: setattr(dec.model.layers[1].w2, "core", None))
    refused("do not fit maxTokens", tokens=range(MAX_TOKENS + 1))
    refused("do not fit maxTokens", pos0=MAX_TOKENS - 2)
    refused("do not fit maxTokens", pos0=-1)
    refused("do not fit maxTokens", tokens=())
    refused("chunk must be", chunk=0)
    refused("chunk must be", chunk=65)


# ---------------------------------------------------------------- run(): the default loop is today's, prefill=True replaces P - 1 steps
class StepGraph:
    """Stands in for the captured step: a replay makes the step's calls."""

    def __init__(self, dec, effort, dense, sampled):
        self.dec, self.args = dec, (effort, dense, True if sampled else None)

    def replay(self):
        self.dec.token_step(*self.args)


def runnable(monkeypatch):
    rec, dec = decoder(monkeypatch)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(dec, "_graph", lambda effort, dense, sampled=False: StepGraph(dec, effort, dense, sampled))
    monkeypatch.setattr(dec, "status", lambda: 0)
    dec._prefill_buffers(2)
    rec.watch(dec)
    return rec, dec


def test_run_without_prefill_is_the_token_loop(monkeypatch):
    with open(GOLDEN) as f:
        golden = json.load(f)
    rec, dec = runnable(monkeypatch)
    ids, _, _ = dec.run([1, 2, 3], 4, dense=True)
    assert json.loads(json.dumps(rec.records)) == golden["fp16-dense"] * 4
    assert len(ids) == 4 and dec.last_prefill_s is None
    rec.records.clear()
    dec.run([1, 2, 3], 4, effort=0.25)
    assert json.loads(json.dumps(rec.records)) == golden["fp16-default"] * 4


def test_run_with_prefill_replaces_the_first_steps(monkeypatch):
    with open(GOLDEN) as f:
        golden = json.load(f)
    rec, dec = runnable(monkeypatch)
    ids, _, _ = dec.run([1, 2, 3, 4], 6, effort=0.25, prefill=True, prefill_chunk=2)
    want = block_calls(dec.cfg, 0, 2) + block_calls(dec.cfg, 2, 1) + golden["fp16-default"] * 3
    assert json.loads(json.dumps(rec.records)) == want
    assert ids[:3] == [-1, -1, -1] and len(ids) == 6 and dec.last_prefill_s is not None
    rec.records.clear()
    ids, _, _ = dec.run([5], 2, dense=True, prefill=True)                                      # a prompt of one token: nothing to prefill
    assert json.loads(json.dumps(rec.records)) == golden["fp16-dense"] * 2 and -1 not in ids
    with pytest.raises(ValueError, match="forced"):
        dec.run([1, 2, 3], 3, forced=True, prefill=True)
