"""The calls ``Decoder.prefill(weights="buckets")`` makes, on a machine without a GPU: tests/test_prefill_trace_cpu.py's walk with every
effort_dense_gemm_rows(core) replaced by effort_bucket_gemm_rows(handle, expert 0) -- routed: effort_dense_gemm_rows_routed(cores) by
effort_bucket_gemm_rows_routed(handle) --, no core looked at, and its refusals.  The stand-in bundles get what the bucket path reads of
an ExpertWeights: ``percentLoad``, ``numExperts`` and ``handle`` (the bundle itself, so that the recorder writes its name)."""
import json

import pytest

from tests.test_decode_trace_cpu import BUNDLES
from tests.test_prefill_trace_cpu import MAX_TOKENS, ROPE, block_calls, decoder, runnable  # noqa: F401


def bucket_decoder(monkeypatch, layout="fp16", experts=1, cores=False, ok=1, **ctor):
    """A Decoder over stand-in bundles WITHOUT cores whose library answers ``ok`` to effort_weights_bucket_dense_ok."""
    rec, dec = decoder(monkeypatch, layout, experts, **ctor)
    asked = []
    for L in dec.model.layers:
        for w in BUNDLES:
            ew = getattr(L, w)
            ew.percentLoad, ew.handle = 8 if ew.q4 else 16, ew
            ew.numExperts = experts if w in ("w1", "w2", "w3") else 1
            if not cores:
                ew.core = None

    def dense_ok(handle, out):
        asked.append(handle.name)
        out._obj.value = ok
        return 0
    rec.lib_module.lib().effort_weights_bucket_dense_ok = dense_ok
    return rec, dec, asked


def watch(rec, dec):
    """Recorder.watch for a model without cores."""
    for L in dec.model.layers:
        for w in BUNDLES:
            if getattr(L, w).core is None:
                getattr(L, w).core = dec.model.norm             # (named as `norm` if it ever reached a call: it must not)
    rec.watch(dec)
    for L in dec.model.layers:
        for w in BUNDLES:
            if getattr(L, w).core is dec.model.norm:
                getattr(L, w).core = None
    rec.add("norm", dec.model.norm)


def bucket_block_calls(cfg, pos0, rows, layers=2):
    """block_calls with every core multiply turned into the bucket multiply of the same bundle."""
    calls = []
    for call in block_calls(cfg, pos0, rows, layers):
        if call[0] == "effort_dense_gemm_rows":
            _, ctx, core, x, out, _i, _o, r = call
            call = ["effort_bucket_gemm_rows", ctx, core[:-len(".core")], 0, x, out, r]
        calls.append(call)
    return calls


def routed_block_calls(cfg, pos0, rows, layers=2):
    S, H, E = cfg.stateDim, cfg.hiddenDim, cfg.numExperts
    calls = []
    for call in bucket_block_calls(cfg, pos0, rows, layers):
        if call[0] == "effort_bucket_gemm_rows" and call[2].endswith((".w1", ".w3", ".w2")):
            continue                                             # the dense FFN's three multiplies and its silu are replaced below
        if call[0] == "effort_silu_mul":
            continue
        if call[0] == "effort_add_rmsnorm_mul_rows" and call[3] == "pf_ffnOut":
            call = call[:3] + [None] + call[4:]                 # the mix landed on h: nothing is pending
        calls.append(call)
        if call[0] == "effort_add_rmsnorm_mul_rows" and call[4].endswith("ffnNorm"):
            n = int(call[4][1])
            L = f"L{n}."
            calls += [["effort_moe_route_rows", "ctx", "pf_h", L + "ffnNorm", L + "ffnGate", S, E, GATE_OUT(n, cfg), IDX2(n, cfg), "pf_gateVals", rows],
                      ["effort_bucket_gemm_rows_routed", "ctx", L + "w1", IDX2(n, cfg), "pf_norm", 0, "pf_x1r", rows],
                      ["effort_bucket_gemm_rows_routed", "ctx", L + "w3", IDX2(n, cfg), "pf_norm", 0, "pf_x3r", rows],
                      ["effort_silu_mul", "ctx", "pf_x1r", "pf_x3r", "pf_x2r", rows * 2 * H],
                      ["effort_bucket_gemm_rows_routed", "ctx", L + "w2", IDX2(n, cfg), "pf_x2r", 1, "pf_ffnOutR", rows],
                      ["effort_mix2_add_rows", "ctx", "pf_h", "pf_ffnOutR", "pf_gateVals", S, rows]]
    return calls


CHUNK = 2


def IDX2(n, cfg):                                                # layer n's rows of pf_gateIdxs [layers][chunk][2] (int32): a pointer at a byte offset
    return "pf_gateIdxs" if n == 0 else ["pf_gateIdxs", n * CHUNK * 2 * 4]


def GATE_OUT(n, cfg):
    return "pf_gateOut" if n == 0 else ["pf_gateOut", n * CHUNK * cfg.numExperts * 4]


def test_prefill_from_buckets_makes_the_block_walk_without_cores(monkeypatch):
    rec, dec, asked = bucket_decoder(monkeypatch)
    dec._prefill_buffers(CHUNK)
    watch(rec, dec)
    dec.prefill([7, 1, 30, 2, 9], chunk=CHUNK, weights="buckets")
    got = json.loads(json.dumps(rec.records))
    want = bucket_block_calls(dec.cfg, 0, 2) + bucket_block_calls(dec.cfg, 2, 2) + bucket_block_calls(dec.cfg, 4, 1)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i} of {len(want)}"
    assert len(got) == len(want)
    assert [r[0] for r in got].count("effort_bucket_gemm_rows") == 3 * (4 + 3 + 3) and "effort_dense_gemm_rows" not in [r[0] for r in got]
    assert asked == [f"L{n}.{w}" for n in range(2) for w in BUNDLES], "every handle is asked once, before the first call"
    assert int(dec.pos[0]) == 5


def test_prefill_from_buckets_routed(monkeypatch):
    rec, dec, asked = bucket_decoder(monkeypatch, experts=4)
    dec._prefill_buffers(CHUNK)
    watch(rec, dec)
    dec.prefill([3, 4, 5], chunk=CHUNK, ffn="routed", weights="buckets")
    got = json.loads(json.dumps(rec.records))
    want = routed_block_calls(dec.cfg, 0, 2) + routed_block_calls(dec.cfg, 2, 1)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i} of {len(want)}"
    assert len(got) == len(want)
    names = [r[0] for r in got]
    assert names.count("effort_bucket_gemm_rows_routed") == 2 * 3 and "effort_dense_gemm_rows_routed" not in names      # (the last layer stops at its cache write)


def test_the_default_is_the_cores_walk_call_for_call(monkeypatch):
    rec, dec, asked = bucket_decoder(monkeypatch, cores=True)
    dec._prefill_buffers(CHUNK)
    rec.watch(dec)
    dec.prefill([7, 1, 30], chunk=CHUNK)
    default = json.loads(json.dumps(rec.records))
    rec.records.clear()
    dec.prefill([7, 1, 30], chunk=CHUNK, weights="cores")
    assert json.loads(json.dumps(rec.records)) == default == block_calls(dec.cfg, 0, 2) + block_calls(dec.cfg, 2, 1)
    assert asked == []


def test_run_passes_prefill_weights_on(monkeypatch):
    import torch

    from tests.test_prefill_trace_cpu import StepGraph
    rec, dec, asked = bucket_decoder(monkeypatch, cores=True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(dec, "_graph", lambda effort, dense, sampled=False: StepGraph(dec, effort, dense, sampled))
    monkeypatch.setattr(dec, "status", lambda: 0)
    dec._prefill_buffers(CHUNK)
    rec.watch(dec)
    ids, _, _ = dec.run([1, 2, 3, 4], 5, effort=0.25, prefill=True, prefill_chunk=CHUNK, prefill_weights="buckets")
    got = json.loads(json.dumps(rec.records))
    want = bucket_block_calls(dec.cfg, 0, 2) + bucket_block_calls(dec.cfg, 2, 1)
    assert got[:len(want)] == want and ids[:3] == [-1, -1, -1]
    assert "effort_bucket_gemm_rows" not in [r[0] for r in got[len(want):]]


def test_bucket_refusals_come_before_any_call(monkeypatch):
    def refused(match, layout="fp16", experts=1, spoil=None, ok=1, cores=False, asks=0, **kw):
        ctor = {k: kw.pop(k) for k in ("world", "emulate_world") if k in kw}
        rec, dec, asked = bucket_decoder(monkeypatch, layout, experts, cores=cores, ok=ok, **ctor)
        if spoil:
            spoil(dec)
        dec.pos.fill_(1)
        kw.setdefault("weights", "buckets")
        with pytest.raises(ValueError, match=match):
            dec.prefill([1, 2, 3], chunk=CHUNK, **kw)
        assert rec.records == [] and int(dec.pos[0]) == 1 and dec._pf is None and len(asked) == asks

    refused("weights must be 'cores' or 'buckets'", weights="core")
    refused("FP16 with its buckets loaded", layout="q4ref", cores=True)                        # Q4 and core-only bundles
    refused("FP16 with its buckets loaded", layout="f16ref", cores=True)                       # FP16, but wk, wv, wo core-only
    refused("percentLoad 16", spoil=lambda dec: setattr(dec.model.layers[1].w3, "percentLoad", 8))
    refused("column-sharded", world=2, emulate_world=True)
    refused("un-bucketable", ok=0, asks=1)                                                      # the first handle's answer ends it
    refused("dense-FFN models only", experts=4)
    refused("ffn='routed' is for Mixtral", ffn="routed")
    refused("do not fit maxTokens", pos0=MAX_TOKENS - 2)
    refused("attention must be", attention="tiles")
    # the default refusals stay word for word on a model without cores
    refused("every bundle needs its f16 core", weights="cores")


def test_the_new_prototypes_agree_with_the_binding():
    """The three entry points of the bucket path: declared in the header, bound in _lib.py, with the header's arity and C types."""
    import ctypes as C

    from effort_amd import _lib
    from tests.test_abi import _prototypes
    protos = _prototypes()
    want = {"effort_weights_bucket_dense_ok": ("int", ["ptr", "ptr"]),
            "effort_bucket_gemm_rows": ("int", ["ptr", "ptr", "int", "ptr", "ptr", "int"]),
            "effort_bucket_gemm_rows_routed": ("int", ["ptr", "ptr", "ptr", "ptr", "int", "ptr", "int"])}
    for name, proto in want.items():
        assert protos[name] == proto, name
        res, args = _lib._SIGS[name]
        assert res is C.c_int and ["int" if a is C.c_int else "ptr" for a in args] == proto[1], name
