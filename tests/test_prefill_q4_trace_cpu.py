"""The calls ``Decoder.prefill(weights="q4")`` makes, on a machine without a GPU: tests/test_prefill_trace_cpu.py's walk on the
reference's Q4 layout (wq, w1, w2, w3 in Q4; wk, wv, wo their cores alone) with the core multiply of every Q4 bundle replaced by
effort_q4_gemm_rows(handle, expert 0), no core of a Q4 bundle looked at, and its refusals.  The stand-in bundles get what the path
reads of an ExpertWeights: ``handle`` (the bundle itself, so that the recorder writes its name)."""
import json

import pytest

from tests.test_decode_trace_cpu import BUNDLES
from tests.test_prefill_trace_cpu import MAX_TOKENS, StepGraph, block_calls, decoder

CHUNK = 2
Q4_BUNDLES = ("wq", "w1", "w2", "w3")


def q4_decoder(monkeypatch, layout="q4ref", experts=1, cores=False, ok=1, **ctor):
    """A Decoder over stand-in bundles whose Q4 bundles have NO core and whose library answers ``ok`` to effort_weights_q4_dense_ok."""
    rec, dec = decoder(monkeypatch, layout, experts, **ctor)
    asked = []
    for L in dec.model.layers:
        for w in BUNDLES:
            ew = getattr(L, w)
            ew.percentLoad, ew.handle, ew.numExperts = 8 if ew.q4 else 16, ew, 1
            if ew.bucketsLoaded and not cores:
                ew.core = None

    def dense_ok(handle, out):
        asked.append(handle.name)
        out._obj.value = ok
        return 0
    rec.lib_module.lib().effort_weights_q4_dense_ok = dense_ok
    return rec, dec, asked


def watch(rec, dec):
    """Recorder.watch for a model whose Q4 bundles have no core."""
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


def q4_block_calls(cfg, pos0, rows, layers=2):
    """block_calls with the core multiply of every Q4 bundle turned into the Q4 multiply of the same bundle."""
    calls = []
    for call in block_calls(cfg, pos0, rows, layers):
        if call[0] == "effort_dense_gemm_rows" and call[2].split(".")[1] in Q4_BUNDLES:
            _, ctx, core, x, out, _i, _o, r = call
            call = ["effort_q4_gemm_rows", ctx, core[:-len(".core")], 0, x, out, r]
        calls.append(call)
    return calls


def test_prefill_q4_makes_the_block_walk_per_bundle(monkeypatch):
    rec, dec, asked = q4_decoder(monkeypatch)
    dec._prefill_buffers(CHUNK)
    watch(rec, dec)
    dec.prefill([7, 1, 30, 2, 9], chunk=CHUNK, weights="q4")
    got = json.loads(json.dumps(rec.records))
    want = q4_block_calls(dec.cfg, 0, 2) + q4_block_calls(dec.cfg, 2, 2) + q4_block_calls(dec.cfg, 4, 1)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"record {i} of {len(want)}"
    assert len(got) == len(want)
    names = [r[0] for r in got]
    assert names.count("effort_q4_gemm_rows") == 3 * (4 + 1) and names.count("effort_dense_gemm_rows") == 3 * (3 + 2)
    assert sorted({r[2].split(".")[1] for r in got if r[0] == "effort_q4_gemm_rows"}) == sorted(Q4_BUNDLES)
    assert sorted({r[2].split(".")[1] for r in got if r[0] == "effort_dense_gemm_rows"}) == ["wk", "wo", "wv"]
    flat = json.dumps(got)
    assert not any(f"L{n}.{w}.core" in flat for n in range(2) for w in Q4_BUNDLES), "a Q4 bundle's core was named"
    assert '"norm"' not in flat
    assert asked == [f"L{n}.{w}" for n in range(2) for w in BUNDLES if w in Q4_BUNDLES], "every Q4 handle is asked once, before the first call"
    assert int(dec.pos[0]) == 5


def test_the_default_walk_is_unchanged_call_for_call(monkeypatch):
    rec, dec, asked = q4_decoder(monkeypatch, cores=True)
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
    rec, dec, asked = q4_decoder(monkeypatch, cores=True)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(dec, "_graph", lambda effort, dense, sampled=False: StepGraph(dec, effort, dense, sampled))
    monkeypatch.setattr(dec, "status", lambda: 0)
    dec._prefill_buffers(CHUNK)
    rec.watch(dec)
    ids, _, _ = dec.run([1, 2, 3, 4], 5, effort=0.25, prefill=True, prefill_chunk=CHUNK, prefill_weights="q4")
    got = json.loads(json.dumps(rec.records))
    want = q4_block_calls(dec.cfg, 0, 2) + q4_block_calls(dec.cfg, 2, 1)
    assert got[:len(want)] == want and ids[:3] == [-1, -1, -1]
    assert "effort_q4_gemm_rows" not in [r[0] for r in got[len(want):]]
    assert len(asked) == 2 * len(Q4_BUNDLES)


def test_q4_refusals_come_before_any_call(monkeypatch):
    def refused(match, layout="q4ref", experts=1, spoil=None, ok=1, cores=False, asks=0, **kw):
        ctor = {k: kw.pop(k) for k in ("world", "emulate_world") if k in kw}
        rec, dec, asked = q4_decoder(monkeypatch, layout, experts, cores=cores, ok=ok, **ctor)
        if spoil:
            spoil(dec)
        dec.pos.fill_(1)
        kw.setdefault("weights", "q4")
        with pytest.raises(ValueError, match=match):
            dec.prefill([1, 2, 3], chunk=CHUNK, **kw)
        assert rec.records == [] and int(dec.pos[0]) == 1 and dec._pf is None and len(asked) == asks

    refused("weights must be 'cores' or 'buckets'", weights="Q4")
    refused("weights='buckets'", layout="fp16")                                                # FP16 bucketed bundles: "buckets" is their path
    refused("weights='buckets'", layout="kinds")                                               # one of them is enough
    refused("core of every core-only bundle", spoil=lambda dec: setattr(dec.model.layers[1].wv, "core", None))
    refused("un-bucketable", ok=0, asks=1)                                                     # the first handle's answer ends it
    refused("ffn='dense' alone", ffn="routed")
    refused("ffn='dense' alone", layout="fp16", experts=4, ffn="routed")
    refused("column-sharded", layout="fp16", world=2, emulate_world=True)
    refused("do not fit maxTokens", pos0=MAX_TOKENS - 2)
    refused("attention must be", attention="tiles")
    # the two older paths keep their words on a Q4 model without the cores of its Q4 bundles
    refused("every bundle needs its f16 core", weights="cores")
    refused("FP16 with its buckets loaded", weights="buckets")


def test_the_new_prototypes_agree_with_the_binding():
    """The two entry points of the Q4 path: declared in the header, bound in _lib.py, with the header's arity and C types."""
    import ctypes as C

    from effort_amd import _lib
    from tests.test_abi import _prototypes
    protos = _prototypes()
    want = {"effort_weights_q4_dense_ok": ("int", ["ptr", "ptr"]),
            "effort_q4_gemm_rows": ("int", ["ptr", "ptr", "int", "ptr", "ptr", "int"])}
    for name, proto in want.items():
        assert protos[name] == proto, name
        res, args = _lib._SIGS[name]
        assert res is C.c_int and ["int" if a is C.c_int else "ptr" for a in args] == proto[1], name
