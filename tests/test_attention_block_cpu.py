"""effort_attention_block without a GPU: declared in include/effort_hip.h with effort_attention_rows's arguments, bound in
effort_amd._lib._SIGS, exported by the library and refusing bad arguments with effort_attention_rows's codes (values before shape
before pointers: no context is needed); and where ``Decoder.prefill`` / ``Decoder.run`` put it -- with the recorder of
tests/test_decode_trace_cpu.py standing in for the C ABI."""
import ctypes as C
import json

import pytest

from tests.test_prefill_abi import ERR_ARG, ERR_SHAPE, I, P, _header_params
from tests.test_prefill_trace_cpu import block_calls, decoder, runnable

NAME = "effort_attention_block"
KINDS = [P, P, P, P, I, I, P, I, I, I]


# ---------------------------------------------------------------- the ABI
def test_header_and_binding_declare_it_like_attention_rows():
    from effort_amd import _lib
    assert _header_params(NAME) == KINDS == _header_params("effort_attention_rows")
    res, args = _lib._SIGS[NAME]
    assert res is C.c_int and [P if a is C.c_void_p else {C.c_int: I}[a] for a in args] == KINDS
    assert _lib._SIGS[NAME] == _lib._SIGS["effort_attention_rows"]


def test_refusals_without_a_context(hip_lib_built):
    """Every refusal of effort_attention_rows, the same code for the same arguments."""
    import effort_amd
    lib = effort_amd.lib()
    block, rows_ = lib.effort_attention_block, lib.effort_attention_rows
    cases = [((0, 16, None, 8, 128, 32), ERR_ARG)]                                       # nothing wrong but the null pointers
    cases += [((0, rows, None, 8, 128, 128), ERR_ARG) for rows in (0, 65, -1)]           # rows outside 1 .. 64
    cases += [((pos0, rows, None, 8, 128, maxTokens), ERR_ARG)                           # pos0 < 0, pos0 + rows > maxTokens
              for pos0, rows, maxTokens in ((-1, 4, 32), (29, 4, 32), (32, 1, 32), (0, 33, 32), (2147483647, 2, 32))]
    cases += [((28, 4, None, 8, hd, 32), ERR_SHAPE) for hd in (96, 32, 512, 0)]          # headDim other than 64 / 128 / 256
    cases += [((0, 4, None, 8, 128, 8193), ERR_SHAPE)]                                   # maxTokens > 8192
    cases += [((0, 65, None, 8, 96, 8193), ERR_ARG)]                                     # the range is judged before the shape
    for tail, code in cases:
        assert block(None, None, None, None, *tail) == code, tail
        assert rows_(None, None, None, None, *tail) == code, tail
    assert block(None, None, None, None, 28, 4, None, 8, 128, 32) == ERR_ARG             # the last block of a cache is legal: only the pointers are wrong


# ---------------------------------------------------------------- where the Decoder puts it
def with_block(calls):
    return [[NAME] + c[1:] if c[0] == "effort_attention_rows" else c for c in calls]


def test_prefill_block_attention_replaces_that_one_call(monkeypatch):
    rec, dec = decoder(monkeypatch)
    dec._prefill_buffers(2)
    rec.watch(dec)
    dec.prefill([7, 1, 30, 2, 9], chunk=2, attention="block")
    want = block_calls(dec.cfg, 0, 2) + block_calls(dec.cfg, 2, 2) + block_calls(dec.cfg, 4, 1)
    assert sum(c[0] == "effort_attention_rows" for c in want) == 3
    assert json.loads(json.dumps(rec.records)) == with_block(want)
    assert int(dec.pos[0]) == 5
    rec.records.clear()
    dec.prefill([7, 1, 30, 2, 9], chunk=2)                                               # the default: today's sequence
    assert json.loads(json.dumps(rec.records)) == want
    rec.records.clear()
    dec.prefill([7, 1, 30, 2, 9], 0, 2, "rows")
    assert json.loads(json.dumps(rec.records)) == want


def test_an_unknown_attention_is_refused_before_any_call(monkeypatch):
    rec, dec = decoder(monkeypatch)
    dec.pos.fill_(1)
    for bad in ("flash", "", None, "Block"):
        with pytest.raises(ValueError, match="attention must be"):
            dec.prefill([1, 2, 3], chunk=2, attention=bad)
        assert rec.records == [] and int(dec.pos[0]) == 1 and dec._pf is None


def test_run_passes_the_choice_through(monkeypatch):
    rec, dec = runnable(monkeypatch)
    ids, _, _ = dec.run([1, 2, 3, 4], 6, effort=0.25, prefill=True, prefill_chunk=2, prefill_attention="block")
    got = json.loads(json.dumps(rec.records))
    n = len(block_calls(dec.cfg, 0, 2) + block_calls(dec.cfg, 2, 1))
    assert got[:n] == with_block(block_calls(dec.cfg, 0, 2) + block_calls(dec.cfg, 2, 1))
    assert NAME not in [c[0] for c in got[n:]] and ids[:3] == [-1, -1, -1]
    rec.records.clear()
    dec.run([1, 2, 3, 4], 6, effort=0.25, prefill=True, prefill_chunk=2)                 # the default stays effort_attention_rows
    assert json.loads(json.dumps(rec.records))[:n] == block_calls(dec.cfg, 0, 2) + block_calls(dec.cfg, 2, 1)
    rec.records.clear()
    with pytest.raises(ValueError, match="attention must be"):
        dec.run([1, 2, 3, 4], 6, prefill=True, prefill_attention="flash")
    assert rec.records == []
