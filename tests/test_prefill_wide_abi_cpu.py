"""CPU tests of the wide block multiply's boundary (effort_dense_gemm_rows_wide, ``Decoder.prefill(wide=True)``): declared in
include/effort_hip.h with its row limit, bound in effort_amd._lib._SIGS, refusing bad values before it looks at a pointer, and the
Decoder's refusals before any call.  Neither a context nor a GPU is needed; nothing is computed."""
import ctypes as C

import pytest

from tests.test_prefill_abi import ERR_ARG, ERR_SHAPE, I, P, _header_params, _header_src
from tests.test_prefill_trace_cpu import decoder

NAME, KINDS = "effort_dense_gemm_rows_wide", [P, P, P, P, I, I, I]


def test_header_and_binding_have_the_wide_entry_point():
    import re

    from effort_amd import _lib
    assert _header_params(NAME) == KINDS
    assert re.search(r"#define\s+EFFORT_PREFILL_WIDE_MAX_ROWS\s+256\b", _header_src())
    assert re.search(r"#define\s+EFFORT_PREFILL_MAX_ROWS\s+64\b", _header_src())
    res, args = _lib._SIGS[NAME]
    assert res is C.c_int and [P if a is C.c_void_p else {C.c_int: I}[a] for a in args] == KINDS


def test_null_and_bad_values_return_their_codes(hip_lib_built):
    import effort_amd
    wide = effort_amd.lib().effort_dense_gemm_rows_wide
    assert wide(None, None, None, None, 4096, 4096, 256) == ERR_ARG                # values fine: the null pointers
    for rows in (0, 257, -1):
        assert wide(None, None, None, None, 4096, 4096, rows) == ERR_ARG
    assert wide(None, None, None, None, 48, 4096, 200) == ERR_SHAPE                # inDim % 32 != 0
    assert wide(None, None, None, None, 48, 4096, 257) == ERR_ARG                  # the values before the shape
    assert wide(None, None, None, None, 0, 4096, 200) == ERR_ARG


@pytest.mark.parametrize("layout,experts,kw,match", [
    ("fp16", 1, dict(chunk=257), "chunk must be 1 .. 256"),
    ("fp16", 1, dict(weights="buckets"), "wide=True serves"),
    ("q4ref", 1, dict(weights="q4"), "wide=True serves"),
    ("fp16", 4, dict(ffn="routed"), "wide=True serves"),
])
def test_decoder_refuses_before_any_call(monkeypatch, layout, experts, kw, match):
    rec, dec = decoder(monkeypatch, layout, experts)
    with pytest.raises(ValueError, match=match):
        dec.prefill([1, 2, 3], wide=True, **kw)
    assert rec.records == [] and dec._pf is None
