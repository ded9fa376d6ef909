"""CPU tests of effort_rope_attention_f16 (effort_amd/csrc/kv16_short.hip): declared in include/effort_hip.h, bound in
effort_amd._lib._SIGS with the argument kinds the header gives it, and refusing bad values -- judged before the pointers, so no context
and no GPU is needed -- with its codes in their order."""
import ctypes as C

import pytest

from tests.test_prefill_abi import ERR_ARG, ERR_SHAPE, F, I, P, _header_params

WANT = [P] * 8 + [I, I, I, I, I, F]


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    import effort_amd
    return effort_amd.lib()


def test_header_and_binding_agree():
    from effort_amd import _lib
    assert _header_params("effort_rope_attention_f16") == WANT
    res, args = _lib._SIGS["effort_rope_attention_f16"]
    assert res is C.c_int and [P if a is C.c_void_p else {C.c_int: I, C.c_float: F}[a] for a in args] == WANT


def test_refusals_and_their_order(lib):
    def call(rope=1e6, **kw):
        shape = dict(dict(nh=8, nkv=2, hd=128, cacheRows=600, maxKeys=520), **kw)
        return lib.effort_rope_attention_f16(*(None,) * 8, *shape.values(), C.c_float(rope))
    assert call() == call(maxKeys=1) == call(cacheRows=32768, maxKeys=2048) == call(maxKeys=600) == ERR_ARG      # a good shape reaches the pointers
    for bad in (dict(hd=96), dict(nkv=3), dict(maxKeys=0), dict(cacheRows=4096, maxKeys=2049), dict(maxKeys=601), dict(cacheRows=32769),
                dict(cacheRows=0), dict(rope=1.0)):
        assert call(**bad) == ERR_SHAPE, bad
