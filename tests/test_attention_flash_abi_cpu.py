"""CPU tests of effort_attention_flash_f16 (effort_amd/csrc/attention_flash16.hip): declared in include/effort_hip.h, bound in
effort_amd._lib._SIGS with the argument kinds the header gives it -- effort_attention_block_f16's, one for one -- and refusing bad values,
judged before the pointers, so no context and no GPU is needed, with its codes in their order."""
import ctypes as C

import pytest

from tests.test_prefill_abi import ERR_ARG, ERR_SHAPE, I, P, _header_params

WANT = [P] * 4 + [I, I, P, I, I, I, I]


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    import effort_amd
    return effort_amd.lib()


def test_header_and_binding_agree():
    from effort_amd import _lib
    assert _header_params("effort_attention_flash_f16") == WANT == _header_params("effort_attention_block_f16")
    res, args = _lib._SIGS["effort_attention_flash_f16"]
    assert res is C.c_int and [P if a is C.c_void_p else {C.c_int: I}[a] for a in args] == WANT


def test_refusals_and_their_order(lib):
    def call(**kw):
        a = dict(dict(pos0=5, rows=17, nh=8, nkv=2, hd=128, maxTokens=600), **kw)
        return lib.effort_attention_flash_f16(None, None, None, None, a["pos0"], a["rows"], None, a["nh"], a["nkv"], a["hd"], a["maxTokens"])
    assert call() == call(rows=1) == call(rows=64, pos0=536) == call(maxTokens=32768) == ERR_ARG       # a good shape reaches the pointers
    for bad in (dict(rows=0), dict(rows=65), dict(pos0=-1), dict(pos0=584), dict(rows=0, hd=96)):      # the range comes first
        assert call(**bad) == ERR_ARG, bad
    for bad in (dict(hd=96), dict(nkv=3), dict(nh=0), dict(maxTokens=32769, pos0=0)):
        assert call(**bad) == ERR_SHAPE, bad
