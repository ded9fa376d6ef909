"""CPU tests of effort_attention_flash_group_f16 (effort_amd/csrc/attention_flash_group.hip): declared in include/effort_hip.h with
effort_attention_flash_f16's parameters and its own row limit, bound in effort_amd._lib._SIGS with the same kinds, and refusing bad
values -- judged before the pointers, so no context and no GPU is needed -- with that entry point's codes in its order."""
import ctypes as C
import re

import pytest

from tests.test_prefill_abi import ERR_ARG, ERR_SHAPE, I, P, _header_params, _header_src

WANT = [P] * 4 + [I, I, P, I, I, I, I]


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    import effort_amd
    return effort_amd.lib()


def test_header_and_binding_agree():
    from effort_amd import _lib
    assert _header_params("effort_attention_flash_group_f16") == WANT == _header_params("effort_attention_flash_f16")
    assert re.search(r"^#define EFFORT_ATTENTION_GROUP_MAX_ROWS 256$", _header_src(), flags=re.M)
    res, args = _lib._SIGS["effort_attention_flash_group_f16"]
    assert res is C.c_int and [P if a is C.c_void_p else {C.c_int: I}[a] for a in args] == WANT


def test_refusals_and_their_order(lib):
    def call(**kw):
        a = dict(dict(pos0=5, rows=130, nh=8, nkv=2, hd=128, maxTokens=600), **kw)
        return lib.effort_attention_flash_group_f16(None, None, None, None, a["pos0"], a["rows"], None, a["nh"], a["nkv"], a["hd"], a["maxTokens"])
    assert call() == call(rows=1) == call(rows=256, pos0=344) == call(maxTokens=32768) == ERR_ARG      # a good shape reaches the pointers
    for bad in (dict(rows=0), dict(rows=257), dict(pos0=-1), dict(pos0=471), dict(rows=0, hd=96)):     # the range comes first
        assert call(**bad) == ERR_ARG, bad
    for bad in (dict(hd=96), dict(nkv=3), dict(nh=0), dict(maxTokens=32769, pos0=0)):
        assert call(**bad) == ERR_SHAPE, bad
