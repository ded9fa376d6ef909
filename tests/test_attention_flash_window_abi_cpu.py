"""CPU tests of effort_attention_flash_window (effort_amd/csrc/attention_flash_window.hip): declared in include/effort_hip.h with
effort_attention_block_window's parameters, one for one, bound in effort_amd._lib._SIGS with the same kinds, and refusing what it
refuses with the same code -- the values are judged before the pointers, so no context and no GPU is needed."""
import ctypes as C

import pytest

from tests.test_prefill_abi import ERR_ARG, ERR_SHAPE, I, P, _header_params

WANT = [P, P, P, P, I, I, P, I, I, I, I, I]


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    import effort_amd
    return effort_amd.lib()


def test_header_and_binding_agree():
    from effort_amd import _lib
    assert _header_params("effort_attention_flash_window") == WANT == _header_params("effort_attention_block_window")
    res, args = _lib._SIGS["effort_attention_flash_window"]
    assert res is C.c_int and [P if a is C.c_void_p else {C.c_int: I}[a] for a in args] == WANT
    assert _lib._SIGS["effort_attention_block_window"] == (res, args)


GOOD = dict(pos0=200, rows=64, nh=8, nkv=2, hd=128, ringRows=96, window=33)


@pytest.mark.parametrize("change,code", [
    (dict(), ERR_ARG), (dict(rows=1, window=96), ERR_ARG), (dict(pos0=1048576 - 64), ERR_ARG),          # a good shape reaches the pointers
    (dict(rows=0), ERR_ARG), (dict(rows=65), ERR_ARG), (dict(rows=0, hd=96), ERR_ARG), (dict(pos0=-1), ERR_ARG),   # rows and pos0 come first
    (dict(hd=96), ERR_SHAPE), (dict(nkv=3), ERR_SHAPE), (dict(rows=1, window=97), ERR_SHAPE),           # window > ringRows
    (dict(window=34), ERR_SHAPE),                                                                       # window - 1 > ringRows - rows
    (dict(ringRows=32769), ERR_SHAPE), (dict(pos0=1048576 - 63), ERR_SHAPE)])
def test_refusals_are_the_block_window_kernels(lib, change, code):
    a = dict(GOOD, **change)
    args = (None,) * 4 + (a["pos0"], a["rows"], None, a["nh"], a["nkv"], a["hd"], a["ringRows"], a["window"])
    assert lib.effort_attention_flash_window(*args) == code == lib.effort_attention_block_window(*args), change
