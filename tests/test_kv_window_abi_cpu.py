"""CPU tests of the rolling-cache entry points (effort_amd/csrc/kv_window.hip): declared in include/effort_hip.h, bound in
effort_amd._lib._SIGS with the argument kinds the header gives them, refusing bad values -- judged before the pointers, so no context
and no GPU is needed -- with their codes in their order; and the key range of a split, the function the kernel itself calls, reached
through effort_debug_attention_window_range."""
import ctypes as C

import pytest

from tests.test_prefill_abi import ERR_ARG, ERR_SHAPE, F, I, P, _header_params

WANT = {
    "effort_rope_kv_ring": [P] * 8 + [I, I, I, I, I, F],
    "effort_rope_kv_rows_ring": [P] * 7 + [I, I, I, I, I, I, F],
    "effort_attention_window": [P] * 7 + [I, I, I, I, I, I],
    "effort_attention_block_window": [P, P, P, P, I, I, P, I, I, I, I, I],
    "effort_attention_window_default_splits": [P, I, I],
}
WINDOW, POSITIONS = 130, (0, 63, 64, 129, 130, 131, 191, 192, 193, 259, 386, 100000)


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    import effort_amd
    return effort_amd.lib()


def test_header_and_binding_agree():
    from effort_amd import _lib
    for name, kinds in WANT.items():
        assert _header_params(name) == kinds, name
        res, args = _lib._SIGS[name]
        assert res is C.c_int and [P if a is C.c_void_p else {C.c_int: I, C.c_float: F}[a] for a in args] == kinds, name


def test_refusals_and_their_order(lib):
    rope, n = C.c_float(1e6), (None,) * 8
    ring = lambda **kw: lib.effort_rope_kv_ring(*n, *(dict(dict(nh=8, nkv=2, hd=128, ringRows=96, maxPos=4096), **kw).values()), rope)            # noqa: E731
    rows_ring = lambda pos0, rows, ringRows=96, hd=128: lib.effort_rope_kv_rows_ring(*n[:7], pos0, rows, 8, 2, hd, ringRows, rope)              # noqa: E731
    attend = lambda hd=128, ringRows=96, window=96, splits=0, nkv=2: lib.effort_attention_window(*n[:7], 8, nkv, hd, ringRows, window, splits)  # noqa: E731
    block = lambda pos0, rows, ringRows=96, window=33, hd=128: lib.effort_attention_block_window(*n[:4], pos0, rows, None, 8, 2, hd, ringRows, window)   # noqa: E731
    # a good shape reaches the pointers
    assert ring() == rows_ring(0, 64) == attend() == block(0, 64) == ERR_ARG
    # the shape comes before a bad split count and before the pointers
    for bad in (dict(hd=96), dict(nkv=3), dict(ringRows=0), dict(ringRows=32769), dict(maxPos=0), dict(maxPos=1048577)):
        assert ring(**bad) == ERR_SHAPE, bad
    assert ring(maxPos=1048576) == ERR_ARG and lib.effort_rope_kv_ring(*n, 8, 2, 128, 96, 4096, C.c_float(1.0)) == ERR_SHAPE
    for bad in (dict(hd=96), dict(nkv=3), dict(window=0), dict(window=97), dict(ringRows=32769, window=5)):
        assert attend(splits=65, **bad) == ERR_SHAPE, bad
    assert attend(splits=65) == attend(splits=-1) == ERR_ARG and attend(ringRows=32768, window=32768) == ERR_ARG
    # the block forms: rows and pos0 first, then the shape -- the block's room in the ring and the last position included
    for pos0, rows in ((0, 0), (0, 65), (-1, 4)):
        assert rows_ring(pos0, rows, hd=96) == block(pos0, rows, hd=96) == ERR_ARG, (pos0, rows)
    assert block(0, 64, window=34) == ERR_SHAPE and block(0, 64, window=33) == ERR_ARG        # window + rows - 1 <= ringRows
    assert block(0, 1, window=97) == ERR_SHAPE and block(0, 4, hd=96) == ERR_SHAPE
    assert rows_ring(0, 64, ringRows=63) == ERR_SHAPE and rows_ring(0, 4, hd=96) == ERR_SHAPE
    assert rows_ring(1048576 - 4, 4) == block(1048576 - 4, 4) == ERR_ARG                      # the last block that fits
    assert rows_ring(1048576 - 3, 4) == block(1048576 - 3, 4) == ERR_SHAPE
    assert lib.effort_attention_window_default_splits(None, 8, 4096) == ERR_ARG


def ranges(lib, pos, window, S):
    out = []
    for s in range(S):
        t = (C.c_int * 2)()
        assert lib.effort_debug_attention_window_range(pos, window, S, s, t) == 0
        out.append((t[0], t[1]))
    return out


@pytest.mark.parametrize("S", (1, 3, 4, 64))
def test_split_ranges_cover_the_live_tiles(lib, S):
    for pos in POSITIONS:
        tLo, tHi = max(0, pos + 1 - WINDOW) // 64, pos // 64
        at = tLo
        for t0, t1 in ranges(lib, pos, WINDOW, S):                                # disjoint, ascending, every live tile once
            assert t0 == at and t0 <= t1, (pos, S)
            at = t1
        assert at == tHi + 1 and tHi - tLo + 1 <= (WINDOW + 63) // 64 + 1, (pos, S)
        if pos < WINDOW:                                                          # lo = 0: attention_split_tiles exactly
            for s, got in enumerate(ranges(lib, pos, WINDOW, S)):
                t = (C.c_int * 2)()
                assert lib.effort_debug_attention_split_range(pos + 1, S, s, t) == 0 and got == (t[0], t[1]), (pos, S, s)
    for bad in ((-1, 4, S, 0), (64, 0, S, 0), (64, 4, S, S), (64, 4, S, -1), (64, 4, 0, 0), (64, 4, 65, 0)):
        assert lib.effort_debug_attention_window_range(*bad, (C.c_int * 2)()) == ERR_ARG, bad
