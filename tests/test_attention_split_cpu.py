"""The host side of effort_attention_split (effort_amd/csrc/attention_split.h), on a machine without a GPU: the key range of a split --
the function the kernel itself calls, reached through effort_debug_attention_split_range -- and the size of the scratch."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib(hip_lib_built):
    import effort_amd
    return effort_amd.lib()


def ranges(lib, nTok, S):
    out = []
    for s in range(S):
        t = (C.c_int * 2)()
        assert lib.effort_debug_attention_split_range(nTok, S, s, t) == 0
        out.append((t[0], t[1]))
    return out


@pytest.mark.parametrize("S", list(range(1, 10)) + [64])
def test_split_ranges_partition_the_tiles(lib, S):
    for nTok in list(range(1, 301)) + [8192]:
        nTiles, at = -(-nTok // 64), 0
        per = -(-nTiles // S)
        for s, (t0, t1) in enumerate(ranges(lib, nTok, S)):
            assert t0 == at and t0 <= t1 <= nTiles, (nTok, S, s, t0, t1)                # ascending, disjoint, whole tiles
            assert t1 - t0 == per or t1 == nTiles, (nTok, S, s)                          # ceil(tiles / S) each until the tiles run out
            at = t1
        assert at == nTiles, (nTok, S)                                                   # every tile, once
    for bad in ((0, S, 0), (64, S, S), (64, S, -1), (64, 0, 0), (64, 65, 0)):
        assert lib.effort_debug_attention_split_range(*bad, (C.c_int * 2)()) == -1, bad
    assert lib.effort_debug_attention_split_range(64, S, 0, None) == -1


def test_scratch_bytes(lib):
    f = lib.effort_attention_split_scratch_bytes
    for nh, hd, S in ((32, 128, 32), (8, 64, 1), (4, 256, 64), (1, 64, 3)):
        assert f(nh, hd, S) == 4 * nh * S * (hd + 2)
    for bad in ((0, 128, 4), (32, 96, 4), (32, 128, 0), (32, 128, 65), (-1, 64, 1)):
        assert f(*bad) == 0, bad
    assert lib.effort_attention_split_default_splits(None, 8, 8192) == -1
