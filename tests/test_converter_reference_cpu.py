"""tests/converter_reference.py (the numpy restatement the GPU converter tests compare with) against the oracle's converter, on the CPU.

The restatement is written from the converter's description, the oracle from the reference's Metal text: the two agreeing bit for bit
on every weight family -- ties, signed zeros, padding that leaks, a stopped half counter, infinities and subnormals -- is what makes
the restatement a second opinion.  No GPU is needed.  NaN weights are out of scope (tests/converter_reference.py).
"""
import numpy as np
import pytest

from tests import converter_reference as cr

ROWS = 64


def oracle_rows(oracle_cpu, rows_u16):
    out = np.empty((rows_u16.shape[0], 16, rows_u16.shape[1] // 16), np.uint16)
    dropped = 0
    for k, row in enumerate(rows_u16):
        ranked, oob = oracle_cpu.bucketize_row(row.view(np.float16), 16)
        out[k] = ranked.view(np.uint16)
        dropped += oob
    return out, dropped


@pytest.mark.parametrize("family", cr.FAMILIES)
@pytest.mark.parametrize("outDim", [64, 1024, 1088])
def test_restatement_equals_oracle(oracle_cpu, outDim, family):
    """1088 pads to 2048 (padding can leak: the counted walk); 64 and 1024 are powers of two (never padded)."""
    W, _ = cr.family_matrix(family, outDim, ROWS)
    rows = np.ascontiguousarray(W.T)
    want, want_dropped = oracle_rows(oracle_cpu, rows)
    got, dropped = cr.bucketize_rows(rows, outDim)
    assert got.tobytes() == want.tobytes()
    assert dropped == want_dropped
    lit, lit_dropped = cr.bucketize_rows(rows, outDim, literal=True)       # the counted walk alone says the same on every row
    assert lit.tobytes() == want.tobytes() and lit_dropped == want_dropped
    visits = cr.bucket0_visits(rows, outDim)
    if outDim != 1088:
        assert max(visits) == 16
    elif family in ("grid16", "grid3", "signed_zero", "overfill"):
        assert max(visits) > 17                                            # padding leaked: the counted walk was really taken
    print(f"{family} outDim {outDim}: dropped {dropped}, bucket-0 visits up to {max(visits)}")


def test_stats_and_probes_equal_oracle(oracle_cpu):
    """The whole conversion of the smallest accepted matrix, with infinities and subnormals in it: buckets, all four stat lanes, probes."""
    outDim, inDim = 64, 4096
    W, planted = cr.family_matrix("extremes", outDim, inDim)
    b, s, p, oob = oracle_cpu.convert_fp16(W.view(np.float16))
    got, dropped = cr.bucketize_rows(np.ascontiguousarray(W.T), outDim)
    layout = np.ascontiguousarray(got.transpose(1, 0, 2)).reshape(16 * inDim, outDim // 16)       # [(rank * inDim + row)][bucket]
    assert layout.tobytes() == b.view(np.uint16).tobytes() and dropped == oob == 0
    st = cr.stats_rows(layout, outDim // 16)
    so = s.view(np.uint16)
    assert all(np.array_equal(so[:, 0], so[:, k]) for k in (1, 2, 3))
    assert cr.stats_match(st, so[:, 0])
    # an infinity at position 0 of its bucket stays one and gives an infinite mean; at position 15 it reads as a NaN (0x7C0F), and so does the mean
    assert (st == 0x7C00).sum() >= 4 and ((st & 0x7FFF) > 0x7C00).sum() >= 4
    assert np.array_equal(st[(st & 0x7FFF) <= 0x7C00], so[:, 0][(st & 0x7FFF) <= 0x7C00])
    assert cr.probes(W).tobytes() == p.view(np.uint16).tobytes()


@pytest.mark.parametrize("outDim", [11008, 14336])
def test_overfill_regime(oracle_cpu, outDim):
    """A row with more than 2048 zeros in more than 2048 padding entries: the walk visits bucket 0 more than 2048 times and its half
    counter stops at 2048 (2049 is no half), so every later visit writes the same half, 2049 -- bucket 120's.  11008 has 5376 padding
    entries; 14336 has exactly 2048, the network keeps all of them ahead of the real zeros, and bucket 0's own members take it past 2048.

    Nothing is ever DROPPED, at these or any sizes: a write is dropped past the row's C * 17 halfs, the stopped counter points at
    half 2049, and the only rows that are padded at all have C >= 260 (outDim >= 4160; below 4096 the converter takes powers of two
    only).  A full bucket 0 overwrites the halfs of the buckets behind it instead, counters included -- as the reference does.  The
    restatement and the oracle agree on that, bit for bit."""
    W, _ = cr.family_matrix("overfill", outDim, 6)
    rows = np.ascontiguousarray(W.T)
    want, want_dropped = oracle_rows(oracle_cpu, rows)
    got, dropped = cr.bucketize_rows(rows, outDim)
    visits = cr.bucket0_visits(rows, outDim)
    print(f"overfill outDim {outDim}: dropped {dropped} (oracle {want_dropped}), bucket-0 visits {visits}")
    assert got.tobytes() == want.tobytes() and dropped == want_dropped
    assert min(visits) > 2048
    assert dropped == 0 and cr.lds_bytes(outDim) <= cr.LDS_LIMIT


def test_size_limit_formula():
    """The largest sort: 16384 outputs fit the workgroup's LDS, the next multiple of 64 does not (it pads to 32768)."""
    assert cr.lds_bytes(16384) == 133136 <= cr.LDS_LIMIT
    first_refused = next(n for n in range(16384 + 64, 32768, 64) if cr.lds_bytes(n) > cr.LDS_LIMIT)
    assert first_refused == 16448 and cr.lds_bytes(16448) == 198936
