"""A second, independent restatement of the FP16 bucket converter (numpy only) and the weight families that strain it.

Written from the description in effort_amd/csrc/convert.hip's header and DESIGN 2, not from oracle/ (which it never calls):
tests/test_converter_reference_cpu.py pins it bit for bit to the oracle, tests/test_gpu_converter_edges.py pins the HIP converter to it.

One INPUT row (a column of the HF matrix W [outDim, inDim]: the outDim weights one input feeds) is converted on its own:

  1. the row's (bits, output index) pairs are padded with (0, index 0) to P = the next power of two >= outDim;
  2. the compare-exchange network runs over them: for p in 0..log2(P)-1, for q in 0..p, every position gid with bit 2^(p-q) clear
     meets gid | 2^(p-q), and the two are exchanged iff (|a| < |b|) == (((gid >> p) & 2) == 0), |x| being the 15 magnitude bits.
     The result descends by magnitude; the network is not stable, so equal magnitudes land where the network leaves them;
  3. the first outDim sorted entries are kept and walked in order.  An entry with index i belongs to bucket i // 16 at position
     i % 16; it becomes (bits & 0xFFF0) | position and takes the next free rank of its bucket;
  4. when index 0 shows up more than once among the kept entries (zero padding that tied with real zeros), the walk is the
     reference's literal one: the row owns C * 17 halfs, bucket b's counter at b * 17 and its ranks behind it; the counter is a HALF that
     gains 1.0 per visit (and stops at 2048, where 2049 rounds back), the entry is written at b * 17 + 1 + ushort(counter) -- into
     the next buckets' halfs when bucket 0 is full -- and a write past C * 17 is counted as dropped.

NaN weights are out of scope everywhere here: the reference orders floats and the kernel orders bit patterns, and the two are only
defined to agree without NaNs.
"""
from __future__ import annotations

import functools

import numpy as np

B = 16                                   # outputs per bucket of the FP16 layout


def next_pow2(n: int) -> int:
    p = 1
    while p < n:
        p <<= 1
    return p


@functools.lru_cache(maxsize=None)
def _network(P: int):
    """The compare-exchange stages for P entries: a list of (lower positions, upper positions, ascending?)."""
    logn = P.bit_length() - 1
    m = np.arange(P // 2, dtype=np.int64)
    stages = []
    for p in range(logn):
        for q in range(p + 1):
            sh = p - q
            lo = ((m >> sh) << (sh + 1)) | (m & ((1 << sh) - 1))
            stages.append((lo, lo | (1 << sh), ((lo >> p) & 2) == 0))
    return stages


def sort_rows(rows_u16: np.ndarray):
    """[R, n] row bits -> (sorted bits [R, n], their output indices [R, n]): steps 1-3's first half, all rows at once."""
    rows_u16 = np.ascontiguousarray(rows_u16, dtype=np.uint16)
    R, n = rows_u16.shape
    P = next_pow2(n)
    # one 64-bit word per entry: magnitude | bits | index -- only the magnitude field is ever compared
    key = np.zeros((R, P), np.uint64)
    v = rows_u16.astype(np.uint64)
    key[:, :n] = ((v & np.uint64(0x7FFF)) << np.uint64(32)) | (v << np.uint64(16)) | np.arange(n, dtype=np.uint64)[None, :]
    for lo, hi, asc in _network(P):
        a, b = key[:, lo], key[:, hi]
        swap = ((a >> np.uint64(32)) < (b >> np.uint64(32))) == asc[None, :]
        key[:, lo] = np.where(swap, b, a)
        key[:, hi] = np.where(swap, a, b)
    key = key[:, :n]
    return ((key >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.uint16), (key & np.uint64(0xFFFF)).astype(np.uint16)


@functools.lru_cache(maxsize=None)
def _half_tables():
    """(counter half + 1.0 as a half, counter half as a ushort) for every half bit pattern."""
    with np.errstate(all="ignore"):
        f = np.arange(65536, dtype=np.uint32).astype(np.uint16).view(np.float16).astype(np.float32)
        inc = (f + np.float32(1.0)).astype(np.float16).view(np.uint16)
        u = np.where(f > 0, np.minimum(np.nan_to_num(f, nan=0.0, posinf=65535.0), np.float32(65535.0)), np.float32(0.0))
    return inc.tolist(), np.floor(u).astype(np.int64).tolist()


def walk_counted(vals: np.ndarray, idxs: np.ndarray, C: int):
    """Step 4, literally, for one row -> (ranks [16, C], dropped, visits of bucket 0)."""
    inc, ushort = _half_tables()
    lim = C * (B + 1)
    bv = [0] * lim
    dropped = visits0 = 0
    for v, i in zip(vals.tolist(), idxs.tolist()):
        off = (i // B) * (B + 1)
        slot = off + 1 + ushort[bv[off]]
        if slot < lim:
            bv[slot] = (v & 0xFFF0) | (i % B)
        else:
            dropped += 1
        bv[off] = inc[bv[off]]
        visits0 += off == 0
    a = np.asarray(bv, np.uint16).reshape(C, B + 1)
    return np.ascontiguousarray(a[:, 1:].T), dropped, visits0


def walk_ranked(vals: np.ndarray, idxs: np.ndarray, C: int) -> np.ndarray:
    """Step 3 for one row whose kept indices are all different: the running rank inside each bucket, without the loop."""
    n = C * B
    bkt = (idxs // B).astype(np.int64)
    order = np.argsort(bkt, kind="stable")                   # bucket by bucket, each in walk order
    rank = np.empty(n, np.int64)
    rank[order] = np.arange(n) % B                           # every bucket has exactly 16 members
    out = np.empty((B, C), np.uint16)
    out[rank, bkt] = (vals & np.uint16(0xFFF0)) | (idxs % B).astype(np.uint16)
    return out


def bucketize_rows(W_rows_u16: np.ndarray, outDim: int, literal: bool = False):
    """[R, outDim] input rows (bits) -> (rank rows u16 [R, 16, C], dropped).  ``literal``: take the counted walk for every row."""
    W_rows_u16 = np.ascontiguousarray(W_rows_u16, dtype=np.uint16).reshape(-1, outDim)
    assert outDim % B == 0
    C = outDim // B
    out = np.empty((W_rows_u16.shape[0], B, C), np.uint16)
    dropped = 0
    for r0 in range(0, W_rows_u16.shape[0], 16):             # (a few rows at a time: the sort holds 8 bytes per padded entry)
        vals, idxs = sort_rows(W_rows_u16[r0:r0 + 16])
        for k in range(vals.shape[0]):
            if literal or int((idxs[k] == 0).sum()) != 1:
                out[r0 + k], d, _ = walk_counted(vals[k], idxs[k], C)
                dropped += d
            else:
                out[r0 + k] = walk_ranked(vals[k], idxs[k], C)
    return out, dropped


def bucket0_visits(W_rows_u16: np.ndarray, outDim: int) -> list[int]:
    """How often each row's walk visits bucket 0 (16 unless padding leaked; above 2048 its half counter has stopped)."""
    vals, idxs = sort_rows(np.ascontiguousarray(W_rows_u16, dtype=np.uint16).reshape(-1, outDim))
    return [int((idxs[k] < B).sum()) for k in range(vals.shape[0])]


def stats_rows(rank_rows: np.ndarray, C: int) -> np.ndarray:
    """[..., C] bucket rows (bits) -> their stat (bits): the f32 sum of |x| in column order, / float32(C), rounded to half."""
    with np.errstate(all="ignore"):
        a = np.abs(np.ascontiguousarray(rank_rows, dtype=np.uint16).view(np.float16).astype(np.float32))
        s = np.cumsum(a, axis=-1, dtype=np.float32)[..., -1]          # cumsum adds left to right; np.sum would pair up
        return (s / np.float32(C)).astype(np.float16).view(np.uint16)


def stats_match(a_u16: np.ndarray, b_u16: np.ndarray) -> bool:
    """Stat bits equal -- or NaN on both sides.  An infinite weight at a position other than 0 turns into a NaN once the position
    replaces its low mantissa bits (0x7C00 | 15), and its bucket row's mean is then a NaN whose payload no one defines (numpy
    keeps it, the oracle's conversion clears it): which rows have a NaN mean is pinned, its payload is not."""
    a, b = np.asarray(a_u16, np.uint16), np.asarray(b_u16, np.uint16)
    nan_a, nan_b = (a & 0x7FFF) > 0x7C00, (b & 0x7FFF) > 0x7C00
    return bool(np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a], b[~nan_b]))


def probes(W_u16: np.ndarray) -> np.ndarray:
    """probes[id * rep + i] = W[id][id + i], rep = 4096 / outDim below 4096 outputs and 1 from there."""
    outDim = W_u16.shape[0]
    rep = 1 if outDim >= 4096 else 4096 // outDim
    ids = np.arange(4096 // rep)
    out = np.empty(4096, np.uint16)
    for i in range(rep):
        out[ids * rep + i] = W_u16[ids, ids + i]
    return out


def lds_bytes(outDim: int) -> int:
    """What one workgroup of the sort asks for: values and indices of the padded row, the 17-half buckets, the rank rows, a counter."""
    return next_pow2(outDim) * 4 + (outDim // B) * (B + 1) * 2 + outDim * 2 + 16


LDS_LIMIT = 160 * 1024 - 64


# ---------------------------------------------------------------- weight families
FAMILIES = ("gauss", "grid16", "grid3", "equal", "signed_zero", "overfill", "extremes")

# +-65504, +-Inf, the smallest and the largest subnormal, the smallest normal
SPECIALS = (0x7BFF, 0xFBFF, 0x7C00, 0xFC00, 0x0001, 0x03FF, 0x0400)


def _bits(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.float16)).view(np.uint16)


def family_matrix(family: str, outDim: int, inDim: int, seed: int = 2024):
    """(W bits u16 [outDim, inDim], the input rows that carry planted values) of one family; every value is an exact half.

    gauss        N(0, 0.02^2): the control.
    grid16       k / 16 * 0.05, k in -8..8: 17 levels, nearly every comparison of the sort a tie (a de-quantised int4 checkpoint).
    grid3        -a, 0, +a a third each: the zeros tie with the padding of a non-power-of-two row.
    equal        an input row's weights all the same: +x on even input rows, -x on odd ones.
    signed_zero  +0 / -0 at random, five non-zero weights per input row.
    overfill     Gaussian, three weights in ten zeroed (+0 / -0): with more than 2048 padding entries the walk visits bucket 0 more
                 than 2048 times and its half counter stops.
    extremes     Gaussian with each of SPECIALS planted at positions 0 and 15 of the first and of the last bucket, every
                 (special, place) pair in an input row of its own, and one more input row that has them all.
    """
    rng = np.random.default_rng(seed + 7919 * FAMILIES.index(family))
    planted: list[int] = []
    if family in ("gauss", "overfill", "extremes"):
        W = _bits(rng.standard_normal((outDim, inDim), dtype=np.float32) * np.float32(0.02)).copy()
        if family == "overfill":
            z = rng.random((outDim, inDim), dtype=np.float32)
            W[z < 0.15] = 0x0000
            W[(z >= 0.15) & (z < 0.3)] = 0x8000
        elif family == "extremes":
            places = sorted({0, B - 1, outDim - B, outDim - 1})
            pairs = [(s, o) for s in SPECIALS for o in places]
            rows = rng.choice(inDim, len(pairs) + 1, replace=False)
            for (s, o), r in zip(pairs, rows):
                W[o, r] = s
            for k, s in enumerate(SPECIALS):                      # the last row: every special at once, spread over the places
                W[places[k % len(places)] ^ (k // len(places)), rows[-1]] = s
            planted = sorted(int(r) for r in rows)
    elif family == "grid16":
        W = _bits(rng.integers(-8, 9, (outDim, inDim)).astype(np.float32) / np.float32(16) * np.float32(0.05)).copy()
    elif family == "grid3":
        W = _bits(rng.integers(-1, 2, (outDim, inDim)).astype(np.float32) * np.float32(0.03)).copy()
    elif family == "equal":
        x = _bits(np.float16(0.0371))
        W = np.empty((outDim, inDim), np.uint16)
        W[:, 0::2] = x
        W[:, 1::2] = x | np.uint16(0x8000)
    elif family == "signed_zero":
        W = (rng.integers(0, 2, (outDim, inDim)).astype(np.uint16) << np.uint16(15))
        o = rng.integers(0, outDim, (5, inDim))
        W[o, np.arange(inDim)[None, :]] = _bits(rng.standard_normal((5, inDim), dtype=np.float32) * np.float32(0.02) + np.float32(0.001))
    else:
        raise ValueError(family)
    assert not ((W & 0x7FFF) > 0x7C00).any()                      # no NaN
    return W, planted


def sample_rows(inDim: int, planted, seed: int = 5, count: int = 64) -> np.ndarray:
    """The input rows compared bit for bit: the first four, the last four, every planted row, the rest seeded at random."""
    rows = list(dict.fromkeys([0, 1, 2, 3, inDim - 4, inDim - 3, inDim - 2, inDim - 1] + [int(r) for r in planted]))
    assert len(rows) <= count
    for r in np.random.default_rng(seed).permutation(inDim).tolist():
        if len(rows) >= min(count, inDim):
            break
        if r not in rows:
            rows.append(r)
    return np.asarray(sorted(rows), np.int64)
