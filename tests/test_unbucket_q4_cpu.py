"""``effort_amd.weights.unbucket_q4`` -- the specification of the matrix ``Decoder.prefill(weights="q4")`` multiplies a Q4 bundle by --
against the restatement of the reference's Q4 layout (oracle/q4_layout.py: ``convert``, ``draft_mul_no_effort``), on the host.

For every bundle the converter writes: every element of U4 is named exactly once; |U4| is the mean of the bucket row that names it
and sign(U4) the weight's sign, a zero weight (+0 or -0) counting as + (the Metal kernel's reading of a clear sign bit, not the Python
draft's sign(0) == 0); and the float64 product U4 * v is the draft's effort-free multiply plus v[i // 8] * avg[i] for every zero
entry -- both are float64 sums of the same terms in another order."""
import glob
import os

import numpy as np
import pytest
import torch

from oracle import q4_layout

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def with_zeros():
    """A 40 x 160 matrix in which one entry in six is +0 and one in six is -0.0 (whole buckets of zeros among them)."""
    rng = np.random.default_rng(11)
    core2 = (rng.standard_normal((40, 160)) * 0.05).astype(np.float16)
    kind = rng.integers(0, 6, core2.shape)
    core2[kind == 0] = np.float16(0.0)
    core2[kind == 1] = np.float16(-0.0)
    core2[3, 8:16] = np.float16(-0.0)
    core2[5, 32:40] = np.float16(0.0)
    return core2, rng.standard_normal(40)


def cases():
    out = []
    for path in sorted(glob.glob(os.path.join(GOLDEN, "q4_*.npz"))):
        g = np.load(path)
        out.append(pytest.param(g["core2"], g["v"].astype(np.float64), id=os.path.basename(path)))
    out.append(pytest.param(*with_zeros(), id="zeros"))
    return out


def spec(layout, inDim, outDim):
    buckets = torch.from_numpy(layout["buckets"].view(np.int16).copy())
    stats = torch.from_numpy(layout["bucket.stats"].copy())
    from effort_amd.weights import unbucket_q4
    U = unbucket_q4(buckets, stats, inDim, outDim)
    assert U.dtype == torch.float16 and tuple(U.shape) == (1, outDim, inDim)
    return U[0].numpy()


@pytest.mark.parametrize("core2,v", cases())
def test_unbucket_q4_is_the_converters_matrix(core2, v):
    inDim, outDim = core2.shape
    assert len(q4_layout.extract_outliers(core2)[0]) > 0, "the outliers are part of the case"
    L = q4_layout.convert(core2)
    U = spec(L, inDim, outDim)
    vals, pos, avg = L["_vals_rows"], L["_pos_rows"].astype(np.int64), L["_avg"]
    nb = outDim // 8
    # bucket row i = 8 j + r, bucket b names output 8 b + pos[i][b]: every (output, input) exactly once
    i = np.arange(8 * inDim)[:, None].repeat(nb, 1)
    o = np.arange(nb)[None, :] * 8 + pos
    named = np.zeros((outDim, inDim), np.int64)
    np.add.at(named, (o, i // 8), 1)
    assert (named == 1).all()
    # |U4| is the row mean, sign(U4) the weight's sign, a zero weight +
    assert np.array_equal(np.abs(U[o, i // 8]).view(np.uint16), avg[i].view(np.uint16))
    want_minus = vals < 0
    assert np.array_equal(np.signbit(U[o, i // 8]), want_minus)
    zero = vals == 0
    assert not np.signbit(U[o, i // 8][zero]).any()
    # the float64 product: the draft's multiply plus the zero entries' +m terms
    terms = v[i // 8] * avg[i].astype(np.float64)
    want = q4_layout.draft_mul_no_effort(L, v, outDim)
    np.add.at(want, o[zero], terms[zero])
    mass = np.zeros(outDim)
    np.add.at(mass, o, np.abs(terms))
    got = U.astype(np.float64) @ v
    assert (np.abs(got - want) <= 8 * inDim * 2.0 ** -52 * mass).all()
    if zero.any():
        assert np.abs(terms[zero]).max() > 0, "the zero entries carry weight in this case"


def test_the_zero_case_has_both_zeros():
    core2, _ = with_zeros()
    kept = q4_layout.extract_outliers(core2)[1]
    assert ((kept == 0) & ~np.signbit(kept)).sum() > 100 and ((kept == 0) & np.signbit(kept)).sum() > 100


def test_what_is_not_unbucketable_raises():
    from effort_amd.weights import unbucket_q4
    g = np.load(os.path.join(GOLDEN, "q4_64x256.npz"))
    inDim, outDim = g["core2"].shape
    L = q4_layout.convert(g["core2"])
    buckets = torch.from_numpy(L["buckets"].view(np.int16).copy())
    stats = torch.from_numpy(L["bucket.stats"].copy())
    unbucket_q4(buckets, stats, inDim, outDim)
    # rank 3 of input 5, word 2, nibble 1 takes the position rank 4 holds: a duplicate, and one position unnamed
    dup = buckets.clone()
    w3, w4 = int(dup[8 * 5 + 3, 2]) & 0xFFFF, int(dup[8 * 5 + 4, 2]) & 0xFFFF
    w3 = (w3 & ~0x0700) | (w4 & 0x0700)
    dup[8 * 5 + 3, 2] = w3 - 0x10000 if w3 & 0x8000 else w3
    with pytest.raises(ValueError, match="eight different positions"):
        unbucket_q4(dup, stats, inDim, outDim)
    for bad in (1.0 + 2.0 ** -12, float("inf"), float("nan"), 1e-9):
        s = stats.clone()
        s[17, 1] = bad
        with pytest.raises(ValueError, match="finite f16 number"):
            unbucket_q4(buckets, s, inDim, outDim)
    s = stats.clone()
    s[17, 0] = float("nan")                                        # lane 0 is not read
    assert torch.equal(unbucket_q4(buckets, s, inDim, outDim).view(torch.int16), unbucket_q4(buckets, stats, inDim, outDim).view(torch.int16))
    with pytest.raises(ValueError, match="buckets"):
        unbucket_q4(buckets[:-1], stats, inDim, outDim)


def test_expert_weights_unbucket_keeps_refusing_q4():
    from effort_amd.weights import ExpertWeights
    ew = object.__new__(ExpertWeights)
    ew.q4, ew.bucketsLoaded, ew.percentLoad, ew._handle = True, True, 8, None
    with pytest.raises(ValueError, match="FP16 bundle"):
        ew.unbucket()
    ew.q4 = False
    with pytest.raises(ValueError, match="Q4 bundle"):
        ew.unbucket_q4()
