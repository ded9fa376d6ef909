"""The FP16 bucket converter (effort_amd/csrc/convert.hip: probes, transpose, sort + bucketize, stats) at model shapes, on tied weights and
on special half values -- against tests/converter_reference.py (a numpy restatement pinned to the oracle by
tests/test_converter_reference_cpu.py) on 64 sampled input rows, and against properties that need no reference at all on every row.

Input rows convert independently, one workgroup each, so a case converts the whole matrix on the device, compares the sampled rows bit
for bit and checks the rest with tensor operations; no full-matrix CPU conversion is made.

Code paths per shape (outDim, inDim); P = the padded sort length, rep = probes per matrix row, "counted" = the literal one-lane walk
a row takes when padding ties with its zeros and leaks into the kept entries, "ranked" = the parallel rank path:

  (64, 4096)       P 64, not padded, ranked only; C = 4, the smallest the converter accepts (16 and 32 outputs: refused, C % 4); rep 64
  (4096, 4096)     P 4096, not padded, ranked only (zeros and ties or not); rep 1
  (4160, 4112)     P 8192, 4032 padding entries; both dimensions ragged (65 x 64.25 transpose tiles); counted wherever a row has a zero
  (11008, 4096)    P 16384, 5376 padding entries: `overfill` -- counted, bucket 0's half counter stopped at 2048
  (14336, 4096)    P 16384, 2048 padding entries (Mistral w1 / w3); counted for the families with zeros, `overfill` stops the counter too
  (16384, 4096)    P 16384, not padded: the largest sort, the whole of posOf[n] used; ranked only
  (4096, 14336)    P 4096, 14336 workgroups, 229376 stats rows, 224 x 64 transpose tiles (Mistral w2); ranked only
  pitched          (4160, 4096): 640-byte rows for 520 bytes of payload; (14336, 4096): the aligned pitch IS the dense one (1792)

Size limit.  One workgroup holds P * 4 + C * 17 * 2 + outDim * 2 + 16 bytes of LDS and may have 160 KiB - 64: 16384 outputs need 133136
bytes, and 16448 -- the next size the other rules allow -- pads to 32768 and would need 198936.  The entry point refuses everything above
16384 (EFFORT_ERR_CONVERT) before anything is enqueued, so the accepted / refused boundary is 16384 / 16448 by both rules.

What a padded row with zeros holds.  The counted walk is the reference's: a full bucket 0 writes on into the halfs of the buckets behind
it.  Nothing is ever out of the row's own halfs (tests/test_converter_reference_cpu.py::test_overfill_regime says why), so
convert_status() is 0 for every matrix here, but such a row no longer holds a permutation of its weights.  The reference-free properties
are therefore asserted on the rows that cannot be padded into: every row of a power-of-two outDim, and elsewhere the rows without a
zero weight.  The others are pinned by the sampled rows alone.

NaN weights are out of scope: the reference orders floats, the kernel bit patterns, and only without NaNs are the two defined to agree.
(An infinite weight at a bucket position other than 0 reads as a NaN once stored -- 0x7C00 | pos --; its bucket row's mean is then a
NaN, pinned as such, payload left open: converter_reference.stats_match.)
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import converter_reference as cr
from tests.util import cos, make_v

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL_REL = 2e-5                      # the project's bar for f32 outputs (tests/test_gpu_parity.py)
EFFORT_ERR_CONVERT = -6

CORE = ("gauss", "grid16", "extremes")
CASES = ([(4096, 4096, f) for f in cr.FAMILIES] + [(14336, 4096, f) for f in cr.FAMILIES] + [(11008, 4096, "overfill")] +
         [(o, i, f) for o, i in ((64, 4096), (16384, 4096), (4096, 14336), (4160, 4112)) for f in CORE])


@pytest.fixture(scope="module")
def ea(hip_lib_built):
    import effort_amd
    assert torch.cuda.is_available()
    effort_amd.gpu(0)
    return effort_amd


def dev16(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(DEV)


def u16(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def convert(ea, Wd):
    g = ea.gpu()
    g.convert_status()
    t = {}
    ea.bucketize(Wd.view(torch.float16), "", t)
    g.eval()
    status = g.convert_status()
    assert g.convert_status() == 0                                        # the read cleared it
    return t, status


def sampled_reference(W, rows):
    outDim = W.shape[0]
    want, dropped = cr.bucketize_rows(np.ascontiguousarray(W[:, rows].T), outDim)
    return want, dropped


def check_sampled_rows(t, W, rows, want, inDim):
    """Assertion 1: the sampled input rows, buckets and all four stat lanes, bit for bit."""
    C_ = W.shape[0] // 16
    idx = torch.from_numpy(rows).to(DEV)
    got = u16(t["buckets"].view(torch.int16).reshape(16, inDim, C_)[:, idx].permute(1, 0, 2))
    assert got.tobytes() == want.tobytes()
    st = u16(t["bucket.stats"].view(torch.int16).reshape(16, inDim, 4)[:, idx].permute(1, 0, 2))     # [row][rank][lane]
    want_st = cr.stats_rows(want, C_)
    for lane in range(4):
        assert cr.stats_match(st[:, :, lane], want_st), lane
    assert np.array_equal(st[:, :, 0], st[:, :, 1]) and np.array_equal(st[:, :, 0], st[:, :, 2]) and np.array_equal(st[:, :, 0], st[:, :, 3])


def check_properties(t, Wd, outDim, inDim):
    """Assertions 2 and 3 on every row that cannot be padded into, with no reference: the bucket entries of an input row, scattered back
    to out = bucket * 16 + (bits & 15), are a permutation of its outputs and hold W[out][in] & 0xFFF0, sign included; within a bucket
    the magnitudes do not increase from one rank to the next."""
    C_ = outDim // 16
    WT = (Wd.t().contiguous().to(torch.int32) & 0xFFFF)                                      # [in][out]
    sure = torch.ones(inDim, dtype=torch.bool, device=DEV) if cr.next_pow2(outDim) == outDim else ~((WT & 0x7FFF) == 0).any(dim=1)
    b = (t["buckets"].view(torch.int16).reshape(16, inDim, C_).permute(1, 0, 2).to(torch.int32) & 0xFFFF)     # [in][rank][bucket]
    out = (torch.arange(C_, device=DEV, dtype=torch.int64)[None, None, :] * 16 + (b & 15).to(torch.int64))
    flat_out, flat_b = out.reshape(inDim, outDim), b.reshape(inDim, outDim)
    named = torch.zeros((inDim, outDim), dtype=torch.int32, device=DEV).scatter_add_(1, flat_out, torch.ones_like(flat_b))
    assert bool((named[sure] == 1).all())
    back = torch.full((inDim, outDim), -1, dtype=torch.int32, device=DEV).scatter_(1, flat_out, flat_b & 0xFFF0)
    assert torch.equal(back[sure], (WT & 0xFFF0)[sure])
    # rank order on the weights' own magnitudes, all 15 bits (what the sort compared) ...
    mag = torch.gather(WT & 0x7FFF, 1, flat_out).reshape(inDim, 16, C_)
    assert bool((mag[sure][:, :-1] >= mag[sure][:, 1:]).all())
    # ... and on the stored ones, which have lost four bits: the weaker check, but it reads nothing except the buckets
    stored = b & 0x7FF0
    assert bool((stored[sure][:, :-1] >= stored[sure][:, 1:]).all())
    return sure


@pytest.mark.parametrize("outDim,inDim,family", CASES)
def test_converter_edges(ea, outDim, inDim, family):
    W, planted = cr.family_matrix(family, outDim, inDim)
    Wd = dev16(W)
    t, status = convert(ea, Wd)
    rows = cr.sample_rows(inDim, planted)
    assert len(rows) == 64 and set(planted) <= set(rows.tolist())
    want, dropped = sampled_reference(W, rows)
    check_sampled_rows(t, W, rows, want, inDim)
    # no write can leave a row's own halfs at any accepted size (test_overfill_regime), so the count over ALL rows is the sampled rows' count: 0
    assert status == dropped == 0
    sure = check_properties(t, Wd, outDim, inDim)
    if family in ("gauss", "equal", "extremes") or cr.next_pow2(outDim) == outDim:
        assert int(sure.sum()) >= inDim - inDim // 8                     # the properties really covered the matrix
    if family == "overfill" and cr.next_pow2(outDim) != outDim:
        assert min(cr.bucket0_visits(np.ascontiguousarray(W[:, rows[:4]].T), outDim)) > 2048          # the half counter did stop
    # assertion 4: probes[id * rep + i] = W[id][id + i]
    assert u16(t["probes"]).tobytes() == cr.probes(W).tobytes()
    if bool(sure.all()):
        from effort_amd.weights import unbucket
        U = unbucket(t["buckets"], inDim, outDim)[0].view(torch.int16).to(torch.int32) & 0xFFFF
        assert torch.equal(U & 0xFFF0, Wd.to(torch.int32) & 0xFFF0)
        assert torch.equal(U[(U & 0xFFF0) != 0] & 15, (torch.arange(outDim, device=DEV, dtype=torch.int32)[:, None] & 15).expand(outDim, inDim)[(U & 0xFFF0) != 0])


def test_size_limit(ea):
    """The first outDim the LDS formula refuses, in steps of 64 above 16384, is refused with EFFORT_ERR_CONVERT and nothing is written;
    so are 16 and 32 outputs (a bucket row of fewer than four columns).  One step below, 16384, converts: CASES has it."""
    first_refused = next(n for n in range(16384 + 64, 32768 + 64, 64) if cr.lds_bytes(n) > cr.LDS_LIMIT)
    assert first_refused == 16448 and cr.lds_bytes(first_refused - 64) <= cr.LDS_LIMIT
    assert any(o == first_refused - 64 for o, _, _ in CASES)
    import effort_amd
    lib, g = effort_amd.lib(), ea.gpu()
    g._bind_stream()
    g.convert_status()
    p = lambda x: C.c_void_p(x.data_ptr())
    for outDim in (first_refused, 16, 32):
        inDim = 4096
        W = torch.full((outDim, inDim), 0.5, dtype=torch.float16, device=DEV)
        b = torch.full((inDim * 16, max(outDim // 16, 1)), 0x5A5A, dtype=torch.int16, device=DEV)
        s = torch.full((inDim * 16, 4), 0x5A5A, dtype=torch.int16, device=DEV)
        pr = torch.full((4096,), 0x5A5A, dtype=torch.int16, device=DEV)
        assert lib.effort_convert_fp16(g.ctx, p(W), outDim, inDim, p(b), p(s), p(pr)) == EFFORT_ERR_CONVERT, outDim
        assert lib.effort_convert_fp16_pitched(g.ctx, p(W), outDim, inDim, p(b), 0, p(s), p(pr)) == EFFORT_ERR_CONVERT, outDim
        g.eval()
        assert bool((b == 0x5A5A).all()) and bool((s == 0x5A5A).all()) and bool((pr == 0x5A5A).all()), outDim
        with pytest.raises(effort_amd.EffortError) as e:
            ea.bucketize(W, "", {})
        assert e.value.code == EFFORT_ERR_CONVERT
    assert g.convert_status() == 0


@pytest.mark.parametrize("family", ["gauss", "grid16"])
@pytest.mark.parametrize("outDim,inDim", [(4160, 4096), (14336, 4096)])
def test_pitched_equals_unpitched(ea, outDim, inDim, family):
    """Assertion 5: rows effort_aligned_row_pitch bytes apart hold what the dense rows hold, the stats (read 8 bytes at a time at the
    pitch) are the same, and the padding of a destination filled with 0xFFFF is untouched."""
    import effort_amd
    lib, g = effort_amd.lib(), ea.gpu()
    W, _ = cr.family_matrix(family, outDim, inDim)
    Wd = dev16(W)
    t, _ = convert(ea, Wd)
    C_ = outDim // 16
    pitch = lib.effort_aligned_row_pitch(outDim)
    assert pitch == {4160: 640, 14336: 1792}[outDim] and pitch % 128 == 0 and pitch >= C_ * 2
    storage = torch.full((inDim * 16, pitch // 2), -1, dtype=torch.int16, device=DEV)
    stats = torch.full((inDim * 16, 4), -1, dtype=torch.int16, device=DEV)
    probes = torch.full((4096,), -1, dtype=torch.int16, device=DEV)
    p = lambda x: C.c_void_p(x.data_ptr())
    g._bind_stream()
    g.check(lib.effort_convert_fp16_pitched(g.ctx, p(Wd), outDim, inDim, p(storage), pitch, p(stats), p(probes)), "pitched")
    g.eval()
    assert g.convert_status() == 0
    assert torch.equal(storage[:, :C_], t["buckets"].view(torch.int16))
    assert bool((storage[:, C_:] == -1).all())
    assert torch.equal(stats, t["bucket.stats"].view(torch.int16)) and torch.equal(probes, t["probes"].view(torch.int16))


def close(out, want):
    tol = ATOL_REL * float(np.abs(want).max() + 1e-30)
    err = float(np.abs(out - want).max())
    print(f"max|err| {err:.3e} (bar {tol:.3e}), cos {cos(out, want):.9f}")
    return err <= tol and cos(out, want) >= 0.999999


def half_f64(bits: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(bits, dtype=np.uint16).view(np.float16).astype(np.float64)


@pytest.mark.parametrize("outDim,inDim,family", [(14336, 4096, "grid16"), (4096, 14336, "gauss"), (14336, 4096, "gauss")])
def test_closing_product(ea, outDim, inDim, family):
    """Assertion 6: the device-converted bundle, registered, through bucketMul at effort 1.0, against a float64 product.

    The multiply takes a bucket entry as the half it is, position bits included (bucketMul.metal: "a bit of noise"), so the matrix it
    multiplies by is U[out][in] = (W[out][in] & 0xFFF0) | (out & 15) -- from W alone, no converter involved -- and not W & 0xFFF0: that
    one is up to 15 / 1024 of each weight away, three decades above the bar (printed below).
    (14336, grid16) is a padded shape whose every row has zeros: the counted walk overwrites some 690 real weights of each row
    (the module docstring), as the reference does, so no product over W can hold there.  Its input is non-zero on the 64 sampled input
    rows only, and the expected product is summed from the restatement's entries of those rows.  (14336, gauss) is the same shape on
    rows the walk leaves whole: the input is zero on the few rows that hold a zero weight."""
    W, planted = cr.family_matrix(family, outDim, inDim)
    Wd = dev16(W)
    t, _ = convert(ea, Wd)
    ew = ea.ExpertWeights(t["buckets"], t["bucket.stats"], t["probes"], inSize=inDim, outSize=outDim)
    v = make_v(inDim, seed=61).astype(np.float32)
    if family == "grid16":
        rows = cr.sample_rows(inDim, planted)
        entries, _ = sampled_reference(W, rows)                                                  # [row][rank][bucket]
        keep = np.zeros(inDim, bool)
        keep[rows] = True
        v[~keep] = 0.0
        want = np.zeros(outDim, np.float64)
        outs = (np.arange(outDim // 16)[None, None, :] * 16 + (entries & 15)).reshape(len(rows), -1)
        for k, r in enumerate(rows):
            np.add.at(want, outs[k], half_f64(entries[k].reshape(-1)) * np.float64(v[r]))
    else:
        v[((W & 0x7FFF) == 0).any(axis=0)] = 0.0                                                 # (none at a power of two would matter; harmless there)
        U = (W & np.uint16(0xFFF0)) | (np.arange(outDim, dtype=np.uint16)[:, None] & np.uint16(15))
        want = half_f64(U) @ v.astype(np.float64)
        literal = half_f64(W & np.uint16(0xFFF0)) @ v.astype(np.float64)
        print(f"W & 0xFFF0 without the position bits is {float(np.abs(literal - want).max()):.3e} away from U")
    out = torch.full((outDim,), float("nan"), device=DEV)
    ea.bucketMul(torch.from_numpy(v).to(DEV), ew, None, out, 1.0)
    ea.gpu().eval()
    assert close(out.cpu().numpy().astype(np.float64), want)
