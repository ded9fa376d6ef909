"""The wide block multiply on the GPU (effort_amd/csrc/prefill_wide.hip, effort_dense_gemm_rows_wide, ``Decoder.prefill(wide=True)``): every
row has the bits effort_dense_gemm_rows writes for it in slices of 64 (the contract that keeps the caches independent of the chunk) and
meets float64 at DENSE_BAND; refusals leave out alone; a 150-token wide block writes the caches blocks of 64 write.
"""
import numpy as np
import pytest
import torch

from tests import glue_reference as ref
from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import DEV, P, dev, gpu, lib, nans  # noqa: F401  (gpu: the fixture)
from tests.test_gpu_parity import DENSE_BAND, dense_close
from tests.util import make_v, make_w

pytestmark = pytest.mark.gpu
MAX_ROWS, SENTINEL = 256, -555.0

# (outDim, inDim, rows) and what each reaches.  A workgroup owns 128 W rows and one token group (ceil(tiles / 8) groups of equal width);
# the k split is the 64-row kernel's (stages of 256, walked here in halves of 128).
CASES = [
    (17, 32, 65),          # one live column past the old limit (5 token tiles, the last with one column); a ragged row tile
    (136, 96, 130),        # ragged in W rows against a 128-row workgroup, in tokens (two groups: 80 + 50), and a partial chunk
    (16, 1056, 256),       # full width; the last stage holds 32 live elements; 5 splits
    (1024, 4096, 200),     # 16 one-stage splits plus the reduce; token groups 112 + 88
    (4096, 4096, 256),     # even multi-stage splits: the double-buffered loop
    (16400, 512, 77),      # one split of two stages that writes out itself
    (8200, 4096, 129),     # above 64 MiB: the nt stream read by more than one token group
    (24, 64, 1),           # the old range through the new kernel
    (24, 64, 64),
]
_IN = {}


def inputs(outDim, inDim):
    """W f16 (numpy and device) and 256 heavy-tailed rows per matrix shape, made once and left unchanged."""
    if (outDim, inDim) not in _IN:
        W = make_w(outDim, inDim, seed=3)
        _IN[(outDim, inDim)] = (W, dev(W.view(np.int16)), np.stack([make_v(inDim, seed=100 + r, heavy=True) for r in range(MAX_ROWS)]))
    return _IN[(outDim, inDim)]


def call(gpu, fn, Wd, x_rows, outDim, inDim, beyond=float("nan")):
    """``fn`` on a NaN-filled out with a sentinel tail; x rows at and beyond ``rows`` hold ``beyond``.  Returns out f32 [rows][outDim]."""
    rows = len(x_rows)
    x = torch.full((rows + 3, inDim), beyond, dtype=torch.float32, device=DEV)
    x[:rows] = dev(np.ascontiguousarray(x_rows, dtype=np.float32))
    out = nans(rows * outDim + 8)
    out[rows * outDim:] = SENTINEL
    gpu.check(fn(gpu.ctx, P(Wd), P(x), P(out), inDim, outDim, rows), "dense_gemm_rows")
    gpu.eval()
    assert bool((out[rows * outDim:] == SENTINEL).all()), "wrote past rows * outDim"
    return out[:rows * outDim].view(rows, outDim)


@pytest.mark.parametrize("outDim,inDim,rows", CASES)
def test_wide_rows_have_the_64_row_kernels_bits_and_meet_float64(gpu, outDim, inDim, rows):
    W, Wd, X = inputs(outDim, inDim)
    wide = call(gpu, lib().effort_dense_gemm_rows_wide, Wd, X[:rows], outDim, inDim)
    assert bool(torch.isfinite(wide).all()), "a NaN row of x beyond `rows` (or of out) reached a result"
    again = call(gpu, lib().effort_dense_gemm_rows_wide, Wd, X[:rows], outDim, inDim, beyond=1.0)
    assert torch.equal(wide.view(torch.int32), again.view(torch.int32)), "x rows beyond `rows` changed the result"
    for r0 in range(0, rows, 64):
        old = call(gpu, lib().effort_dense_gemm_rows, Wd, X[r0:min(r0 + 64, rows)], outDim, inDim)
        assert torch.equal(wide[r0:r0 + 64].view(torch.int32), old.view(torch.int32)), f"rows {r0} .. against effort_dense_gemm_rows"
    got, worst = wide.cpu().numpy(), 0.0
    for r in sorted({r for t in range(0, rows, 16) for r in (t, min(t + 15, rows - 1))}):
        want = ref.dense(W, X[r])
        worst = max(worst, float((np.abs(got[r] - want) / (DENSE_BAND * np.abs(want).max() + DENSE_BAND * np.abs(want))).max()))
        assert dense_close(got[r], want, DENSE_BAND), (r, float(np.abs(got[r] - want).max() / np.abs(want).max()))
    print(f"dense_gemm_rows_wide ({outDim}, {inDim}, {rows}): worst error over the 1e-5 band {worst:.3g}")


def test_wide_refusals_leave_out_alone(gpu):
    _, Wd, X = inputs(24, 64)
    x, out, wide = dev(X[:2].copy()), nans(2 * 24), lib().effort_dense_gemm_rows_wide
    for rows in (0, 257, -1):
        assert wide(gpu.ctx, P(Wd), P(x), P(out), 64, 24, rows) == -1
    assert wide(gpu.ctx, P(Wd), P(x), P(out), 48, 24, 2) == -2
    assert wide(gpu.ctx, P(Wd), P(x), None, 64, 24, 2) == -1
    gpu.eval()
    assert bool(torch.isnan(out).all())


@pytest.mark.parametrize("kw,attention", [(dict(), "block"), (dict(kv_cache="f16"), "flash")])
def test_decoder_wide_prefill_writes_the_same_caches(small_model, kw, attention):  # noqa: F811
    from effort_amd.decode import Decoder
    prompt = [int(t) for t in np.random.default_rng([121]).integers(0, 512, 150)]
    dec, got = Decoder(small_model, maxTokens=160, **kw), []
    for how in (dict(chunk=150, wide=True), dict(chunk=64)):
        for c in dec.kCache + dec.vCache:
            c.fill_(float("nan"))
        dec.prefill(prompt, attention=attention, **how)
        dec.tokId.fill_(7)
        dec.token_step(dense=True)
        got.append([c[:151].clone().view(torch.int16) for c in dec.kCache + dec.vCache] + [dec.logits.clone().view(torch.int32)])
        assert bool(torch.isfinite(dec.logits).all()) and all(bool(torch.isnan(c[151:].float()).all()) for c in dec.kCache + dec.vCache)
    assert all(torch.equal(a, b) for a, b in zip(*got)), "caches or logits differ between the wide block and blocks of 64"
