"""effort_attention_flash_group_f16 (effort_amd/csrc/attention_flash_group.hip, ``Decoder.prefill(attention="flash_group")``): the f16-MFMA
block attention with a GQA group's query heads sharing each K / V tile, blocks to 256 rows.  Held to float64 at the UNCHANGED bar
``within_bar`` and, bit for bit, to effort_attention_flash_f16 on the same block in slices of at most 64 rows; every cache row and q row
the kernel must not read is NaN."""
import numpy as np
import pytest
import torch

from tests.test_gpu_attention_flash import flash_call, marker_rows
from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import DEV, P, bar_figures, dev, gpu, lib, nans, within_bar  # noqa: F401
from tests.test_gpu_kv16 import want_of

pytestmark = pytest.mark.gpu


def group_call(gpu, q, K, V, pos0, nh, check=True):
    """flash_call's operands and checks for effort_attention_flash_group_f16: q [rows <= 256][nh * hd] at pos0, NaN in every cache row at or
    past pos0 + rows and every q row at or past rows.  Returns out [rows][nh * hd]."""
    rows, nkv, hd, maxTokens, caches = len(q), K.shape[1], K.shape[2], (len(K) + 63) // 64 * 64, []
    assert len(K) == pos0 + rows
    for c in (K, V):
        caches.append(torch.full((maxTokens, nkv, hd), float("nan"), dtype=torch.float16, device=DEV))
        caches[-1][:len(c)] = dev(c)
    qd, out = nans(256, nh * hd), nans(rows * nh * hd + 8)
    qd[:rows] = dev(q)
    gpu.check(lib().effort_attention_flash_group_f16(gpu.ctx, P(qd), P(caches[0]), P(caches[1]), pos0, rows, P(out), nh, nkv, hd, maxTokens),
              "attention_flash_group_f16")
    gpu.eval()
    assert bool(torch.isnan(out[rows * nh * hd:]).all()), "wrote past out[rows]"
    got = out[:rows * nh * hd].view(rows, nh * hd).cpu().numpy()
    assert np.isfinite(got).all(), "a NaN reached a result: a row that must not be read, or a masked key multiplied in"
    for r in range(rows if check else 0):
        want = want_of(q[r], K[:pos0 + r + 1], V[:pos0 + r + 1], nh)
        assert within_bar(got[r], want), (pos0, rows, r, bar_figures(got[r], want))
    return out[:rows * nh * hd].view(rows, nh * hd)


SHAPES = [(8, 1, 64), (8, 2, 128), (8, 1, 128), (4, 1, 256), (4, 2, 128), (2, 2, 128)]     # HPW 8; 4; R 8 in two head groups; HPW 2, two groups; R 2; R 1
BLOCKS = [(0, 1), (27, 17), (5, 65), (120, 130), (37, 256)]      # ...; the 64-row edge; across the waves' 128-key round and two sub-block edges; the most


@pytest.mark.parametrize("nh,nkv,hd,pos0,rows,mag", [s + b + (1.0,) for s in SHAPES for b in BLOCKS] + [(8, 2, 128) + b + (2.0 ** 6,) for b in BLOCKS])
def test_group_attention_matches_float64_and_the_sliced_flash_bits(gpu, nh, nkv, hd, pos0, rows, mag):
    rng = np.random.default_rng([131, nh, nkv, hd, pos0, rows])
    K, V = (rng.standard_normal((pos0 + rows, nkv, hd), dtype=np.float32).astype(np.float16) for _ in "kv")
    q = rng.standard_normal((rows, nh * hd), dtype=np.float32) * np.float32(mag)
    got = group_call(gpu, q, K, V, pos0, nh)                                               # (a) float64, every row
    for r0 in range(0, rows, 64):                                                          # (b) the bits of the 64-row entry point
        n = min(64, rows - r0)
        want = flash_call(gpu, q[r0:r0 + n], K[:pos0 + r0 + n], V[:pos0 + r0 + n], pos0 + r0, nh, check=False)[0]
        assert torch.equal(got[r0:r0 + n].view(torch.int32), want.view(torch.int32)), (r0, n)


@pytest.mark.parametrize("nh,hd", [(4, 128), (8, 64)])
def test_group_attention_keeps_the_heads_of_a_workgroup_apart(gpu, nh, hd):
    """One KV head, nh = HPW query heads in one workgroup.  Query r (position 64 + r) of head j finds c * q[r][j] in cache row
    32 + nh r + j: the 32 places of key tile 1 carry one (query, head)'s whole weight each; V row t is t + 1, so out[r][j] must be
    33 + nh r + j in every d.  A head that picks up another head's scores, probabilities or accumulator moves by O(1)."""
    pos0, rows, rng = 64, 32 // nh, np.random.default_rng([132, hd])
    q, K = rng.standard_normal((rows, nh * hd), dtype=np.float32), rng.standard_normal((pos0 + rows, 1, hd), dtype=np.float32).astype(np.float16)
    K[32:64, 0] = marker_rows(q, nh, hd).reshape(32, hd)
    V = np.broadcast_to(np.arange(1, pos0 + rows + 1, dtype=np.float16)[:, None, None], K.shape).copy()
    got = group_call(gpu, q, K, V, pos0, nh).view(rows, nh, hd).cpu().numpy()
    assert abs(got - np.arange(33, 65).reshape(rows, nh, 1)).max() < 1e-2, "a head's weight landed on another head's key"


def test_decoder_prefill_with_flash_group_attention(small_model):  # noqa: F811
    from effort_amd.decode import Decoder
    prompt = [int(t) for t in np.random.default_rng([133]).integers(0, 512, 150)]          # one wide block over three sub-blocks
    dec, got = Decoder(small_model, maxTokens=160, kv_cache="f16"), []
    for how in (dict(chunk=256, wide=True, attention="flash_group"), dict(chunk=64, attention="flash")):
        for c in dec.kCache + dec.vCache:
            c.fill_(float("nan"))
        dec.prefill(prompt, **how)
        dec.tokId.fill_(7)
        dec.token_step(dense=True)
        got.append([c[:151].clone().view(torch.int16) for c in dec.kCache + dec.vCache] + [dec.logits.clone().view(torch.int32)])
        assert bool(torch.isfinite(dec.logits).all()) and all(bool(torch.isnan(c[151:].float()).all()) for c in dec.kCache + dec.vCache)
    assert all(torch.equal(a, b) for a, b in zip(*got)), "caches or logits differ between 'flash_group' on a wide block and 'flash' in blocks of 64"
    for refused in (Decoder(small_model, maxTokens=64), Decoder(small_model, maxTokens=64, kv_cache="f16", window=24)):
        with pytest.raises(ValueError, match="'flash_group'"):
            refused.prefill(prompt[:40], attention="flash_group")
