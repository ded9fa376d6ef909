"""Prefill straight from the Q4 buckets on the GPU (effort_amd/csrc/prefill_q4.hip, Decoder.prefill(weights="q4")).

The contract is BITS for the multiply: on a handle without outliers effort_q4_gemm_rows writes what effort_dense_gemm_rows writes when
the un-bucketed matrix (``effort_amd.weights.unbucket_q4``, pinned to the converter's layout by tests/test_unbucket_q4_cpu.py) is given
to it as the core -- and that kernel is pinned to float64 by tests/test_gpu_prefill.py.  The outlier term is a chain of f32 fmaf
steps in the order of the handle's index; it is held to the rounding bound of such a chain in either order, doubled, and to being the
same bits whatever the block holds.

The bundles are built directly (the converter reaches a small part of what registration accepts): random nibbles with a random
permutation of the eight positions per bucket, random f16 means in stats lane 1 -- lane 0 holds another number, so a read of the
wrong lane shows."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_glue import DEV, P, gpu, lib  # noqa: F401  (gpu: the fixture)
from tests.test_gpu_prefill_buckets import ERR_ARG, ERR_CONVERT, ERR_KIND, ERR_SHAPE, MAX_ROWS, SENTINEL, core_rows, fresh_out, padded_x, same_bits, x_rows

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- bundles
def deal_q4(E, outDim, inDim, gen):
    """Random Q4 words int16 [E, 8 * in, out / 32]: per (e, j, bucket of 8 outputs) a random permutation of the positions over the
    eight ranks, random signs."""
    nb = outDim // 8
    pos = torch.rand((E, inDim, nb, 8), generator=gen, device=DEV).argsort(3).to(torch.int32)          # [e][j][b][rank]
    sign = (torch.rand((E, inDim, nb, 8), generator=gen, device=DEV) < 0.5).to(torch.int32)
    nib = (sign * 8 + pos).permute(0, 1, 3, 2).reshape(E, inDim * 8, nb)                                # row 8 j + rank
    w = (nib[..., 0::4] << 12) | (nib[..., 1::4] << 8) | (nib[..., 2::4] << 4) | nib[..., 3::4]
    return ((w ^ 0x8000) - 0x8000).to(torch.int16).contiguous()


class Q4Bundle:
    """A registered Q4 bundle built directly.  ``ew.buckets`` [E, 8 * in, out / 32] and ``ew.stats`` [E, 8 * in, 2] are what the
    handle reads: rewrite them in place, then ``ew.refresh()``."""

    def __init__(self, outDim, inDim, E=1, seed=0, outliers=None):
        from effort_amd.weights import ExpertWeights
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed * 1000003 + outDim * 31 + inDim)
        words = deal_q4(E, outDim, inDim, gen)
        mean = (0.002 + 0.04 * torch.rand((E, 8 * inDim), generator=gen, device=DEV)).to(torch.float16).float()
        stats = torch.stack([mean * 3.0 + 1.0, mean], dim=2).contiguous()
        probes = (torch.randn((E, 4096), generator=gen, device=DEV) * 0.02).to(torch.float16)
        self.ew = ExpertWeights(words, stats, probes, inDim, outDim, None, E, outliers=outliers, q4=True)
        assert self.ew.buckets.data_ptr() == words.data_ptr() and self.ew.stats.data_ptr() == stats.data_ptr()
        self.outDim, self.inDim, self.E, self.gen = outDim, inDim, E, gen

    @property
    def U(self):
        """unbucket_q4() of the bundle as it is NOW: f16 [E, out, in]."""
        return self.ew.unbucket_q4()


def q4_rows(gpu, ew, expert, x, rows, expect=0):
    """The call with NaN x rows past ``rows`` on a NaN out with a sentinel tail.  Returns out [rows][outDim] (or the return code)."""
    n = rows * ew.outSize if 1 <= rows <= MAX_ROWS else 8
    out = fresh_out(n)
    rc = lib().effort_q4_gemm_rows(gpu.ctx, ew.handle, expert, P(padded_x(x, max(0, min(rows, MAX_ROWS)))), P(out), rows)
    gpu.eval()
    assert rc == expect, (rc, expect)
    assert bool((out[n:] == SENTINEL).all()), "wrote past rows * outDim"
    if expect:
        assert bool(torch.isnan(out[:n]).all()), "a refused call wrote to out"
        return rc
    return out[:n].view(rows, ew.outSize)


def dense_ok(gpu, ew):
    ok = C.c_int(-1)
    gpu.check(lib().effort_weights_q4_dense_ok(ew.handle, C.byref(ok)), "weights_q4_dense_ok")
    return ok.value


# ---------------------------------------------------------------- 1. bits
# (outDim, inDim, rows) and what each reaches.  A bucket row is outDim / 32 words; a workgroup owns 16 of them (512 outputs); the row
# pieces are 16-byte loads when the word count is a multiple of 8, else 2-byte loads; the k split is the core kernel's.
BIT_SHAPES = [
    (32, 4096, 1),          # one word per row
    (96, 4096, 16),         # three words: 2-byte-aligned rows
    (1056, 4096, 17),       # 33 words: a ragged last workgroup of one word, one live column in the second token tile
    (64, 4128, 5),          # a last stage of 32 live k
    (4096, 4096, 64),       # the wq shape
    (1024, 14336, 64),      # the longest K
    (16384, 4096, 16),      # the widest output, above the nt threshold
]


@pytest.mark.parametrize("outDim,inDim,rows", BIT_SHAPES)
def test_q4_multiply_is_the_core_multiply_on_the_unbucketed_matrix(gpu, outDim, inDim, rows):
    b = Q4Bundle(outDim, inDim)
    x = x_rows(inDim)
    got = q4_rows(gpu, b.ew, 0, x, rows)
    want = core_rows(gpu, b.U[0], x, rows)
    assert bool(torch.isfinite(got).all()), "stale LDS, an x row past `rows` or a dead k reached a result"
    assert same_bits(got, want)


# ---------------------------------------------------------------- 2. masking and independence
def test_a_row_does_not_depend_on_the_block(gpu):
    b = Q4Bundle(1056, 4096)
    x = x_rows(4096)
    full = q4_rows(gpu, b.ew, 0, x, 64)
    assert same_bits(full, core_rows(gpu, b.U[0], x, 64))
    for rows in (1, 5, 16, 17, 64):
        assert same_bits(q4_rows(gpu, b.ew, 0, x, rows), full[:rows]), rows
    alone = q4_rows(gpu, b.ew, 0, x[40:41], 1)               # row 40 as a block of its own
    assert same_bits(alone, full[40:41])


def test_other_experts_are_not_read(gpu):
    """Experts 0 and 1 get NaN means and other nibbles (still permutations), in place and WITHOUT a refresh: a refresh would judge
    the handle again and refuse NaN means.  The compact means of the handle are the first check's, so the NaN shows only through a
    read of the stats, the nibbles through a read of another expert's rows."""
    b = Q4Bundle(96, 4096, E=3)
    x = x_rows(4096)
    assert dense_ok(gpu, b.ew) == 1
    clean = q4_rows(gpu, b.ew, 2, x, 17)
    assert same_bits(clean, core_rows(gpu, b.U[2], x, 17))
    before1 = q4_rows(gpu, b.ew, 1, x, 17)
    b.ew.buckets[:2] = deal_q4(2, 96, 4096, b.gen)
    b.ew.stats[:2] = float("nan")
    torch.cuda.synchronize()
    assert same_bits(q4_rows(gpu, b.ew, 2, x, 17), clean)
    assert not same_bits(q4_rows(gpu, b.ew, 1, x, 17), before1), "the scramble was not where expert 1 is read"


# ---------------------------------------------------------------- 3. outliers
def outlier_table(outDim, inDim):
    """f32 [n, 4] = (value, input, output, 0): outputs with no, one and many outliers, the last output among them, two outliers on
    one input (on two outputs, and twice on the same output)."""
    rng = np.random.default_rng(3)
    rows = []

    def add(o, n, ins=None):
        ins = rng.integers(0, inDim, n) if ins is None else ins
        for i in ins:
            rows.append((float(np.float16(rng.standard_normal() * 0.3)), float(i), float(o), 0.0))
    add(7, 300)
    add(64, 1)
    add(outDim - 1, 5)
    for o in range(100, 164):                                # a whole block's worth of different counts, block boundaries inside
        add(o, o % 4)
    add(200, 2, ins=[1234, 77])
    add(201, 3, ins=[1234, 4095, 1234])
    t = np.array(rows, np.float32)
    return t[rng.permutation(len(t))]                        # (table order, not output order)


def test_outliers_are_added_in_f32_per_output(gpu):
    outDim, inDim = 1056, 4096
    table = outlier_table(outDim, inDim)
    plain = Q4Bundle(outDim, inDim)
    withol = Q4Bundle(outDim, inDim, outliers=torch.from_numpy(table).to(DEV))
    assert torch.equal(plain.ew.buckets, withol.ew.buckets) and torch.equal(plain.ew.stats, withol.ew.stats)
    x = x_rows(inDim)
    base = q4_rows(gpu, plain.ew, 0, x, 64)
    got = q4_rows(gpu, withol.ew, 0, x, 64)
    assert bool(torch.isfinite(got).all())
    count = np.bincount(table[:, 2].astype(np.int64), minlength=outDim)
    none = torch.from_numpy(count == 0).to(DEV)
    assert same_bits(got[:, none], base[:, none])
    x64 = x[:64].double().cpu().numpy()
    S = np.zeros((64, outDim))
    mass = np.zeros((64, outDim))
    for val, i, o, _ in table.astype(np.float64):
        S[:, int(o)] += val * x64[:, int(i)]
        mass[:, int(o)] += np.abs(val * x64[:, int(i)])
    b64 = base.double().cpu().numpy()
    err = np.abs(got.double().cpu().numpy() - (b64 + S))
    bound = 2.0 ** -23 * (count[None, :] + 1) * (np.abs(b64) + mass)
    worst = float((err[:, count > 0] / bound[:, count > 0]).max())
    print(f"outlier term: worst error over its bound {worst:.3f}")
    assert (err[:, count > 0] <= bound[:, count > 0]).all()
    assert bool((got[:, ~none] != base[:, ~none]).any())
    # the term of row r does not depend on the block
    for rows in (1, 5, 17):
        assert same_bits(q4_rows(gpu, withol.ew, 0, x, rows), got[:rows]), rows
    assert same_bits(q4_rows(gpu, withol.ew, 0, x[40:41], 1), got[40:41])


# ---------------------------------------------------------------- 4. the check and the refusals
def test_the_check_is_cached_until_a_refresh(gpu):
    from effort_amd.weights import ExpertWeights
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    core = (torch.randn((4096, 4096), generator=gen, device=DEV) * 0.02).to(torch.float16)      # (the probes are the diagonal: 4096 of them)
    ew = ExpertWeights.from_core_q4(core)                    # converter output, 2 % outliers
    assert ew.outliers is not None and dense_ok(gpu, ew) == 1
    x = x_rows(4096)
    clean = q4_rows(gpu, ew, 0, x, 5)
    assert bool(torch.isfinite(clean).all())
    # one nibble takes the position of the next rank's: a duplicate
    i, c = 8 * 4000 + 3, 2
    kept = int(ew.buckets[0, i, c])
    other = int(ew.buckets[0, i + 1, c])
    ew.buckets[0, i, c] = ((kept & 0xFFFF & ~0x0700) | (other & 0x0700)) - (0x10000 if kept < 0 else 0)
    assert int(ew.buckets[0, i, c]) != kept
    assert dense_ok(gpu, ew) == 1, "the answer is cached until a refresh"
    ew.refresh()
    assert dense_ok(gpu, ew) == 0
    assert q4_rows(gpu, ew, 0, x, 5, expect=ERR_CONVERT) == ERR_CONVERT
    with pytest.raises(ValueError, match="eight different positions"):
        ew.unbucket_q4()
    ew.buckets[0, i, c] = kept
    ew.refresh()
    assert dense_ok(gpu, ew) == 1
    assert same_bits(q4_rows(gpu, ew, 0, x, 5), clean)
    # one mean that is no f16 number
    m = float(ew.stats[0, i, 1])
    ew.stats[0, i, 1] = m * (1.0 + 2.0 ** -14)
    assert dense_ok(gpu, ew) == 1
    ew.refresh()
    assert dense_ok(gpu, ew) == 0
    assert q4_rows(gpu, ew, 0, x, 5, expect=ERR_CONVERT) == ERR_CONVERT
    ew.stats[0, i, 1] = m
    ew.refresh()
    assert dense_ok(gpu, ew) == 1
    assert same_bits(q4_rows(gpu, ew, 0, x, 5), clean)


def test_a_bad_bundle_is_found_by_the_first_multiply(gpu):
    b = Q4Bundle(64, 4096, E=2)
    b.ew.stats[1, 9, 1] = float("inf")                       # expert 1; no check was run yet
    assert q4_rows(gpu, b.ew, 0, x_rows(4096), 3, expect=ERR_CONVERT) == ERR_CONVERT      # the HANDLE is judged, whichever expert is asked for


def test_refusals_enqueue_nothing(gpu):
    from tests.test_gpu_prefill_buckets import Bundle
    b = Q4Bundle(128, 4096, E=2)
    x = x_rows(4096)
    h = b.ew.handle
    for rows in (0, -1, 65):
        q4_rows(gpu, b.ew, 0, x, rows, expect=ERR_ARG)
    for expert in (-1, 2):
        q4_rows(gpu, b.ew, expert, x, 4, expect=ERR_ARG)
    out = fresh_out(4 * 128)
    xs = padded_x(x, 4)
    assert lib().effort_q4_gemm_rows(gpu.ctx, h, 0, None, P(out), 4) == ERR_ARG
    assert lib().effort_q4_gemm_rows(gpu.ctx, h, 0, P(xs), None, 4) == ERR_ARG
    assert lib().effort_q4_gemm_rows(gpu.ctx, None, 0, P(xs), P(out), 4) == ERR_ARG
    assert lib().effort_q4_gemm_rows(None, h, 0, P(xs), P(out), 4) == ERR_ARG
    assert lib().effort_weights_q4_dense_ok(None, C.byref(C.c_int(0))) == ERR_ARG
    assert lib().effort_weights_q4_dense_ok(h, None) == ERR_ARG

    def both(ew, code, inDim=4096, x_ptr=True):
        xx = padded_x(x_rows(inDim), 4)
        o1 = fresh_out(4 * ew.outSize)
        assert lib().effort_q4_gemm_rows(gpu.ctx, ew.handle, 0, P(xx) if x_ptr else None, P(o1), 4) == code
        ok = C.c_int(7)
        assert lib().effort_weights_q4_dense_ok(ew.handle, C.byref(ok)) == code and ok.value == 7
        gpu.eval()
        assert bool(torch.isnan(o1[:-8]).all()) and bool((o1[-8:] == SENTINEL).all())

    fp16 = Bundle(64, 4096)
    both(fp16.ew, ERR_KIND)
    both(fp16.ew, ERR_KIND, x_ptr=False)                     # values before pointers
    both(b.ew.column_shard(0, 2), ERR_SHAPE)                 # a column-shard view
    both(Q4Bundle(32, 4112).ew, ERR_SHAPE, inDim=4112)       # inDim % 32 != 0
    # the FP16 bucket entry points keep refusing Q4 handles
    o1 = fresh_out(4 * 128)
    assert lib().effort_bucket_gemm_rows(gpu.ctx, h, 0, P(xs), P(o1), 4) == ERR_KIND
    ok = C.c_int(7)
    assert lib().effort_weights_bucket_dense_ok(h, C.byref(ok)) == ERR_KIND and ok.value == 7
    gpu.eval()
    assert bool(torch.isnan(o1[:-8]).all()) and bool(torch.isnan(out[:-8]).all()), "a refused call wrote to out"
    assert bool((out[-8:] == SENTINEL).all())


# ---------------------------------------------------------------- 5. Decoder.prefill(weights="q4")
MAXTOK, VOCAB = 16, 512
PROMPT = [3, 500, 17, 256, 9, 41, 77, 130, 2, 311, 5, 64]
Q4_BUNDLES = ("wq", "w1", "w2", "w3")


def config():
    from effort_amd.decode import MistralConfig
    return MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=2, numHeads=32, numHeadsKV=8, headDim=128, vocab=VOCAB)


def caches(dec, T):
    return [c[:T].clone() for c in dec.kCache + dec.vCache]


def prefill_caches(model, T=len(PROMPT), **kw):
    from effort_amd.decode import Decoder
    dec = Decoder(model, maxTokens=MAXTOK)
    for c in dec.kCache + dec.vCache:
        c.fill_(float("nan"))
    dec.prefill(PROMPT[:T], **kw)
    torch.cuda.synchronize()
    assert int(dec.pos[0]) == T
    got = caches(dec, T)
    assert all(bool(torch.isfinite(c).all()) for c in got)
    return got


def only_kv_cores(model):
    for L in model.layers:
        for w in ("wq", "wk", "wv", "wo", "w1", "w2", "w3"):
            ew = getattr(L, w)
            assert (ew.core is None) == (w in Q4_BUNDLES), w
            assert ew.bucketsLoaded == (w in Q4_BUNDLES) and ew.q4


def test_q4_prefill_without_outliers_is_the_cores_prefill_on_the_unbucketed_matrices(hip_lib_built):
    from effort_amd.decode import Decoder, Model
    torch.cuda.set_device(0)
    bare = Model.random(config(), seed=21, q4=True, keep_cores=False, q4_perc=0)
    cored = Model.random(config(), seed=21, q4=True, q4_perc=0)
    only_kv_cores(bare)
    for La, Lb in zip(bare.layers, cored.layers):
        for w in Q4_BUNDLES:
            a, b = getattr(La, w), getattr(Lb, w)
            assert a.outliers is None and torch.equal(a.buckets, b.buckets) and torch.equal(a.stats, b.stats)
            b.core = b.unbucket_q4()[0]
    with pytest.raises(ValueError, match="every bundle needs its f16 core"):
        Decoder(bare, maxTokens=MAXTOK).prefill(PROMPT)      # the default call still refuses a model without those cores
    with pytest.raises(ValueError, match="FP16 with its buckets loaded"):
        Decoder(bare, maxTokens=MAXTOK).prefill(PROMPT, weights="buckets")
    from_q4 = prefill_caches(bare, weights="q4")
    from_cores = prefill_caches(cored, weights="cores")
    assert all(same_bits(a, b) for a, b in zip(from_q4, from_cores))
    for chunk in (1, 5):
        small = prefill_caches(bare, weights="q4", chunk=chunk)
        assert all(same_bits(a, b) for a, b in zip(small, from_q4)), f"chunk {chunk} against chunk 64"


def test_q4_prefill_with_outliers_then_decodes(hip_lib_built):
    from effort_amd.decode import Decoder, Model
    torch.cuda.set_device(0)
    bare = Model.random(config(), seed=22, q4=True, keep_cores=False)
    only_kv_cores(bare)
    assert all(getattr(L, w).outliers.shape[0] == int(4096 * 4096 * 0.02) for L in bare.layers for w in Q4_BUNDLES)
    whole = prefill_caches(bare, weights="q4")
    for chunk in (1, 5):
        small = prefill_caches(bare, weights="q4", chunk=chunk)
        assert all(same_bits(a, b) for a, b in zip(small, whole)), f"chunk {chunk} against chunk 64"
    dec = Decoder(bare, maxTokens=MAXTOK)
    ids, _, _ = dec.run(PROMPT, MAXTOK, effort=0.25, prefill=True, prefill_weights="q4")         # raises on a device status
    P1 = len(PROMPT) - 1
    assert ids[:P1] == [-1] * P1 and all(0 <= t < VOCAB for t in ids[P1:]) and dec.status() == 0
    only_kv_cores(bare)
