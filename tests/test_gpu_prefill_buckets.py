"""Prefill straight from the bucketed weights on the GPU (effort_amd/csrc/prefill_buckets.hip, Decoder.prefill(weights="buckets")).

The contract is BITS: effort_bucket_gemm_rows writes what effort_dense_gemm_rows writes when the un-bucketed matrix
(``effort_amd.weights.unbucket``, pinned to the converter by tests/test_unbucket_cpu.py) is given to it as the core -- and that kernel
is pinned to float64 by tests/test_gpu_prefill.py.  So every check here compares bits, none a tolerance.

The bundles are built directly (as tests/edge_shapes.py builds its own: the converters reach a small part of what registration
accepts): a random f16 matrix, every weight's low four bits replaced by its position in its bucket, the 16 entries of every bucket
dealt to the 16 ranks in a random order.  "NaN buckets" of an expert that must not be read keep their position bits (0x7E00 | pos: a
NaN all the same), so that the handle stays un-bucketable and only a READ of them can show."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.test_gpu_glue import DEV, P, gpu, lib  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
MAX_ROWS = 64
SENTINEL = -555.0
NAN16 = 0x7E00
ERR_ARG, ERR_SHAPE, ERR_KIND, ERR_CONVERT = -1, -2, -5, -6


def same_bits(a, b) -> bool:
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


# ---------------------------------------------------------------- bundles
def deal(W, gen):
    """f16 [E, out, in] on the device -> bucket words int16 [E, 16 * in, out / 16]: (w & 0xFFF0) | position, the ranks in random order."""
    E, o, i = W.shape
    cols = o // 16
    w = W.view(torch.int16).to(torch.int32) & 0xFFF0
    w |= (torch.arange(o, device=W.device, dtype=torch.int32) % 16)[None, :, None]
    w = w.permute(0, 2, 1).reshape(E, i, cols, 16)                                    # [e][j][c][position]
    order = torch.rand((E, i, cols, 16), generator=gen, device=W.device).argsort(3)
    w = torch.gather(w, 3, order)                                                     # [e][j][c][rank]
    w = w.permute(0, 3, 1, 2).reshape(E, 16 * i, cols)
    return ((w ^ 0x8000) - 0x8000).to(torch.int16)


class Bundle:
    """A registered FP16 bundle built directly.  ``words``: the view of its payload [E, 16 * in, cols] (rewrite it in place, then
    ``ew.refresh()``); ``pitch`` in bytes (None: dense), the padding NaN."""

    def __init__(self, outDim, inDim, E=1, pitch=None, seed=0):
        from effort_amd.weights import ExpertWeights
        gen = torch.Generator(device=DEV)
        gen.manual_seed(seed * 1000003 + outDim * 31 + inDim)
        W = (torch.randn((E, outDim, inDim), generator=gen, device=DEV) * 0.02).to(torch.float16)
        cols, rows = outDim // 16, 16 * inDim
        b = deal(W, gen)
        if pitch is None:
            self.store = b.contiguous()
            self.words = self.store
        else:
            assert pitch % 4 == 0 and pitch >= 2 * cols
            self.store = torch.full((E, rows, pitch // 2), NAN16, dtype=torch.int16, device=DEV)
            self.store[:, :, :cols] = b
            self.words = self.store[:, :, :cols]
        mean = self.words.view(torch.float16).abs().float().mean(2).to(torch.float16)
        stats = mean[:, :, None].expand(E, rows, 4).contiguous()
        probes = (torch.randn((E, 4096), generator=gen, device=DEV) * 0.02).to(torch.float16)
        self.ew = ExpertWeights(self.words, stats, probes, inDim, outDim, 16, E)
        assert self.ew.rowPitch == (pitch or 2 * cols)
        self.outDim, self.inDim, self.E = outDim, inDim, E

    @property
    def U(self):
        """unbucket() of the payload as it is NOW: f16 [E, out, in]."""
        from effort_amd.weights import unbucket
        return unbucket(self.words, self.inDim, self.outDim)

    def poison(self, experts):
        """The buckets of ``experts`` become NaN that keep their position bits."""
        for e in experts:
            self.words[e] = (self.words[e] & 15) | NAN16


_X = {}


def x_rows(inDim):
    """64 heavy-tailed input rows per inDim, shared and left unchanged."""
    if inDim not in _X:
        gen = torch.Generator(device=DEV)
        gen.manual_seed(inDim)
        x = torch.randn((2 * MAX_ROWS, inDim), generator=gen, device=DEV)
        _X[inDim] = x * torch.exp(0.8 * torch.randn((2 * MAX_ROWS, inDim), generator=gen, device=DEV))
    return _X[inDim]


def padded_x(x, rows, beyond=float("nan"), alloc=MAX_ROWS):
    full = torch.full((alloc, x.shape[1]), beyond, dtype=torch.float32, device=DEV)
    full[:rows] = x[:rows]
    return full


def fresh_out(n):
    out = torch.full((n + 8,), float("nan"), dtype=torch.float32, device=DEV)
    out[n:] = SENTINEL
    return out


def bucket_rows(gpu, bundle, expert, x, rows, expect=0):
    """The call with NaN x rows past ``rows`` on a NaN out with a sentinel tail.  Returns out [rows][outDim] (or the return code)."""
    n = rows * bundle.outDim if 1 <= rows <= MAX_ROWS else 8
    out = fresh_out(n)
    rc = lib().effort_bucket_gemm_rows(gpu.ctx, bundle.ew.handle, expert, P(padded_x(x, max(0, min(rows, MAX_ROWS)))), P(out), rows)
    gpu.eval()
    assert rc == expect, (rc, expect)
    assert bool((out[n:] == SENTINEL).all()), "wrote past rows * outDim"
    if expect:
        assert bool(torch.isnan(out[:n]).all()), "a refused call wrote to out"
        return rc
    return out[:n].view(rows, bundle.outDim)


def core_rows(gpu, U, x, rows):
    outDim, inDim = U.shape
    out = fresh_out(rows * outDim)
    gpu.check(lib().effort_dense_gemm_rows(gpu.ctx, P(U.contiguous()), P(padded_x(x, rows)), P(out), inDim, outDim, rows), "dense_gemm_rows")
    gpu.eval()
    return out[:rows * outDim].view(rows, outDim)


# ---------------------------------------------------------------- 1. bits
# (outDim, inDim, rows, pitch in bytes or None) and what each reaches.  cols = outDim / 16 bucket columns; a workgroup owns 32 of them; the
# row pieces are 16-byte loads when pitch % 16 == 0 and cols % 8 == 0, else 4-byte loads; the k split is the core kernel's.
BIT_SHAPES = [
    (32, 4096, 1, None),         # 2 columns (a 4-byte row), one workgroup with 30 dead columns; 16 splits of one stage (the cap); one live token
    (96, 4096, 16, None),        # the dense pitch of 12 bytes: no 16-byte load is legal; 6 columns
    (96, 4096, 16, 128),         # the same matrix on whole lines, the padding NaN
    (1056, 4096, 17, None),      # 66 columns: two full tiles and a ragged one of 2; NT 2 with one live column in the second tile; pitch 132
    (64, 4128, 5, None),         # a last stage of 32 live k: chunks of zeros behind it are still stepped through
    (4096, 4096, 64, 512),       # the wq shape, 16-byte loads, NT 4, 4 splits of 4 stages
    (1024, 14336, 64, 128),      # the longest K: 56 stages, 14 splits
    (8224, 4096, 16, None),      # above 64 MiB: the nt stream; 514 columns (4-byte loads), a ragged last tile of 2
    (8192, 4224, 16, 1024),      # above 64 MiB with 16-byte loads; 17 stages, the last one half live
]


@pytest.mark.parametrize("outDim,inDim,rows,pitch", BIT_SHAPES)
def test_bucket_multiply_is_the_core_multiply_on_the_unbucketed_matrix(gpu, outDim, inDim, rows, pitch):
    b = Bundle(outDim, inDim, pitch=pitch)
    x = x_rows(inDim)
    got = bucket_rows(gpu, b, 0, x, rows)
    want = core_rows(gpu, b.U[0], x, rows)
    assert bool(torch.isfinite(got).all()), "NaN from the pitch padding, an x row past `rows` or a dead k reached a result"
    assert same_bits(got, want)


# ---------------------------------------------------------------- 2. masking and independence
def test_a_row_does_not_depend_on_the_block(gpu):
    b = Bundle(1056, 4096, pitch=2176)                       # whole lines and one spare, the padding NaN
    x = x_rows(4096)
    full = bucket_rows(gpu, b, 0, x, 64)
    want = core_rows(gpu, b.U[0], x, 64)
    assert same_bits(full, want)
    for rows in (1, 5, 16, 17, 64):
        assert same_bits(bucket_rows(gpu, b, 0, x, rows), full[:rows]), rows
    alone = bucket_rows(gpu, b, 0, x[40:41], 1)              # row 40 as a block of its own
    assert same_bits(alone, full[40:41])


def test_other_experts_are_not_read(gpu):
    b = Bundle(64, 4096, E=3, pitch=128)
    x = x_rows(4096)
    clean = bucket_rows(gpu, b, 2, x, 17)
    assert same_bits(clean, core_rows(gpu, b.U[2], x, 17))
    b.poison((0, 1))
    b.ew.refresh()                                           # the check runs again: NaN with their positions stay un-bucketable
    assert same_bits(bucket_rows(gpu, b, 2, x, 17), clean)
    assert bool(torch.isnan(bucket_rows(gpu, b, 1, x, 17)).any()), "the poison was not where expert 1 is read"


# ---------------------------------------------------------------- 3. collisions
def dense_ok(gpu, ew):
    ok = C.c_int(-1)
    gpu.check(lib().effort_weights_bucket_dense_ok(ew.handle, C.byref(ok)), "weights_bucket_dense_ok")
    return ok.value


def rank_row_of(b, j, c, pos, e=0):
    """The bucket row of expert e whose entry at column c is input j's weight for position pos."""
    col = b.words[e, j::b.inDim, c].to(torch.int32) & 15      # the 16 ranks' entries of (j, c)
    return int((col == pos).nonzero()[0]) * b.inDim + j


def test_collisions_are_refused_and_zero_entries_are_skipped(gpu):
    b = Bundle(96, 4096)
    x = x_rows(4096)
    assert dense_ok(gpu, b.ew) == 1
    clean = bucket_rows(gpu, b, 0, x, 5)
    # a 0x0000 entry in place of a real one: U has +0 there, nothing is refused
    j, c = 4000, 5
    r0 = rank_row_of(b, j, c, 9)
    kept = int(b.words[0, r0, c])
    b.words[0, r0, c] = 0
    b.ew.refresh()
    assert dense_ok(gpu, b.ew) == 1
    U = b.U
    assert int(U.view(torch.int16)[0, 16 * c + 9, j]) == 0
    holed = bucket_rows(gpu, b, 0, x, 5)
    assert same_bits(holed, core_rows(gpu, U[0], x, 5)) and not same_bits(holed, clean)
    # a duplicate position: the entry for position 3 now names position 9's neighbour 4 -- which has an entry already
    b.words[0, r0, c] = kept
    r3 = rank_row_of(b, j, c, 3)
    was = int(b.words[0, r3, c])
    b.words[0, r3, c] = (was & ~15) | 4
    assert dense_ok(gpu, b.ew) == 1, "the answer is cached until a refresh"
    b.ew.refresh()
    assert dense_ok(gpu, b.ew) == 0
    assert bucket_rows(gpu, b, 0, x, 5, expect=ERR_CONVERT) == ERR_CONVERT
    with pytest.raises(ValueError, match="same output position"):
        b.U
    b.words[0, r3, c] = was
    b.ew.refresh()
    assert dense_ok(gpu, b.ew) == 1
    assert same_bits(bucket_rows(gpu, b, 0, x, 5), clean)


def test_a_collision_is_found_by_the_first_multiply(gpu):
    b = Bundle(64, 4096, E=2)
    r = rank_row_of(b, 7, 0, 0, e=1)
    b.words[1, r, 0] = b.words[1, r, 0] | 1                   # expert 1: two entries of (7, 0) name position 1; no refresh, no check was run yet
    assert bucket_rows(gpu, b, 0, x_rows(4096), 3, expect=ERR_CONVERT) == ERR_CONVERT      # the HANDLE is judged, whichever expert is asked for


# ---------------------------------------------------------------- 4. refusals
def test_refusals_enqueue_nothing(gpu):
    from effort_amd.weights import ExpertWeights
    b = Bundle(64, 4096, E=2)
    x = x_rows(4096)
    h = b.ew.handle
    for rows in (0, -1, 65):
        bucket_rows(gpu, b, 0, x, rows, expect=ERR_ARG)
    for expert in (-1, 2):
        bucket_rows(gpu, b, expert, x, 4, expect=ERR_ARG)
    out = fresh_out(4 * 64)
    xs = padded_x(x, 4)
    assert lib().effort_bucket_gemm_rows(gpu.ctx, h, 0, None, P(out), 4) == ERR_ARG
    assert lib().effort_bucket_gemm_rows(gpu.ctx, h, 0, P(xs), None, 4) == ERR_ARG
    assert lib().effort_bucket_gemm_rows(gpu.ctx, None, 0, P(xs), P(out), 4) == ERR_ARG
    assert lib().effort_bucket_gemm_rows(None, h, 0, P(xs), P(out), 4) == ERR_ARG
    idx = torch.zeros(2 * MAX_ROWS, dtype=torch.int32, device=DEV)
    out2 = fresh_out(4 * 2 * 64)
    routed = lambda hh, i, xx, per, oo, rows: lib().effort_bucket_gemm_rows_routed(gpu.ctx, hh, i, xx, per, oo, rows)   # noqa: E731
    assert routed(h, P(idx), P(xs), 2, P(out2), 4) == ERR_ARG
    assert routed(h, P(idx), P(xs), 0, P(out2), 0) == ERR_ARG
    assert routed(h, P(idx), P(xs), 0, P(out2), 65) == ERR_ARG
    assert routed(h, None, P(xs), 0, P(out2), 4) == ERR_ARG
    assert routed(h, P(idx), None, 0, P(out2), 4) == ERR_ARG
    assert routed(h, P(idx), P(xs), 0, None, 4) == ERR_ARG
    assert routed(None, P(idx), P(xs), 0, P(out2), 4) == ERR_ARG

    def both(ew, code, inDim=4096):
        xx = padded_x(x_rows(inDim), 4)
        o1, o2 = fresh_out(4 * ew.outSize), fresh_out(8 * ew.outSize)
        assert lib().effort_bucket_gemm_rows(gpu.ctx, ew.handle, 0, P(xx), P(o1), 4) == code
        assert lib().effort_bucket_gemm_rows_routed(gpu.ctx, ew.handle, P(idx), P(xx), 0, P(o2), 4) == code
        ok = C.c_int(7)
        assert lib().effort_weights_bucket_dense_ok(ew.handle, C.byref(ok)) == code and ok.value == 7
        gpu.eval()
        assert bool(torch.isnan(o1[:-8]).all()) and bool(torch.isnan(o2[:-8]).all())

    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    core = (torch.randn((4096, 4096), generator=gen, device=DEV) * 0.02).to(torch.float16)
    both(ExpertWeights.from_core_q4(core), ERR_KIND)
    both(b.ew.truncated(8), ERR_SHAPE)                       # percentLoad != 16
    both(b.ew.column_shard(0, 2), ERR_SHAPE)                 # a column-shard view
    both(Bundle(32, 4112).ew, ERR_SHAPE, inDim=4112)         # inDim % 32 != 0
    many = Bundle(32, 4096, E=65)
    xx = padded_x(x, 4)
    o2 = fresh_out(8 * 32)
    assert lib().effort_bucket_gemm_rows_routed(gpu.ctx, many.ew.handle, P(idx), P(xx), 0, P(o2), 4) == ERR_SHAPE
    gpu.eval()
    assert bool(torch.isnan(o2[:-8]).all())
    assert same_bits(bucket_rows(gpu, many, 64, x, 2), core_rows(gpu, many.U[64], x, 2))      # (the plain call serves any expert count)
    gpu.eval()
    assert bool(torch.isnan(out[:-8]).all()) and bool(torch.isnan(out2[:-8]).all()), "a refused call wrote to out"
    assert bool((out[-8:] == SENTINEL).all()) and bool((out2[-8:] == SENTINEL).all())


# ---------------------------------------------------------------- 5. the routed front end
_STACKS = {}


def stack_of(outDim, inDim, pitch, E):
    """(clean bundle, per-(expert, input row id) cache of the plain call's row), one per (shape, pitch, expert count); never rewritten."""
    key = (outDim, inDim, pitch, E)
    if key not in _STACKS:
        _STACKS[key] = (Bundle(outDim, inDim, E=E, pitch=pitch, seed=9), {})
    return _STACKS[key]


def routing(kind, rows, seed, E):
    rng = np.random.default_rng(seed)
    if kind == "random":                                     # two distinct experts per token
        idx = np.stack([rng.permutation(E)[:2] for _ in range(rows)])
    elif kind == "one":                                      # every assignment on expert 2: up to 128 columns, walked 64 at a time
        idx = np.full((rows, 2), 2)
    else:                                                    # "clamped": out-of-range expert numbers mean the last expert
        idx = np.stack([rng.permutation(E)[:2] for _ in range(rows)])
        idx[::2, 1] = 7
        idx[-1, 0] = 0xFFFFFFFF
    return idx.astype(np.uint32)


# (outDim, inDim, pitch in bytes or None, experts, rows, kind, xPerSlot) and the instantiation <AUX 0 | 2 (nt), VEC 4 | 1 (dwords per
# load)> of the routed kernel each reaches.  nt is judged by ONE expert's matrix (above 64 MiB), so the two large stacks cannot be smaller;
# two experts is the fewest that still routes.
def _routed(outDim, inDim, pitch, E, rows, kind, xPerSlot):
    return pytest.param(outDim, inDim, pitch, E, rows, kind, xPerSlot, id=f"{outDim}-{rows}-{kind}-{xPerSlot}")


ROUTED_CASES = [
    # 4 and 66 columns on whole lines (pitch 128, 256): no multiple of 8 columns, 4-byte pieces: <0, 1>
    *[_routed(outDim, 4096, (outDim // 16 * 2 + 127) // 128 * 128, 4, rows, kind, xPerSlot)
      for xPerSlot in (0, 1) for kind in ("random", "one", "clamped") for rows in (1, 17, 64) for outDim in (64, 1056)],
    # 8 columns, 16-byte pieces: <0, 4>
    *[_routed(128, 4096, 128, 4, 17, kind, xPerSlot) for xPerSlot in (0, 1) for kind in ("random", "one")],
    _routed(8192, 4224, 1024, 2, 16, "random", 0),           # one expert above 64 MiB, 16-byte pieces: <2, 4>
    _routed(8224, 4096, None, 2, 16, "random", 0),           # above 64 MiB, 514 columns on the dense pitch of 1028: 4-byte pieces: <2, 1>
]


@pytest.mark.parametrize("outDim,inDim,pitch,E,rows,kind,xPerSlot", ROUTED_CASES)
def test_routed_is_the_plain_call_per_assignment(gpu, outDim, inDim, pitch, E, rows, kind, xPerSlot):
    clean, cache = stack_of(outDim, inDim, pitch, E)
    idx = routing(kind, rows, seed=outDim + rows, E=E)
    picked = np.minimum(idx.reshape(-1), E - 1)
    b = clean
    unpicked = sorted(set(range(E)) - set(picked.tolist()))
    if unpicked:                                             # a never-picked expert's buckets are NaN: a copy of the stack, poisoned
        b = Bundle(outDim, inDim, E=E, pitch=pitch, seed=9)
        assert torch.equal(b.words, clean.words)
        b.poison(unpicked)
        b.ew.refresh()
    xsrc = x_rows(inDim)
    xRows = (2 if xPerSlot else 1) * rows
    x = padded_x(xsrc, xRows, alloc=2 * MAX_ROWS)
    idx_d = torch.full((2 * MAX_ROWS,), 3, dtype=torch.int32, device=DEV)
    idx_d[:2 * rows] = torch.from_numpy(idx.reshape(-1).view(np.int32).copy()).to(DEV)
    n = 2 * rows * outDim
    out = fresh_out(n)
    gpu.check(lib().effort_bucket_gemm_rows_routed(gpu.ctx, b.ew.handle, P(idx_d), P(x), xPerSlot, P(out), rows), "bucket_gemm_rows_routed")
    gpu.eval()
    assert bool((out[n:] == SENTINEL).all())
    got = out[:n].view(2 * rows, outDim)
    assert bool(torch.isfinite(got).all())
    for a in range(2 * rows):
        e, xr = int(picked[a]), (a if xPerSlot else a // 2)
        if (e, xr) not in cache:
            cache[(e, xr)] = bucket_rows(gpu, clean, e, xsrc[xr:xr + 1], 1).clone()
        assert same_bits(got[a:a + 1], cache[(e, xr)]), (a, e)


# ---------------------------------------------------------------- 6. Decoder.prefill(weights="buckets")
MAXTOK, VOCAB = 16, 512
PROMPT = [3, 500, 17, 256, 9, 41, 77, 130, 2, 311, 5, 64]


def model_pair(experts):
    """(a model WITHOUT cores, the same seed's model whose cores are unbucket() of its buckets)."""
    from effort_amd.decode import MistralConfig, Model
    cfg = MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=2, numHeads=32, numHeadsKV=8, headDim=128, vocab=VOCAB, numExperts=experts)
    bare = Model.random(cfg, seed=21, keep_cores=False)
    cored = Model.random(cfg, seed=21, keep_cores=True)
    for La, Lb in zip(bare.layers, cored.layers):
        for w in ("wq", "wk", "wv", "wo", "w1", "w2", "w3"):
            a, b = getattr(La, w), getattr(Lb, w)
            assert a.core is None and torch.equal(a.buckets, b.buckets)
            U = b.unbucket()
            b.core = U if b.numExperts > 1 else U[0]
    return bare, cored


@pytest.fixture(scope="module")
def mistral(hip_lib_built):
    torch.cuda.set_device(0)
    return model_pair(1)


@pytest.fixture(scope="module")
def mixtral(hip_lib_built):
    torch.cuda.set_device(0)
    return model_pair(4)


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


def check_decoder(pair, ffn):
    bare, cored = pair
    from effort_amd.decode import Decoder
    with pytest.raises(ValueError, match="every bundle needs its f16 core"):
        Decoder(bare, maxTokens=MAXTOK).prefill(PROMPT, ffn=ffn)                     # the default call still refuses a core-less model
    for attention in ("rows", "block"):
        from_buckets = prefill_caches(bare, ffn=ffn, attention=attention, weights="buckets")
        from_cores = prefill_caches(cored, ffn=ffn, attention=attention, weights="cores")
        assert all(same_bits(a, b) for a, b in zip(from_buckets, from_cores)), attention
        small = prefill_caches(bare, ffn=ffn, attention=attention, weights="buckets", chunk=3)
        assert all(same_bits(a, b) for a, b in zip(small, from_buckets)), f"{attention}: chunk 3 against chunk 64"
    dec = Decoder(bare, maxTokens=MAXTOK)
    ids, _, _ = dec.run(PROMPT, MAXTOK, effort=0.25, prefill=True, prefill_ffn=ffn, prefill_weights="buckets")      # raises on a device status
    P1 = len(PROMPT) - 1
    assert ids[:P1] == [-1] * P1 and all(0 <= t < VOCAB for t in ids[P1:]) and dec.status() == 0


def test_mistral_prefills_without_cores(mistral):
    check_decoder(mistral, "dense")


def test_mixtral_prefills_without_cores(mixtral):
    check_decoder(mixtral, "routed")


def test_bucket_prefill_refusals(mistral):
    from effort_amd.decode import Decoder
    bare, cored = mistral
    dec = Decoder(bare, maxTokens=MAXTOK)
    dec.pos.fill_(2)
    with pytest.raises(ValueError, match="weights must be"):
        dec.prefill(PROMPT, weights="bucket")
    with pytest.raises(ValueError, match="Mixtral"):
        dec.prefill(PROMPT, weights="buckets", ffn="routed")
    L = bare.layers[1]
    whole, L.wo = L.wo, L.wo.truncated(8)
    try:
        with pytest.raises(ValueError, match="percentLoad 16"):
            dec.prefill(PROMPT, weights="buckets")
    finally:
        L.wo = whole
    assert int(dec.pos[0]) == 2 and dec._pf is None
