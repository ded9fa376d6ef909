"""The sampled pick on the GPU (effort_amd/csrc/sample.hip through effort_topk / effort_sample, and the Decoder around it) against the
numpy specification of effort_amd/sampling.py.

Bars: the top-K selection is exact (indices and value bits); top_k = 1 and a greedy temperature are effort_argmax bit for bit (id, history,
position, status word); a drawn id equals ``sample_reference``'s whenever the reference's margin -- the distance from u * S to the nearest
cumulative boundary, over S -- is at least 1e-4 (the kernel's f32 running sums of <= 64 terms with expf at a few ulp are within 1e-5
relative of the float64 ones; 1e-4 leaves a factor of ten), and at most 5 % of a configuration's draws may fall below that margin."""
import ctypes as C

import numpy as np
import pytest
import torch

from effort_amd.sampling import Sampling, sample_reference, sample_reference_many, topk_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN, MAX_EXCLUDED = 1e-4, 0.05

NS = (1, 5, 63, 64, 65, 1000, 1024, 1025, 4099, 32000, 40000)
KS = (1, 2, 16, 63, 64)
FAMILIES = ("gauss", "equal", "quant8", "zeros", "nan_inf", "all_nan", "tail", "tail_ties")


def make(family: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + n % 997)
    g = rng.standard_normal(n).astype(np.float32)
    if family == "gauss":
        return g
    if family == "equal":                                   # every logit equal: the result is 0 .. K-1
        return np.full(n, 1.25, dtype=np.float32)
    if family == "quant8":                                  # 8 levels: the threshold cuts through a tie class of about n / 8
        return np.clip(np.floor(g * 2), -4, 3).astype(np.float32)
    if family == "zeros":                                   # the two zeros tie; a quarter lies below, a few above
        x = np.where(rng.random(n) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        r = rng.random(n)
        x[r < 0.25] = -1.0
        x[r > 0.97] = 1.0
        return x
    if family == "nan_inf":
        r = rng.random(n)
        g[r < 0.1] = np.nan
        g[r > 0.9] = -np.inf
        return g
    if family == "all_nan":
        return np.full(n, np.nan, dtype=np.float32)
    m = min(n, 80)                                          # the largest values at the last indices (a ragged last vector / last wave range)
    if family == "tail":
        g[n - m:] = 100.0 + 0.5 * np.arange(m, dtype=np.float32)          # n-1 the largest, then n-2, ...
    else:
        g[n - m:] = 50.0                                    # ... and all equal there: the lowest of those indices first
    return g


@pytest.fixture(scope="module")
def gpu(hip_lib_built):
    import effort_amd
    torch.cuda.set_device(0)
    g = effort_amd.gpu()
    g._bind_stream()
    return g


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


@pytest.fixture(scope="module")
def rows():
    """Device copies of every (family, n) input, made once and never modified."""
    return {(f, n): torch.from_numpy(make(f, n)).to(DEV) for f in FAMILIES for n in NS}


# ---------------------------------------------------------------- top-K selection
@pytest.mark.parametrize("family", FAMILIES)
def test_topk_is_exact(gpu, rows, family):
    from effort_amd import _lib
    lib = _lib.lib()
    gpu._bind_stream()
    outs = []
    for n in NS:
        for k in KS:
            idx = torch.full((k,), 12345, dtype=torch.int32, device=DEV)
            val = torch.full((k,), 777.0, dtype=torch.float32, device=DEV)
            gpu.check(lib.effort_topk(gpu.ctx, p(rows[family, n]), n, k, p(idx), p(val)), "topk")
            outs.append((n, k, idx, val))
    gpu.eval()
    assert gpu_status(gpu) == 0                              # no status side effects, all-NaN input included
    for n, k, idx, val in outs:
        want_i, want_v = topk_reference(make(family, n), k)
        got_i = idx.cpu().numpy().view(np.uint32).astype(np.int64)
        got_v = val.cpu().numpy()
        c = want_i.size                                     # min(k, non-NaN logits)
        assert got_i[:c].tolist() == want_i.tolist(), (family, n, k)
        assert got_v[:c].view(np.uint32).tolist() == want_v.view(np.uint32).tolist(), (family, n, k)
        assert (got_i[c:] == 0xFFFFFFFF).all() and np.isneginf(got_v[c:]).all(), (family, n, k)


def test_topk_refuses_bad_arguments(gpu, rows):
    from effort_amd import _lib
    lib = _lib.lib()
    x = rows["gauss", 64]
    idx, val = torch.zeros(64, dtype=torch.int32, device=DEV), torch.zeros(64, device=DEV)
    for n, k in ((64, 0), (64, 65), (0, 4), (-1, 4)):
        assert lib.effort_topk(gpu.ctx, p(x), n, k, p(idx), p(val)) == -1
    assert lib.effort_topk(gpu.ctx, p(x), 64, 4, None, p(val)) == -1 and lib.effort_topk(gpu.ctx, None, 64, 4, p(idx), p(val)) == -1
    par = Sampling().to_device(device=DEV)
    pos = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert lib.effort_sample(gpu.ctx, p(x), 64, None, p(idx), p(pos), None, 0, None, None) == -1
    assert lib.effort_sample(gpu.ctx, p(x), 0, p(par), p(idx), p(pos), None, 0, None, None) == -1
    assert lib.effort_sample(gpu.ctx, p(x), 64, p(par), p(idx), p(pos), p(idx), 0, None, None) == -1
    gpu.eval()
    assert int(pos.item()) == 0                              # nothing was enqueued


# ---------------------------------------------------------------- equivalence with argmax
def gpu_status(g) -> int:
    from effort_amd import _lib
    st = C.c_int(0)
    g.check(_lib.lib().effort_decode_status(g.ctx, C.byref(st)), "decode_status")
    return int(st.value)


def pick(g, x, n, sampling, pos0: int, historyLen: int):
    """One closing call on logits x: effort_argmax (sampling None) or effort_sample.  Returns (id, history, pos, status word)."""
    from effort_amd import _lib
    lib = _lib.lib()
    tok = torch.full((1,), 999999, dtype=torch.int32, device=DEV)
    pos = torch.full((1,), pos0, dtype=torch.int32, device=DEV)
    hist = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    if sampling is None:
        g.check(lib.effort_argmax(g.ctx, p(x), n, p(tok), p(pos), p(hist), historyLen), "argmax")
    else:
        par = sampling.to_device(device=DEV)
        g.check(lib.effort_sample(g.ctx, p(x), n, p(par), p(tok), p(pos), p(hist), historyLen, None, None), "sample")
    g.eval()
    return int(tok.item()), hist.cpu().tolist(), int(pos.item()), gpu_status(g)


@pytest.mark.parametrize("family", FAMILIES)
def test_greedy_settings_equal_argmax(gpu, rows, family):
    gpu._bind_stream()
    assert gpu_status(gpu) >= 0                              # (clears whatever an earlier test left)
    for n in NS:
        x = rows[family, n]
        for pos0, hl in ((3, 8), (4, 4)):                   # inside the history; past it (status bit 0, nothing written)
            if hl == 4 and n not in (5, 1025, 32000):
                continue
            want = pick(gpu, x, n, None, pos0, hl)
            assert want[0] == next(iter(topk_reference(make(family, n), 1)[0].tolist()), 0), (family, n)    # the host answer; every logit NaN: token 0
            assert want[2] == pos0 + 1 and want[3] == (2 if np.isnan(make(family, n)).all() else 0) | (1 if pos0 >= hl else 0)
            for s in (Sampling(top_k=1, temperature=0.8, seed=n), Sampling(top_k=40, temperature=0.0, seed=n),
                      Sampling(top_k=40, temperature=float("nan")), Sampling(top_k=64, temperature=float("inf"), top_p=0.5)):
                assert pick(gpu, x, n, s, pos0, hl) == want, (family, n, s)


def test_device_settings_are_sanitised(gpu, rows):
    """The struct is device memory no host validated: top_k 0 and 1000 clamp to 1 and min(64, n), top_p outside (0, 1] is 1."""
    import struct
    from effort_amd import _lib
    lib = _lib.lib()
    n = 1000
    x = rows["gauss", n]
    xs = make("gauss", n)

    def run(raw, npos=64):
        par = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
        tok, pos = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        hist = torch.zeros(npos, dtype=torch.int32, device=DEV)
        ti, tv = torch.full((64,), -5, dtype=torch.int32, device=DEV), torch.zeros(64, device=DEV)
        for _ in range(npos):
            gpu.check(lib.effort_sample(gpu.ctx, p(x), n, p(par), p(tok), p(pos), p(hist), npos, p(ti), p(tv)), "sample")
        gpu.eval()
        return hist.cpu().tolist(), ti.cpu().tolist()
    h, ti = run(struct.pack("<ffIIIIII", 1.0, 1.0, 0, 5, 0, 0, 0, 0))
    assert h == [int(np.argmax(xs))] * 64 and ti[1:] == [-5] * 63                      # top_k 0 -> 1
    h, ti = run(struct.pack("<ffIIIIII", 2.0, -3.0, 1000, 5, 0, 0, 0, 0))
    ref = Sampling(temperature=2.0, top_k=64, top_p=1.0, seed=5)
    ids, m = sample_reference_many(xs, ref, np.arange(64))
    assert ti == topk_reference(xs, 64)[0].tolist()
    assert all(a == b for a, b, mm in zip(h, ids.tolist(), m) if mm >= MARGIN) and (m < MARGIN).mean() <= MAX_EXCLUDED


# ---------------------------------------------------------------- sampling against the reference
# Three rows of 32000 logits (standard deviation 1, 4, 0.2; numpy default_rng seeds 101, 102, 103), 12 configurations each, 512 draws at
# pos 0 .. 511, seed = 7 * row seed + top_k.  Draws whose REFERENCE margin is below 1e-4, computed on the CPU before any GPU was involved,
# per configuration in the order of CONFIGS (cap: 25 of 512):
#   std 1:   0 2 4 6 6 5 1 1 2 3 5 2
#   std 4:   0 1 5 3 9 2 1 1 4 6 7 9
#   std 0.2: 2 2 3 5 3 9 0 0 3 1 8 9
ROWS = {"std1": (1.0, 101), "std4": (4.0, 102), "flat": (0.2, 103)}
CONFIGS = [(t, k, tp) for t in (0.7, 1.5) for k in (8, 40, 64) for tp in (1.0, 0.9)]
DRAWS = 512


def row(name):
    std, seed = ROWS[name]
    return (np.random.default_rng(seed).standard_normal(32000) * std).astype(np.float32)


def draws(g, x_dev, n, sampling, count):
    """``count`` launches of effort_sample on one row, the position counting by itself from 0: (picks, top-K ids, top-K values)."""
    from effort_amd import _lib
    lib = _lib.lib()
    par = sampling.to_device(device=DEV)
    tok, pos = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    hist = torch.full((count,), -1, dtype=torch.int32, device=DEV)
    ti, tv = torch.full((64,), -5, dtype=torch.int32, device=DEV), torch.zeros(64, device=DEV)
    for _ in range(count):
        g.check(lib.effort_sample(g.ctx, p(x_dev), n, p(par), p(tok), p(pos), p(hist), count, p(ti), p(tv)), "sample")
    g.eval()
    assert int(pos.item()) == count and int(tok.item()) == int(hist[-1].item())
    return hist.cpu().numpy().astype(np.int64), ti.cpu().numpy(), tv.cpu().numpy()


@pytest.mark.parametrize("name", list(ROWS))
def test_draws_match_the_reference(gpu, name):
    gpu._bind_stream()
    x = row(name)
    xd = torch.from_numpy(x).to(DEV)
    for t, k, tp in CONFIGS:
        s = Sampling(temperature=t, top_k=k, top_p=tp, seed=7 * ROWS[name][1] + k)
        want, margin = sample_reference_many(x, s, np.arange(DRAWS))
        keep = margin >= MARGIN
        excluded = int((~keep).sum())
        got, ti, tv = draws(gpu, xd, x.size, s, DRAWS)
        wi, wv = topk_reference(x, k)
        assert ti[:k].tolist() == wi.tolist() and tv[:k].view(np.uint32).tolist() == wv.view(np.uint32).tolist(), (name, t, k, tp)
        bad = np.flatnonzero(keep & (got != want))
        print(f"{name} T={t} k={k} p={tp}: excluded {excluded} / {DRAWS}, mismatches among the kept {bad.size}, distinct ids {len(set(got.tolist()))}")
        assert excluded <= MAX_EXCLUDED * DRAWS, (name, t, k, tp, excluded)
        assert bad.size == 0, (name, t, k, tp, bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
    assert gpu_status(gpu) == 0


def test_seed_and_stream(gpu):
    """The flat row, 256 draws: two seeds differ, a seed repeats itself, stream 1 is another sequence than stream 0."""
    gpu._bind_stream()
    xd = torch.from_numpy(row("flat")).to(DEV)
    run = lambda **kw: draws(gpu, xd, 32000, Sampling(temperature=1.0, top_k=64, **kw), 256)[0].tolist()        # noqa: E731
    a, b, a2, c = run(seed=1), run(seed=2), run(seed=1), run(seed=1, stream=1)
    assert a == a2 and a != b and a != c and b != c
    assert len(set(a)) > 32                                  # 256 draws over 64 near-equal weights


# ---------------------------------------------------------------- the decoder
@pytest.fixture(scope="module")
def small_model(hip_lib_built):
    import effort_amd  # noqa: F401
    from effort_amd.decode import MistralConfig, Model
    cfg = MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=2, numHeads=32, numHeadsKV=8, headDim=128, vocab=512)
    return Model.random(cfg, seed=5)


def check_run_against_reference(ids, logits, s):
    lg = logits.cpu().numpy()
    kept = 0
    for step in range(lg.shape[0]):
        want, margin = sample_reference(lg[step], s, pos=step)
        if margin >= MARGIN:
            kept += 1
            assert ids[step] == want, (step, ids[step], want, margin)
    assert lg.shape[0] - kept <= int(MAX_EXCLUDED * lg.shape[0]), kept
    return kept


def test_decoder_top_k_one_is_the_greedy_run(small_model):
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=32)
    prompt, steps = [3, 77, 130], 12
    ids_g, _, lg_g = dec.run(prompt, steps, effort=0.5, collect_logits=True)
    n_graphs = len(dec._graphs)
    ids_s, _, lg_s = dec.run(prompt, steps, effort=0.5, collect_logits=True, sampling=Sampling(top_k=1, seed=4))
    assert ids_s == ids_g and torch.equal(lg_s, lg_g)
    assert len(dec._graphs) == n_graphs + 1                  # the sampled step is its own graph, once
    ids_d, _, lg_d = dec.run(prompt, steps, dense=True, collect_logits=True)
    ids_ds, _, lg_ds = dec.run(prompt, steps, dense=True, collect_logits=True, sampling=Sampling(temperature=0.0))
    assert ids_ds == ids_d and torch.equal(lg_ds, lg_d)


def test_decoder_sampled_run_follows_the_reference(small_model):
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=32)
    prompt, steps = [3, 77, 130], 24
    s = Sampling(temperature=1.0, top_k=40, top_p=0.95, seed=2024)
    ids, _, lg = dec.run(prompt, steps, effort=0.5, collect_logits=True, sampling=s)
    check_run_against_reference(ids, lg, s)
    ids2, _, lg2 = dec.run(prompt, steps, effort=0.5, collect_logits=True, sampling=s)
    assert ids2 == ids and torch.equal(lg2, lg)              # a run is reproducible from its seed
    # other settings rewrite the 32-byte tensor; the graph is reused, the tokens are what the reference says for the NEW settings
    n_graphs = len(dec._graphs)
    s3 = Sampling(temperature=1.7, top_k=40, top_p=0.95, seed=99)
    ids3, _, lg3 = dec.run(prompt, steps, effort=0.5, collect_logits=True, sampling=s3)
    assert len(dec._graphs) == n_graphs
    check_run_against_reference(ids3, lg3, s3)
    assert ids3 != ids
    greedy, _, _ = dec.run(prompt, steps, effort=0.5)
    assert greedy != ids and dec.status() == 0


def test_decoder_topk_and_pick_among(small_model):
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=32)
    dec.run([3, 77, 130], 6, effort=0.5)
    x = dec.logits.cpu().numpy()
    ids, vals = dec.topk(16)
    wi, wv = topk_reference(x, 16)
    assert ids == wi.tolist() and vals.numpy().view(np.uint32).tolist() == wv.view(np.uint32).tolist()
    assert dec.topk()[0] == ids and dec.topk(1)[0] == [int(np.argmax(x))]
    order = np.argsort(-x.astype(np.float64), kind="stable")
    outside = [int(i) for i in order[16:20]]                 # ranks 17 .. 20: never a hit
    assert dec.pick_among(outside) == 99
    assert dec.pick_among([outside[0], int(order[5]), int(order[2])]) == 3            # rank 3 comes before rank 6: position 3 in the list
    assert dec.pick_among([int(order[15]), outside[1]]) == 1
    assert dec.pick_among([]) == 99
