"""effort_attention_split (effort_amd/csrc/attention_split.hip): decode attention with the keys split across workgroups, one cache copy
read per KV group.  Every case against the float64 reference ``glue_reference.attention`` at the project's f32 bar (``within_bar`` of
tests/test_gpu_glue.py: |got - want| <= 2e-5 * max|want| and cos-sim >= 0.999999).  The caches hold NaN in every row past the position
and in every copy but the first of a KV group: a NaN in the output is a row or a copy the kernel had no business reading."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import glue_reference as ref
from tests.test_gpu_decode import small_model  # noqa: F401  (the fixture)
from tests.test_gpu_glue import BAR_REL, ROPE_BASE, P, bar_figures, dev, gpu, lib, nans, within_bar  # noqa: F401  (gpu: the fixture)

pytestmark = pytest.mark.gpu
POSITIONS = (0, 1, 15, 16, 63, 64, 65, 127, 128, 255, 257, 1030)
SPLITS = (1, 2, 3, 8, 0)
MAXTOK = 1100


def group_caches(Kg, Vg, pos, nh, maxTokens):
    """Device caches [maxTokens][nh][hd] from per-group rows [T][nkv][hd]: rows 0 .. pos of the FIRST copy of each group, NaN elsewhere."""
    nkv = Kg.shape[1]
    kc, vc = nans(maxTokens, nh, Kg.shape[2]), nans(maxTokens, nh, Kg.shape[2])
    kc[:pos + 1, ::nh // nkv] = dev(Kg[:pos + 1])
    vc[:pos + 1, ::nh // nkv] = dev(Vg[:pos + 1])
    return kc, vc


def call(gpu, q, kc, vc, pos, nh, nkv, hd, maxTokens, splits):
    S = splits or lib().effort_attention_split_default_splits(gpu.ctx, nkv, maxTokens)
    scratch = nans(lib().effort_attention_split_scratch_bytes(nh, hd, S) // 4 + 8)
    out, posd = nans(nh * hd + 8), torch.tensor([pos], dtype=torch.int32, device=q.device)
    gpu.check(lib().effort_attention_split(gpu.ctx, P(q), P(kc), P(vc), P(posd), P(out), P(scratch), nh, nkv, hd, maxTokens, splits), "attention_split")
    gpu.eval()
    assert bool(torch.isnan(out[nh * hd:]).all()) and bool(torch.isnan(scratch[-8:]).all()), "wrote past out or the scratch"
    return out[:nh * hd]


def want_of(q, Kg, Vg, pos, nh):
    rep = nh // Kg.shape[1]
    return ref.attention(q.reshape(nh, -1), np.repeat(Kg[:pos + 1], rep, axis=1), np.repeat(Vg[:pos + 1], rep, axis=1))


def check(got, want, tag):
    got = got.cpu().numpy()
    assert np.isfinite(got).all(), (tag, "a NaN reached the output: a row past pos, another copy, or an empty split multiplied in")
    assert within_bar(got, want), (tag, bar_figures(got, want))
    return bar_figures(got, want)[0]


@pytest.mark.parametrize("nh,nkv", [(8, 2), (4, 4), (8, 1), (4, 2)])
@pytest.mark.parametrize("hd", (64, 128, 256))
def test_split_attention_matches_float64(gpu, hd, nh, nkv):
    rng = np.random.default_rng([61, hd, nh, nkv])
    q, Kg, Vg = (rng.standard_normal(s, dtype=np.float32) for s in ((nh * hd,), (MAXTOK, nkv, hd), (MAXTOK, nkv, hd)))
    qd, worst = dev(q), 0.0
    for pos in POSITIONS:
        kc, vc = group_caches(Kg, Vg, pos, nh, MAXTOK)
        want = want_of(q, Kg, Vg, pos, nh)
        outs = {S: call(gpu, qd, kc, vc, pos, nh, nkv, hd, MAXTOK, S) for S in SPLITS}
        worst = max([worst] + [check(o, want, (hd, nh, nkv, pos, S)) for S, o in outs.items()])
        assert torch.equal(outs[3].view(torch.int32), call(gpu, qd, kc, vc, pos, nh, nkv, hd, MAXTOK, 3).view(torch.int32)), "not repeatable"
    print(f"attention_split headDim {hd} heads {nh}/{nkv}: worst error over the bar {worst / BAR_REL:.3g}")


def test_split_attention_at_the_cap(gpu):
    nh, nkv, hd, pos, maxTokens = 8, 2, 128, 8191, 8192
    rng = np.random.default_rng([62])
    q, Kg, Vg = (rng.standard_normal(s, dtype=np.float32) for s in ((nh * hd,), (maxTokens, nkv, hd), (maxTokens, nkv, hd)))
    kc, vc = group_caches(Kg, Vg, pos, nh, maxTokens)
    want = want_of(q, Kg, Vg, pos, nh)
    for S in (0, 7, 64):
        check(call(gpu, dev(q), kc, vc, pos, nh, nkv, hd, maxTokens, S), want, ("cap", S))
    check(call(gpu, dev(q), kc, vc, 9000, nh, nkv, hd, maxTokens, 0), want, "a position past the cache is clamped, as effort_attention clamps")


@pytest.mark.parametrize("target", (1030, 0))
def test_split_attention_weighs_a_marker_key(gpu, target):
    """The whole softmax mass on ONE key, in the last live split or in the first (8 splits of 17 tiles: 6 and 7 are empty): key `target` of
    a group is c * q, its score 40; V row t is t + 1, so every output is target + 1 unless a split's weight in the merge is wrong."""
    nh, nkv, hd, pos = 8, 2, 128, 1030
    rng = np.random.default_rng([63, target])
    qg = rng.standard_normal((nkv, hd), dtype=np.float32)
    q = np.repeat(qg, nh // nkv, axis=0).reshape(-1)                              # the heads of a group ask the same question
    Kg = rng.standard_normal((MAXTOK, nkv, hd), dtype=np.float32)
    Kg[target] = qg * (40.0 * np.sqrt(hd) / (qg.astype(np.float64) ** 2).sum(axis=1))[:, None].astype(np.float32)
    Vg = np.broadcast_to(np.arange(1, MAXTOK + 1, dtype=np.float32)[:, None, None], Kg.shape).copy()
    kc, vc = group_caches(Kg, Vg, pos, nh, MAXTOK)
    want = want_of(q, Kg, Vg, pos, nh)
    assert abs(want - (target + 1)).max() < 1e-6 * (target + 1)
    for S in (8, 3, 0):
        check(call(gpu, dev(q), kc, vc, pos, nh, nkv, hd, MAXTOK, S), want, ("marker", target, S))


def test_split_attention_replays_from_a_graph(gpu):
    """effort_rope_kv + effort_attention_split captured ONCE, replayed at positions 0 .. 70 with the device position incremented between
    replays, against the reference over its own growing float64 cache -- and against the eager calls' bits at every step."""
    nh, nkv, hd, steps, maxTokens, rope = 4, 2, 128, 71, 128, C.c_float(ROPE_BASE)
    rng = np.random.default_rng([64])
    xs = [tuple(rng.standard_normal(n * hd, dtype=np.float32) for n in (nh, nkv, nkv)) for _ in range(steps)]
    scratch = nans(lib().effort_attention_split_scratch_bytes(nh, hd, 2) // 4)
    bufs = {}
    for mode in ("eager", "graph"):
        xq, xk, xv, qr, out = (torch.zeros(n * hd, device="cuda:0") for n in (nh, nkv, nkv, nh, nh))
        kc, vc, posd = nans(maxTokens, nh, hd), nans(maxTokens, nh, hd), torch.zeros(1, dtype=torch.int32, device="cuda:0")

        def step():
            gpu._bind_stream()
            gpu.check(lib().effort_rope_kv(gpu.ctx, P(xq), P(xk), P(xv), P(qr), P(kc), P(vc), P(posd), nh, nkv, hd, maxTokens, rope), "rope_kv")
            gpu.check(lib().effort_attention_split(gpu.ctx, P(qr), P(kc), P(vc), P(posd), P(out), P(scratch), nh, nkv, hd, maxTokens, 2), "attention_split")
        gr = None
        if mode == "graph":
            step()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                step()
            gpu._bind_stream()
        got = []
        for a, b, c in xs:
            xq.copy_(dev(a)), xk.copy_(dev(b)), xv.copy_(dev(c))
            gr.replay() if gr else step()
            got.append(out.clone())
            posd += 1
        gpu.eval()
        bufs[mode] = got
    K, V = np.zeros((0, nh, hd)), np.zeros((0, nh, hd))
    for pos, (a, b, c) in enumerate(xs):
        want, kNew, vNew = ref.rope_attention(a, b, c, K, V, pos, nh, nkv, hd, ROPE_BASE)
        K, V = np.concatenate([K, kNew[None]]), np.concatenate([V, vNew[None]])
        check(bufs["graph"][pos], want, ("replay", pos))
        assert torch.equal(bufs["graph"][pos].view(torch.int32), bufs["eager"][pos].view(torch.int32)), pos


def test_split_attention_refusals_write_nothing(gpu):
    nh, nkv, hd, maxTokens = 8, 2, 64, 64
    q, kc, vc, out, sc = dev(np.ones(nh * hd, dtype=np.float32)), nans(maxTokens, nh, hd), nans(maxTokens, nh, hd), nans(nh * hd), nans(nh * 64 * (hd + 2))
    posd = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    f, ok = lib().effort_attention_split, [gpu.ctx, P(q), P(kc), P(vc), P(posd), P(out), P(sc), nh, nkv, hd, maxTokens, 2]
    for i in range(7):                                                            # a null argument, the scratch included
        assert f(*(ok[:i] + [None] + ok[i + 1:])) == -1, i
    for i, bad in ((7, 6), (7, 24), (8, 3), (8, 0), (9, 96), (9, 512), (10, 0), (10, 8193)):   # R = 3, R = 12, numHeads % numHeadsKV, ...
        assert f(*(ok[:i] + [bad] + ok[i + 1:])) == -2, (i, bad)
    for bad in (-1, 65):
        assert f(*(ok[:11] + [bad])) == -1, bad
    gpu.eval()
    assert bool(torch.isnan(out).all()) and bool(torch.isnan(sc).all())


@pytest.mark.parametrize("how,key", [(dict(dense=True), "dense"), (dict(effort=1.0), 1.0)])
def test_decoder_with_split_attention(small_model, how, key):  # noqa: F811
    """Teacher-forced, 40 steps, on the steps tests/test_gpu_decode.py holds to its 2e-3: the dense path and effort 1.0.  (At effort 0.25
    the multiply's row selection is discontinuous in its input: the existing two-launch attention sits 0.067 of max|logit| from the
    one-launch attention there, and the split attention the same 0.067 -- no attention path is within 2e-3 of another at that effort.)"""
    from effort_amd.decode import Decoder
    forced = [int(t) for t in np.random.default_rng([65]).integers(0, 512, 40)]
    plain = Decoder(small_model, maxTokens=64)
    ids, _, logits = plain.run(forced, 40, forced=True, collect_logits=True, **how)
    assert list(plain._graphs) == [(key,)]
    for start in (0, 20):
        dec = Decoder(small_model, maxTokens=64, split_attention_from=start)
        ids_s, _, logits_s = dec.run(forced, 40, forced=True, collect_logits=True, **how)
        assert sorted(dec._graphs, key=len) == [(key,), (key, "split")]
        err = float((logits_s - logits).abs().max() / logits.abs().max())
        print(f"split_attention_from={start}: logits within {err:.3g} of max|logit| of the plain loop's")
        assert ids_s == ids and err < 2e-3, (start, err)
