"""The generation rules on the GPU (effort_amd/csrc/rules.hip through effort_logit_rules, and the Decoder around it) against the numpy
specification of effort_amd/rules.py.

No tolerances and no excluded cases: the rule arithmetic is exact in float32 (one rounded operation per step), so the ruled logits are
compared as uint32, with ``seq``, ``stop_pos`` and bit 0 of the decode status beside them; a greedy pick is rank 0 of ``topk_reference``."""
import ctypes as C
import struct

import numpy as np
import pytest
import torch

from effort_amd.rules import NO_STOP, Rules, rules_reference
from effort_amd.sampling import Sampling, topk_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INF = float("inf")
FMT = "<ffffIIII8I"

NS = (1, 2, 63, 64, 65, 512, 4095, 32000, 32768, 32769, 70001)
FAMILIES = ("gauss", "ties", "special")
SEQ_LEN = 1100                                              # a full window of 1024 fits, and so does a position behind it
LAST_NS = (0, 1, 64, 1024, 5000)                            # 5000: clamped to 1024 on the device
POS_KINDS = ("0", "1", "W-1", "W", "end-1", "end")          # end = seqLen: past the buffer
WINDOW_KINDS = ("one", "distinct", "mix")
RULESETS = ("rep", "presence", "frequency", "bias", "min_p", "all")
BIAS_SIZES = (0, 1, 256)
MIN_PS = (1.0, 0.05, 0.0)                                   # 0.0: off


def make_row(family: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(77 * FAMILIES.index(family) + n)
    g = (rng.standard_normal(n) * 3.0).astype(np.float32)
    if family == "ties":                                    # a handful of levels, both signs and the zeros among them
        g = (np.clip(np.floor(g), -3, 3) * np.float32(0.5)).astype(np.float32)
    if family == "special":                                 # NaN (one with a payload), both infinities, -0.0: at the ids the windows and tables name
        spots = np.unique(np.concatenate([np.arange(min(n, 12)), rng.integers(0, n, size=min(n, 40))]))
        vals = np.array([np.nan, INF, -INF, -0.0, 0.0], dtype=np.float32)
        g[spots] = vals[np.arange(spots.size) % 5]
        if n > 5:
            g.view(np.uint32)[5] = 0xFFC12345
    return g


def make_window(kind: str, n: int, seed: int):
    """seq, uint32 [SEQ_LEN]: what the steps before consumed."""
    rng = np.random.default_rng(seed)
    if kind == "one":
        seq = np.full(SEQ_LEN, min(3, n - 1), dtype=np.uint32)
    elif kind == "distinct":                                # all different; those >= n (every n below 1100 has some) are ignored
        seq = rng.permutation(max(n, SEQ_LEN)).astype(np.uint32)[:SEQ_LEN]
    else:                                                   # repeats out of a small pool, ids >= n and 0xFFFFFFFF among them
        pool = np.concatenate([rng.integers(0, n, size=24), np.arange(min(n, 12)), [n, n + 7, 0xFFFFFFFF]]).astype(np.uint32)
        seq = pool[rng.integers(0, pool.size, size=SEQ_LEN)]
    return seq


def make_bias(size: int, n: int, seed: int):
    """The two 256-entry tables with ``size`` entries meant: duplicates, ids >= n, -inf, +inf and NaN values among 256; zeros behind."""
    rng = np.random.default_rng(seed)
    ids, vals = np.zeros(256, dtype=np.uint32), np.zeros(256, dtype=np.float32)
    if size == 1:
        ids[0], vals[0] = min(3, n - 1), -1.5
    elif size:
        pool = np.concatenate([rng.integers(0, n, size=90), np.arange(min(n, 12)), [n, n + 1, 0xFFFFFFFF]]).astype(np.uint32)
        ids[:] = pool[rng.integers(0, pool.size, size=256)]
        vals[:] = (rng.standard_normal(256) * 2.0).astype(np.float32)
        r = rng.random(256)
        vals[r < 0.06] = -INF
        vals[(r >= 0.06) & (r < 0.10)] = INF
        vals[(r >= 0.10) & (r < 0.16)] = np.nan
    return ids, vals


def pack(rep=1.0, presence=0.0, frequency=0.0, min_p_log=-INF, last_n=0, n_bias=0, n_stop=0, first_pos=0, stops=()):
    stops = list(stops) + [0] * (8 - len(stops))
    return struct.pack(FMT, rep, presence, frequency, min_p_log, last_n, n_bias, n_stop, first_pos, *stops)


def ruleset_params(ruleset: str, last_n: int, bias_size: int, min_p: float, tok: int, pos: int) -> bytes:
    on = lambda name: ruleset in (name, "all")               # noqa: E731
    stops = (9, tok & 0xFFFFFFFF) if ruleset == "all" else ()
    return pack(rep=1.3 if on("rep") else 1.0, presence=0.4 if on("presence") else 0.0, frequency=0.15 if on("frequency") else 0.0,
                min_p_log=Rules(min_p=min_p).min_p_log() if on("min_p") else -INF, last_n=last_n, n_bias=bias_size if on("bias") else 0,
                n_stop=len(stops), first_pos=pos if pos % 2 else pos + 1, stops=stops)


@pytest.fixture(scope="module")
def gpu(hip_lib_built):
    import effort_amd
    torch.cuda.set_device(0)
    g = effort_amd.gpu()
    g._bind_stream()
    return g


def p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def dev_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32).copy()).to(DEV)


def status(g) -> int:
    from effort_amd import _lib
    st = C.c_int(0)
    g.check(_lib.lib().effort_decode_status(g.ctx, C.byref(st)), "decode_status")
    return int(st.value)


def launch(g, x_dev, n, raw, seq=None, pos=0, tok=None, bias=None, stop0=None, inplace=False):
    """One effort_logit_rules call.  Returns (out as uint32 numpy, seq after as uint32 or None, stop_pos after or None, status word)."""
    from effort_amd import _lib
    lib = _lib.lib()
    par = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(DEV)
    pos_d = dev_u32([pos])
    seq_d = dev_u32(seq) if seq is not None else None
    tok_d = dev_u32([tok]) if tok is not None else None
    ids_d, vals_d = (dev_u32(bias[0]), torch.from_numpy(bias[1].copy()).to(DEV)) if bias is not None else (None, None)
    stop_d = dev_u32([stop0]) if stop0 is not None else None
    out = x_dev.clone() if inplace else torch.full((n,), 12345.0, dtype=torch.float32, device=DEV)
    src = out if inplace else x_dev
    g.check(lib.effort_logit_rules(g.ctx, p(src), n, p(par), p(tok_d), p(pos_d), p(seq_d), 0 if seq is None else int(seq_d.numel()), p(ids_d), p(vals_d),
                                   p(stop_d), p(out)), "logit_rules")
    st = status(g)                                           # (synchronises)
    assert int(pos_d.item()) == np.array([pos], dtype=np.uint32).view(np.int32)[0]              # read, never advanced
    u32 = lambda t: t.cpu().numpy().view(np.uint32)          # noqa: E731
    return u32(out), (u32(seq_d) if seq_d is not None else None), (int(u32(stop_d)[0]) if stop_d is not None else None), st


def check(g, x, x_dev, raw, seq, pos, tok, bias, stop0, what, inplace=False):
    got = launch(g, x_dev, x.size, raw, seq, pos, tok, bias, stop0, inplace)
    ids, vals = bias if bias is not None else (None, None)
    want_out, want_seq, want_stop, want_st = rules_reference(x, raw, seq, pos, tok, ids, vals, stop0)
    assert got[3] == want_st, (what, "status", got[3], want_st)
    assert got[2] == want_stop, (what, "stop_pos", got[2], want_stop)
    if seq is not None:
        assert np.array_equal(got[1], want_seq), (what, "seq")
    bad = np.flatnonzero(got[0] != want_out.view(np.uint32))
    assert bad.size == 0, (what, "out", bad[:8].tolist(), got[0][bad[:8]].tolist(), want_out.view(np.uint32)[bad[:8]].tolist())
    return got


# ---------------------------------------------------------------- the kernel against the specification
@pytest.fixture(scope="module")
def rows():
    """Host and device copies of every (family, n) row, made once and never modified."""
    out = {}
    for f in FAMILIES:
        for n in NS:
            x = make_row(f, n)
            out[f, n] = (x, torch.from_numpy(x).to(DEV))
    return out


def schedule(n: int, family: str):
    """Every window length at every position kind; beside them a walk through the 162 combinations of window kind, rule set, bias table
    size and min_p at a stride coprime to 162, continued from row to row: over the rows every combination comes up."""
    first = 31 * (NS.index(n) * len(FAMILIES) + FAMILIES.index(family))
    i = 0
    for last_n in LAST_NS:
        for pos_kind in POS_KINDS:
            W = min(last_n, 1024)
            pos = {"0": 0, "1": 1, "W-1": max(W - 1, 0), "W": W, "end-1": SEQ_LEN - 1, "end": SEQ_LEN}[pos_kind]
            c = (first + i) * 37 % 162
            yield (last_n, pos, WINDOW_KINDS[c % 3], RULESETS[c // 3 % 6], BIAS_SIZES[c // 18 % 3], MIN_PS[c // 54], i)
            i += 1


def test_the_schedule_covers_what_it_claims():
    seen = {k: set() for k in ("last_n", "pos", "kind", "rules", "bias", "min_p", "all four", "last_n_rules", "pos_rules")}
    for n in NS:
        for f in FAMILIES:
            for last_n, pos, kind, ruleset, bias_size, min_p, _ in schedule(n, f):
                for k, v in (("last_n", last_n), ("pos", pos), ("kind", kind), ("rules", ruleset), ("bias", bias_size), ("min_p", min_p),
                             ("all four", (kind, ruleset, bias_size, min_p)), ("last_n_rules", (last_n, ruleset)), ("pos_rules", (pos, ruleset))):
                    seen[k].add(v)
    assert seen["last_n"] == set(LAST_NS) and seen["kind"] == set(WINDOW_KINDS) and seen["rules"] == set(RULESETS)
    assert {0, 1, 63, 64, 1023, 1024, SEQ_LEN - 1, SEQ_LEN} <= seen["pos"]
    assert len(seen["all four"]) == 162 and len(seen["last_n_rules"]) == 30 and len(seen["pos_rules"]) == 6 * len(seen["pos"])


@pytest.mark.parametrize("n", NS)
def test_kernel_matches_the_specification(gpu, rows, n):
    gpu._bind_stream()
    assert status(gpu) >= 0                                  # (clears whatever an earlier test left)
    for family in FAMILIES:
        x, x_dev = rows[family, n]
        for last_n, pos, kind, ruleset, bias_size, min_p, i in schedule(n, family):
            seq = make_window(kind, n, 1000 * n + i)
            tok = int(seq[(pos + 17) % SEQ_LEN])             # a token of the window's kind
            raw = ruleset_params(ruleset, last_n, bias_size, min_p, tok, pos)
            bias = make_bias(bias_size, n, 31 * n + i)
            check(gpu, x, x_dev, raw, seq, pos, tok, bias, NO_STOP, (n, family, last_n, pos, kind, ruleset, bias_size, min_p))


def test_every_rule_off_is_the_identity(gpu, rows):
    gpu._bind_stream()
    for n in (1, 65, 32000):
        x, x_dev = rows["special", n]
        seq = make_window("mix", n, 5)
        for raw in (Rules().pack(), Rules(last_n=1024).pack(), Rules(last_n=0).pack()):
            got = check(gpu, x, x_dev, raw, seq, 1050, int(seq[3]), make_bias(0, n, 0), NO_STOP, (n, "identity"))
            assert np.array_equal(got[0], x.view(np.uint32))
        got = check(gpu, x, x_dev, Rules().pack(), None, 7, None, None, None, (n, "identity, no seq, no tables, no stop"))
        assert np.array_equal(got[0], x.view(np.uint32))


def test_device_values_are_sanitised(gpu, rows):
    """The struct is device memory no host validated."""
    gpu._bind_stream()
    n = 4095
    x, x_dev = rows["gauss", n]
    seq = make_window("mix", n, 11)
    bias = make_bias(256, n, 12)
    tok = int(seq[0])
    for rep in (float("nan"), -1.5, 0.0, INF, -INF):
        for pen in (float("nan"), INF, -INF):
            raw = pack(rep=rep, presence=pen, frequency=pen, min_p_log=0.7, last_n=0xFFFFFFFF, n_bias=10000, n_stop=99, first_pos=0,
                       stops=(1, 2, 3, 4, 5, 6, 7, tok))
            got = check(gpu, x, x_dev, raw, seq, 1060, tok, bias, NO_STOP, ("sanitise", rep, pen))
            assert got[2] == 1060                            # the eighth stop id counts, a ninth does not exist
    # sanitised penalties are off, the clamped table and window are not: against the same call written with legal values
    legal = pack(last_n=1024, n_bias=256, n_stop=8, stops=(1, 2, 3, 4, 5, 6, 7, tok))
    a = launch(gpu, x_dev, n, legal, seq, 1060, tok, bias, NO_STOP)
    b = launch(gpu, x_dev, n, pack(rep=float("nan"), presence=INF, frequency=float("nan"), min_p_log=float("nan"), last_n=5000, n_bias=257, n_stop=9,
                                   stops=(1, 2, 3, 4, 5, 6, 7, tok)), seq, 1060, tok, bias, NO_STOP)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2] == 1060
    # one finite penalty beside a sanitised one still acts
    check(gpu, x, x_dev, pack(rep=float("nan"), presence=0.5, frequency=INF, min_p_log=-0.0, last_n=64), seq, 100, tok, bias, NO_STOP, "partly sane")


def test_in_place_equals_out_of_place(gpu, rows):
    gpu._bind_stream()
    for n, family in ((63, "special"), (32000, "gauss"), (32769, "ties"), (70001, "special")):
        x, x_dev = rows[family, n]
        seq = make_window("mix", n, 3)
        bias = make_bias(256, n, 4)
        tok = int(seq[5])
        raw = pack(rep=1.2, presence=0.3, frequency=0.1, min_p_log=Rules(min_p=0.05).min_p_log(), last_n=1024, n_bias=256, n_stop=1, stops=(tok,))
        a = check(gpu, x, x_dev, raw, seq, 1070, tok, bias, NO_STOP, (n, family, "out of place"))
        b = check(gpu, x, x_dev, raw, seq, 1070, tok, bias, NO_STOP, (n, family, "in place"), inplace=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]
        assert np.array_equal(x.view(np.uint32), x_dev.cpu().numpy().view(np.uint32))        # the shared row is untouched


def test_refusals_enqueue_nothing(gpu, rows):
    from effort_amd import _lib
    lib = _lib.lib()
    gpu._bind_stream()
    n = 64
    x, x_dev = rows["gauss", n]
    par = torch.frombuffer(bytearray(pack(rep=2.0, last_n=64, n_bias=1, n_stop=1, stops=(3,))), dtype=torch.uint8).to(DEV)
    tok, pos, seq = dev_u32([3]), dev_u32([2]), dev_u32(np.full(8, 3))
    ids, vals = dev_u32(np.zeros(256)), torch.ones(256, device=DEV)
    stop = dev_u32([NO_STOP])
    out = torch.full((n,), 777.0, device=DEV)
    ok = (p(x_dev), n, p(par), p(tok), p(pos), p(seq), 8, p(ids), p(vals), p(stop), p(out))

    def refused(**change):
        names = ("logits_in", "n", "params", "tok", "pos", "seq", "seqLen", "bias_ids", "bias_vals", "stop_pos", "logits_out")
        args = [change.get(k, v) for k, v in zip(names, ok)]
        return lib.effort_logit_rules(gpu.ctx, *args)
    for change in (dict(n=0), dict(n=-5), dict(seqLen=-1), dict(logits_in=None), dict(logits_out=None), dict(params=None), dict(pos=None),
                   dict(tok=None), dict(seq=None), dict(bias_ids=None), dict(bias_vals=None)):
        assert refused(**change) == -1, change
    assert lib.effort_logit_rules(None, *ok) == -1
    gpu.eval()
    assert (out == 777.0).all() and int(pos.item()) == 2 and int(stop.item()) == -1 and seq.cpu().tolist() == [3] * 8 and status(gpu) == 0
    # the pairs may both be absent, and stop_pos too
    assert refused(tok=None, seq=None, seqLen=0, bias_ids=None, bias_vals=None, stop_pos=None) == 0
    gpu.eval()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), x.view(np.uint32)) and status(gpu) == 0


def test_one_captured_graph_serves_every_setting(gpu, rows):
    """effort_logit_rules + effort_argmax captured once; eight replays, the params tensor rewritten between them: every replay is the
    specification for the settings it found, the pick is rank 0 of the ruled row, and seq grows by one each time."""
    from effort_amd import _lib
    lib = _lib.lib()
    n = 32000
    x, x_dev = rows["gauss", n]
    par, ids, vals = Rules().to_device(device=DEV)
    tok, pos, seq, stop = dev_u32([int(np.argmax(x))]), dev_u32([0]), dev_u32(np.zeros(16)), dev_u32([NO_STOP])
    hist = dev_u32(np.zeros(16))
    out = torch.zeros(n, device=DEV)

    def step():
        gpu._bind_stream()
        gpu.check(lib.effort_logit_rules(gpu.ctx, p(x_dev), n, p(par), p(tok), p(pos), p(seq), 16, p(ids), p(vals), p(stop), p(out)), "logit_rules")
        gpu.check(lib.effort_argmax(gpu.ctx, p(out), n, p(tok), p(pos), p(hist), 16), "argmax")
    step()                                                   # warm
    torch.cuda.synchronize()
    tok.copy_(dev_u32([int(np.argmax(x))])), pos.zero_(), seq.zero_(), hist.zero_()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        step()
    gpu._bind_stream()
    top = topk_reference(x, 8)[0].tolist()
    settings = [Rules(repetition_penalty=1.5, last_n=4), Rules(frequency_penalty=3.0, last_n=16), Rules(logit_bias={top[0]: -INF, top[1]: -INF}),
                Rules(min_p=0.5, presence_penalty=20.0, last_n=2), Rules(), Rules(repetition_penalty=4.0, last_n=1024, stop_ids=(top[2], top[0])),
                Rules(logit_bias={t: 5.0 - i for i, t in enumerate(top)}, min_p=0.05), Rules(presence_penalty=100.0, frequency_penalty=-1.0)]
    want_seq, want_stop = np.zeros(16, dtype=np.uint32), NO_STOP
    cur = int(np.argmax(x))
    for i, r in enumerate(settings):
        r.to_device(3, par, ids, vals)
        gr.replay()
        torch.cuda.synchronize()
        want_out, want_seq, want_stop, st = rules_reference(x, r.pack(3), want_seq, i, cur, *r.bias_tables(), want_stop)
        assert st == 0 and np.array_equal(out.cpu().numpy().view(np.uint32), want_out.view(np.uint32)), i
        assert np.array_equal(seq.cpu().numpy().view(np.uint32), want_seq) and want_seq[:i + 1].tolist() == ([int(np.argmax(x))] + hist.cpu().tolist()[:i]), i
        cur = int(topk_reference(want_out, 1)[0][0])
        assert int(tok.item()) == cur == int(hist[i].item()) and int(pos.item()) == i + 1, i
        assert int(stop.cpu().numpy().view(np.uint32)[0]) == want_stop, i
    assert want_stop != NO_STOP and status(gpu) == 0         # (the sixth setting's stop ids met a token past first_pos)


# ---------------------------------------------------------------- the decoder
@pytest.fixture(scope="module")
def small_model(hip_lib_built):
    import effort_amd  # noqa: F401
    from effort_amd.decode import MistralConfig, Model
    cfg = MistralConfig(stateDim=4096, hiddenDim=4096, numLayers=2, numHeads=32, numHeadsKV=8, headDim=128, vocab=512)
    return Model.random(cfg, seed=5)


PROMPT, STEPS, EFFORT = [3, 77, 130], 16, 0.5


class Replays:
    """Stands in for a captured graph of a Decoder: counts the replays and keeps a copy of ``logits_ruled`` after each."""

    def __init__(self, dec, gr):
        self.dec, self.gr, self.count, self.ruled = dec, gr, 0, []

    def replay(self):
        self.gr.replay()
        self.count += 1
        self.ruled.append(self.dec.logits_ruled.clone())


def watch(dec):
    w = {}
    for key, gr in list(dec._graphs.items()):
        if "rules" in key and not isinstance(gr, Replays):
            dec._graphs[key] = w[key] = Replays(dec, gr)
    return w


def bits(t):
    return t.cpu().numpy().view(np.uint32)


def test_decoder_default_rules_are_the_plain_run(small_model):
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=32)
    ids, _, lg = dec.run(PROMPT, STEPS, effort=EFFORT, collect_logits=True)
    assert not dec._rules and dec.stopped_at is None
    n_graphs = len(dec._graphs)
    ids_r, _, lg_r = dec.run(PROMPT, STEPS, effort=EFFORT, collect_logits=True, rules=Rules())
    assert len(dec._graphs) == n_graphs + 1                  # the first Rules added exactly one graph
    assert ids_r == ids and np.array_equal(bits(lg_r), bits(lg)) and dec.stopped_at is None
    assert np.array_equal(bits(dec.logits_ruled), bits(dec.logits))
    ids_2, _, _ = dec.run(PROMPT, STEPS, effort=EFFORT, rules=Rules(repetition_penalty=1.8, last_n=32, logit_bias={ids[5]: -INF}))
    assert len(dec._graphs) == n_graphs + 1                  # a second Rules adds none
    assert ids_2 != ids and ids[5] not in ids_2[len(PROMPT) - 1:]
    assert dec.run(PROMPT, STEPS, effort=EFFORT)[0] == ids and len(dec._graphs) == n_graphs + 1   # the plain graph is still the plain step
    assert dec.status() == 0


def test_decoder_penalised_greedy_run_replayed_on_the_host(small_model):
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=32)
    r = Rules(repetition_penalty=1.3, frequency_penalty=0.2, last_n=8)
    ids, _, lg = dec.run(PROMPT, STEPS, effort=EFFORT, collect_logits=True, rules=r)
    raw, (b_ids, b_vals) = r.pack(len(PROMPT)), r.bias_tables()
    seq, lg = np.zeros(32, dtype=np.uint32), lg.cpu().numpy()
    for step in range(STEPS):
        tok = PROMPT[step] if step < len(PROMPT) else ids[step - 1]
        out, seq, _, st = rules_reference(lg[step], raw, seq, step, tok, b_ids, b_vals, NO_STOP)
        assert st == 0 and ids[step] == int(topk_reference(out, 1)[0][0]), step
        assert out[tok] != lg[step][tok]                     # (the token just fed is in the window: its logit moved, whatever its sign)
    assert np.array_equal(bits(dec.logits_ruled), out.view(np.uint32))
    assert bits(dec.seq)[:STEPS].tolist() == PROMPT + ids[len(PROMPT) - 1:STEPS - 1] == seq[:STEPS].tolist()


def test_decoder_stops_at_a_stop_token(small_model):
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=32)
    steps = 30
    plain = dec.run(PROMPT, steps, effort=EFFORT)[0]
    P = len(PROMPT)
    k = next(k for k in range(P, steps - 8) if plain[k] not in plain[P - 1:k] and PROMPT[1] not in plain[P - 1:k + 1])
    stop = Rules(stop_ids=(plain[k], PROMPT[1]))             # the second id is fed inside the prompt: it does not stop the run there
    dec.run(PROMPT, steps, effort=EFFORT, rules=Rules())      # (the ruled graph exists: wrap it)
    w = watch(dec)
    assert len(w) == 1
    counter = next(iter(w.values()))
    ids, _, lg = dec.run(PROMPT, steps, effort=EFFORT, rules=stop, stop_poll=4, collect_logits=True)
    assert ids == plain[:k + 1] and ids[-1] == plain[k] and dec.stopped_at == k and lg.shape[0] == k + 1
    assert k + 2 <= counter.count <= k + 1 + 4               # it ran on to the next poll, not to the end
    assert int(dec.pos.item()) == k + 1 and int(dec.tokId.item()) == plain[k]
    assert int(bits(dec.stop_pos)[0]) == k + 1               # the step that consumed it
    assert dec.status() == 0
    # the last step's pick counts, though no step consumed it
    counter.count = 0
    ids, _, _ = dec.run(PROMPT, k + 1, effort=EFFORT, rules=stop, stop_poll=4)
    assert ids == plain[:k + 1] and dec.stopped_at == k and counter.count == k + 1 and int(bits(dec.stop_pos)[0]) == NO_STOP
    # no stop id picked: the whole run, stopped_at None
    ids, _, _ = dec.run(PROMPT, k, effort=EFFORT, rules=stop, stop_poll=1)
    assert ids == plain[:k] and dec.stopped_at is None
    # forced: nothing stops
    forced = plain[:k + 4]
    ids, _, _ = dec.run(forced, k + 4, effort=EFFORT, rules=stop, forced=True, stop_poll=1)
    assert len(ids) == k + 4 and dec.stopped_at is None and bits(dec.seq)[:k + 4].tolist() == forced
    assert dec.status() == 0


def test_decoder_sampled_run_with_rules(small_model):
    from effort_amd import _lib
    from effort_amd.decode import Decoder
    lib = _lib.lib()
    dec = Decoder(small_model, maxTokens=32)
    s = Sampling(temperature=1.1, top_k=40, top_p=0.9, seed=77)
    r = Rules(repetition_penalty=1.4, presence_penalty=0.3, last_n=16, min_p=0.02, logit_bias={5: -INF, 9: 2.0})
    dec.run(PROMPT, 4, effort=EFFORT, sampling=s, rules=r)
    assert sorted(dec._graphs) == [(EFFORT, "sampled", "rules")]
    counter = next(iter(watch(dec).values()))
    ids, _, lg = dec.run(PROMPT, STEPS, effort=EFFORT, sampling=s, rules=r, collect_logits=True)
    assert counter.count == STEPS
    g = dec.g
    g._bind_stream()
    par = s.to_device(device=DEV)
    raw, (b_ids, b_vals) = r.pack(len(PROMPT)), r.bias_tables()
    seq, lg = np.zeros(32, dtype=np.uint32), lg.cpu().numpy()
    for step in range(STEPS):
        tok = PROMPT[step] if step < len(PROMPT) else ids[step - 1]
        out, seq, _, _ = rules_reference(lg[step], raw, seq, step, tok, b_ids, b_vals, NO_STOP)
        assert np.array_equal(bits(counter.ruled[step]), out.view(np.uint32)), step
        got, pos = dev_u32([0]), dev_u32([step])
        g.check(lib.effort_sample(g.ctx, p(counter.ruled[step]), 512, p(par), p(got), p(pos), None, 0, None, None), "sample")
        assert int(got.item()) == ids[step], step
    assert 5 not in ids and dec.status() == 0


def test_decoder_prefill_with_rules(small_model):
    from effort_amd.decode import Decoder
    dec = Decoder(small_model, maxTokens=32)
    prompt = [3, 77, 130, 9, 77, 401, 77]
    P = len(prompt)
    r = Rules(repetition_penalty=1.5, frequency_penalty=0.25, last_n=6, stop_ids=(77,))
    dec.run(prompt, 2, effort=EFFORT, rules=r)
    counter = next(iter(watch(dec).values()))
    ids, _, lg = dec.run(prompt, 12, effort=EFFORT, rules=r, prefill=True, collect_logits=True)
    assert ids[:P - 1] == [-1] * (P - 1)
    seq = bits(dec.seq)
    assert seq[:P - 1].tolist() == prompt[:P - 1] and seq[P - 1] == prompt[P - 1]
    host_seq = np.zeros(32, dtype=np.uint32)
    host_seq[:P - 1] = prompt[:P - 1]
    out, host_seq, stop, st = rules_reference(lg[0].cpu().numpy(), r.pack(P), host_seq, P - 1, prompt[P - 1], *r.bias_tables(), NO_STOP)
    assert np.array_equal(bits(counter.ruled[0]), out.view(np.uint32)) and st == 0
    assert stop == NO_STOP                                   # 77 is fed as the last prompt token: below first_pos
    assert not np.array_equal(out.view(np.uint32), bits(lg[0]))                               # the window reached into the prefilled ids
    assert ids[P - 1] == int(topk_reference(out, 1)[0][0])
    end = len(ids)
    assert seq[P:end].tolist() == ids[P - 1:end - 1] and dec.status() == 0
