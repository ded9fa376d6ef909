"""The generation rules on the host (effort_amd/rules.py): the packed struct against include/effort_hip.h, the dataclass's refusals, and
``rules_reference`` -- the numpy restatement of effort_logit_rules' specification -- on hand-made rows whose answers are written out."""
import math
import os
import re
import struct

import numpy as np
import pytest

from effort_amd.rules import MAX_BIAS, MAX_STOP, MAX_WINDOW, NO_STOP, Rules, rules_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
f32 = np.float32


def bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32).tolist()


# ---------------------------------------------------------------- the struct
def test_pack_follows_the_header():
    src = open(os.path.join(ROOT, "include", "effort_hip.h")).read()
    for name, want in (("WINDOW", MAX_WINDOW), ("BIAS", MAX_BIAS), ("STOP", MAX_STOP)):
        assert int(re.search(rf"#define EFFORT_RULES_MAX_{name}\s+(\d+)", src).group(1)) == want
    body = re.search(r"typedef struct effort_rules_params \{(.*?)\} effort_rules_params;", src, flags=re.S).group(1)
    fields = re.findall(r"^\s*(float|uint32_t)\s+(\w+)(\[\w+\])?;", re.sub(r"/\*.*?\*/", "", body), flags=re.M)
    assert [(t, n) for t, n, _ in fields] == [("float", "repetition_penalty"), ("float", "presence_penalty"), ("float", "frequency_penalty"),
                                             ("float", "min_p_log"), ("uint32_t", "last_n"), ("uint32_t", "n_bias"), ("uint32_t", "n_stop"),
                                             ("uint32_t", "first_pos"), ("uint32_t", "stop_ids")]
    assert fields[-1][2] == "[EFFORT_RULES_MAX_STOP]"
    r = Rules(repetition_penalty=1.25, presence_penalty=0.5, frequency_penalty=-0.75, last_n=100, min_p=0.05, logit_bias={7: 1.0, 9: -INF},
              stop_ids=(2, 0xFFFFFFFF, 31999))
    raw = r.pack(first_pos=17)
    assert len(raw) == 64
    assert struct.unpack_from("<fff", raw, 0) == (1.25, 0.5, -0.75)
    assert struct.unpack_from("<f", raw, 12)[0] == float(f32(math.log(0.05)))
    assert struct.unpack_from("<IIII", raw, 16) == (100, 2, 3, 17)
    assert struct.unpack_from("<8I", raw, 32) == (2, 0xFFFFFFFF, 31999, 0, 0, 0, 0, 0)
    # min_p_log: ln in f32 for 0 < min_p <= 1, else -inf
    for p, want in ((1.0, 0.0), (0.5, float(f32(math.log(0.5)))), (0.0, -INF), (-0.1, -INF), (1.5, -INF), (float("nan"), -INF)):
        assert struct.unpack_from("<f", Rules(min_p=p).pack(), 12)[0] == want, p
    raw = Rules().pack()
    assert struct.unpack("<ffffIIII8I", raw) == (1.0, 0.0, 0.0, -INF, 64, 0, 0, 0) + (0,) * 8
    ids, vals = r.bias_tables()
    assert ids.dtype == np.uint32 and vals.dtype == np.float32 and ids.shape == vals.shape == (256,)
    assert ids[:3].tolist() == [7, 9, 0] and vals[:3].tolist() == [1.0, -INF, 0.0]


def test_to_device_rewrites_in_place():
    import torch
    r = Rules(logit_bias={5: 2.0}, stop_ids=(4,))
    par, ids, vals = r.to_device(first_pos=3)
    assert par.dtype == torch.uint8 and bytes(par.numpy().tobytes()) == r.pack(3)
    assert ids.dtype == torch.int32 and vals.dtype == torch.float32 and ids.numel() == vals.numel() == 256
    r2 = Rules(repetition_penalty=2.0, logit_bias={0xFFFFFFFF: 1.0})
    got = r2.to_device(0, par, ids, vals)
    assert got[0] is par and got[1] is ids and got[2] is vals
    assert bytes(par.numpy().tobytes()) == r2.pack(0) and ids[0].item() == -1 and ids[1].item() == 0 and vals[0].item() == 1.0
    with pytest.raises(ValueError):
        r.to_device(0, torch.zeros(32, dtype=torch.uint8), ids, vals)
    with pytest.raises(ValueError):
        r.to_device(0, par, vals, ids)


@pytest.mark.parametrize("kw", [dict(last_n=-1), dict(last_n=1025), dict(last_n=1.5), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
                                dict(repetition_penalty=INF), dict(repetition_penalty=float("nan")), dict(presence_penalty=INF),
                                dict(frequency_penalty=float("nan")), dict(logit_bias={i: 0.0 for i in range(257)}), dict(stop_ids=tuple(range(9))),
                                dict(stop_ids=(-1,)), dict(stop_ids=(1 << 32,)), dict(logit_bias={-3: 1.0}), dict(logit_bias={1 << 32: 1.0}),
                                dict(logit_bias={1.5: 1.0})])
def test_validation_errors(kw):
    with pytest.raises(ValueError):
        Rules(**kw)


def test_the_limits_themselves_are_accepted():
    Rules(last_n=0), Rules(last_n=1024), Rules(logit_bias={i: float("nan") for i in range(256)}), Rules(stop_ids=tuple(range(8)))
    Rules(logit_bias={0xFFFFFFFF: -INF}, stop_ids=(0xFFFFFFFF,), repetition_penalty=1e-30)


# ---------------------------------------------------------------- rules_reference
def ref(x, rules=None, seq=None, pos=0, tok=None, stop_pos=None, first_pos=0, raw=None, bias=True):
    rules = rules or Rules()
    ids, vals = rules.bias_tables() if bias else (None, None)
    return rules_reference(np.asarray(x, dtype=np.float32), raw or rules.pack(first_pos), seq, pos, tok, ids, vals, stop_pos)


def test_identity_keeps_the_bits():
    x = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x3F800000, 0x00000001, 0x80000001],
                 dtype=np.uint32).view(np.float32)          # quiet and signalling NaNs with payloads, the zeros, the infinities, denormals
    seq = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], dtype=np.int32)
    # every rule off: the default, with a window over every element; last_n = 0; no seq at all
    for out, seq_after, stop, st in (ref(x, Rules(last_n=1024), seq, 9, 9), ref(x, Rules(last_n=0), seq, 9, 9), ref(x), ref(x, bias=False)):
        assert bits(out) == bits(x) and st == 0 and stop is None
    out, seq_after, _, _ = ref(x, Rules(), seq, 4, 77)
    assert seq_after.tolist() == [0, 1, 2, 3, 77, 5, 6, 7, 8, 9] and seq_after.dtype == np.uint32 and bits(out) == bits(x)
    assert out is not x


def test_repetition_penalty():
    x = [3.0, -3.0, 0.0, 5.0]
    out = ref(x, Rules(repetition_penalty=1.5), np.array([0, 1, 2, 0], np.int32), 2, 2)[0]
    assert out.tolist() == [2.0, -4.5, 0.0, 5.0]            # positive divided, negative multiplied, zero multiplied, outside the window untouched
    third = ref([1.0], Rules(repetition_penalty=3.0), np.zeros(1, np.int32), 0, 0)[0]
    assert bits(third) == bits(f32(1.0) / f32(3.0))         # the correctly rounded quotient, not 1 * f32(1/3)


def test_frequency_and_presence_by_count():
    x = [1.0, 1.0, 1.0, 1.0]
    seq = np.array([1, 2, 1, 3, 1, 0, 0, 0], np.int32)      # at pos 4: 1 three times, 2 and 3 once
    out = ref(x, Rules(frequency_penalty=0.25, presence_penalty=0.5, last_n=5), seq, 4, 1)[0]
    assert out.tolist() == [1.0, 1.0 - (3 * 0.25 + 0.5), 1.0 - (0.25 + 0.5), 1.0 - (0.25 + 0.5)]
    out = ref(x, Rules(frequency_penalty=0.25, last_n=2), seq, 4, 1)[0]                   # the window is seq[3..4] = 3, 1
    assert out.tolist() == [1.0, 0.75, 1.0, 0.75]
    out = ref(x, Rules(frequency_penalty=0.25, last_n=64), seq, 1, 2)[0]                  # W = pos + 1 = 2: seq[0..1] = 1, 2
    assert out.tolist() == [1.0, 0.75, 0.75, 1.0]
    # the order of the roundings: (f32(c) * f) + p, then l - that
    fr, pr, l = f32(0.1), f32(0.3), f32(0.7)
    out = ref([l], Rules(frequency_penalty=0.1, presence_penalty=0.3, last_n=3), np.zeros(3, np.int32), 2, 0)[0]
    assert bits(out) == bits(l - f32(f32(f32(3.0) * fr) + pr))
    rep = ref([l], Rules(repetition_penalty=1.1, frequency_penalty=0.1, presence_penalty=0.3, last_n=3), np.zeros(3, np.int32), 2, 0)[0]
    assert bits(rep) == bits(f32(l / f32(1.1)) - f32(f32(f32(3.0) * fr) + pr))


def test_bias_last_wins_and_bans():
    x = [1.0, 2.0, 3.0, 4.0]
    ids = np.zeros(256, np.uint32)
    vals = np.zeros(256, np.float32)
    ids[:5], vals[:5] = [2, 1, 2, 9, 2], [10.0, -INF, 20.0, 5.0, np.nan]          # 2 named three times, the last entry NaN = absent; 9 >= n
    raw = struct.pack("<ffffIIII8I", 1.0, 0.0, 0.0, -INF, 0, 5, 0, 0, *([0] * 8))
    out = rules_reference(np.array(x, np.float32), raw, None, 0, None, ids, vals, None)[0]
    assert out.tolist() == [1.0, -INF, 23.0, 4.0]
    out = rules_reference(np.array(x, np.float32), raw, None, 0, None, None, None, None)[0]        # without the tables n_bias counts as 0
    assert out.tolist() == x
    # a bias lands on the penalised value
    out = ref([4.0, 4.0], Rules(repetition_penalty=2.0, logit_bias={0: 1.0}), np.zeros(2, np.int32), 0, 0)[0]
    assert out.tolist() == [3.0, 4.0]
    # +inf + -inf: the canonical NaN; a NaN logit keeps its bits under a bias
    nan = np.array([0x7FC00123], np.uint32).view(np.float32)[0]
    out = ref([INF, nan, -INF], Rules(logit_bias={0: -INF, 1: 3.0, 2: INF}))[0]
    assert bits(out) == [0x7FC00000, 0x7FC00123, 0x7FC00000]


def test_min_p():
    lg = float(f32(math.log(0.5)))
    x = np.array([2.0, 2.0 + lg, 1.3, np.nan, -INF, 2.0 + lg - 1e-6], np.float32)
    out = ref(x, Rules(min_p=0.5))[0]
    thr = f32(2.0) + f32(lg)
    assert out[0] == 2.0 and out[1] == x[1] >= thr and out[2] == -INF and np.isnan(out[3]) and out[4] == -INF
    assert out[5] == (-INF if x[5] < thr else x[5])
    assert ref(x, Rules(min_p=1.0))[0].tolist()[:3] == [2.0, -INF, -INF]
    with_inf = np.array([1.0, INF, -5.0], np.float32)
    assert bits(ref(with_inf, Rules(min_p=0.5))[0]) == bits(with_inf)                     # a +inf maximum: skipped
    all_nan = np.full(4, np.nan, np.float32)
    assert bits(ref(all_nan, Rules(min_p=0.5))[0]) == bits(all_nan)                       # every logit NaN: skipped
    none_left = np.array([-INF, np.nan], np.float32)
    assert bits(ref(none_left, Rules(min_p=0.5))[0]) == bits(none_left)
    # it acts after the bias: the ban moves the maximum
    out = ref([5.0, 1.0, 0.75], Rules(min_p=0.5, logit_bias={0: -INF}))[0]
    assert out.tolist() == [-INF, 1.0, 0.75]
    # a positive min_p_log (device bits no host wrote) is inactive
    raw = struct.pack("<ffffIIII8I", 1.0, 0.0, 0.0, 0.5, 0, 0, 0, 0, *([0] * 8))
    assert ref([5.0, 1.0], raw=raw)[0].tolist() == [5.0, 1.0]


def test_sanitising_and_ids_past_n():
    x = [2.0, -2.0, 1.0]
    seq = np.array([0, 1, 7, -1, 0], np.int32)              # 7 and 0xFFFFFFFF are >= n: ignored
    for rep in (float("nan"), -2.0, 0.0, INF):
        raw = struct.pack("<ffffIIII8I", rep, float("nan"), INF, -INF, 5000, 10000, 99, 0, *([0] * 8))
        out, seq_after, _, st = ref(x, raw=raw, seq=seq, pos=4, tok=0)
        assert out.tolist() == x and st == 0 and seq_after.tolist() == [0, 1, 7, 0xFFFFFFFF, 0]
    raw = struct.pack("<ffffIIII8I", 2.0, 1.0, 0.0, -INF, 5000, 0, 0, 0, *([0] * 8))
    out = ref(x, raw=raw, seq=seq, pos=4, tok=0)[0]
    assert out.tolist() == [0.0, -5.0, 1.0]                 # last_n clamps to 1024 >= pos + 1; ids >= n take no part
    # n_stop clamps to 8: a ninth id (it lies behind the struct's end anyway) never stops
    raw = struct.pack("<ffffIIII8I", 1.0, 0.0, 0.0, -INF, 0, 0, 99, 0, 1, 2, 3, 4, 5, 6, 7, 8)
    assert ref(x, raw=raw, seq=seq, pos=1, tok=8, stop_pos=NO_STOP)[2] == 1
    assert ref(x, raw=raw, seq=seq, pos=1, tok=9, stop_pos=NO_STOP)[2] == NO_STOP


def test_past_the_end_nothing_is_written():
    x = [1.0, 1.0]
    seq = np.array([0, 0, 0], np.int32)
    r = Rules(repetition_penalty=2.0, stop_ids=(1,))
    for pos in (3, 4, 0xFFFFFFFF):
        out, seq_after, stop, st = ref(x, r, seq, pos, 1, stop_pos=NO_STOP)
        assert out.tolist() == x and seq_after.tolist() == [0, 0, 0] and st == 1
        assert stop == pos                                   # the stop rule does not look at seqLen
    out, seq_after, stop, st = ref(x, r, seq, 2, 1, stop_pos=NO_STOP)
    assert out.tolist() == [0.5, 0.5] and seq_after.tolist() == [0, 0, 1] and st == 0 and stop == 2


def test_stop_is_recorded_once_and_never_in_the_prompt():
    x = [0.0] * 4
    seq = np.zeros(8, np.int32)
    r = Rules(stop_ids=(3, 2))
    assert ref(x, r, seq, 4, 3, stop_pos=NO_STOP, first_pos=5)[2] == NO_STOP              # below first_pos
    assert ref(x, r, seq, 5, 3, stop_pos=NO_STOP, first_pos=5)[2] == 5
    assert ref(x, r, seq, 6, 2, stop_pos=5, first_pos=5)[2] == 5                          # only the first stop
    assert ref(x, r, seq, 6, 1, stop_pos=NO_STOP, first_pos=5)[2] == NO_STOP              # not a stop id
    assert ref(x, r, seq, 6, 3, stop_pos=None, first_pos=5)[2] is None                    # no stop reporting
    assert ref(x, r, None, 6, None, stop_pos=NO_STOP, first_pos=5)[2] == NO_STOP          # stop reporting needs tok
    assert ref(x, Rules(), seq, 6, 0, stop_pos=NO_STOP)[2] == NO_STOP                     # n_stop = 0: the zeros behind it are no ids
