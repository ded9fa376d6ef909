"""The calls of a token step with the generation rules on (Decoder.token_step(rules=True)), on a machine without a GPU: the recorded
trace of the same step without them (tests/golden/decode_launches.json, through the recorder of tests/test_decode_trace_cpu.py) with
exactly two differences -- effort_logit_rules is inserted before the last call, and the last call reads ``logits_ruled``."""
import json

import pytest

from .test_decode_trace_cpu import CASES, EFFORT, GOLDEN, Recorder, make_model


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def ruled_trace(monkeypatch, case, rules=True):
    from effort_amd.decode import Decoder
    layout, experts, ctor, step, comm, rocblas, _ = CASES[case]
    rec = Recorder(**comm).install(monkeypatch)
    rec.gpu.dense_rocblas = rocblas
    dec = Decoder(make_model(layout, experts), maxTokens=8, **ctor)
    assert not any(hasattr(dec, a) for a in ("seq", "logits_ruled", "rules_params", "bias_ids", "bias_vals", "stop_pos"))    # made on first use
    dec._rules_buffers()
    rec.watch(dec)
    dec.token_step(EFFORT, rules=rules, **step)
    first, rec.records = rec.records, []
    dec.token_step(EFFORT, rules=True, **step)
    assert rec.records == first, "the second ruled step of a Decoder makes the calls of its first"
    return json.loads(json.dumps(first)), dec


RULES_CALL = ["effort_logit_rules", "ctx", "logits", 32, "rules_params", "tokId", "pos", "seq", 8, "bias_ids", "bias_vals", "stop_pos", "logits_ruled"]


@pytest.mark.parametrize("case", ["fp16-default", "fp16-sampled", "q4ref-default", "mixtral-folded", "fp16-emulated-world2", "fp16-dense"])
def test_ruled_step_is_the_recorded_step_plus_one_call(monkeypatch, golden, case):
    got, _ = ruled_trace(monkeypatch, case)
    want = golden[case]
    assert len(got) == len(want) + 1
    assert got[:-2] == want[:-1]
    assert got[-2] == RULES_CALL
    last = list(want[-1])
    assert last[0] == ("effort_sample" if case == "fp16-sampled" else "effort_argmax") and last[2] == "logits"
    last[2] = "logits_ruled"
    assert got[-1] == last


def test_a_rules_object_writes_its_settings_and_makes_the_same_calls(monkeypatch, golden):
    from effort_amd.rules import Rules
    r = Rules(repetition_penalty=1.2, logit_bias={3: -1.0}, stop_ids=(5,))
    got, dec = ruled_trace(monkeypatch, "fp16-default", rules=r)
    assert got[-2] == RULES_CALL and len(got) == len(golden["fp16-default"]) + 1
    assert bytes(dec.rules_params.numpy().tobytes()) == r.pack(0)
    assert dec.bias_ids[0].item() == 3 and dec.bias_vals[0].item() == -1.0 and dec.stop_pos.item() == -1


def test_a_step_without_rules_makes_no_buffers(monkeypatch, golden):
    from effort_amd.decode import Decoder
    rec = Recorder().install(monkeypatch)
    dec = Decoder(make_model(), maxTokens=8)
    rec.watch(dec)
    dec.token_step(EFFORT, rules=None)
    dec.token_step(EFFORT, rules=False)
    assert json.loads(json.dumps(rec.records)) == golden["fp16-default"] * 2
    assert not hasattr(dec, "seq") and not hasattr(dec, "logits_ruled")
    dec.reset()                                              # (nothing of the rules to clear)
