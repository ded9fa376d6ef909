"""The calls a token step makes (effort_amd/decode.py: Decoder.token_step), on a machine without a GPU.

A ``Decoder`` is built on CPU tensors over stand-in bundles, and every boundary it calls through is replaced by a recorder: the C
ABI (``_lib.lib().effort_*``), the device context (``_gpu``: its ``allgather_outputs`` is the sharded loop's gather), ``basicMul``,
``basicMulExpert``, ``bucketMul``, ``bucketMulQ4`` and ``bucketMulGroup`` (in ``effort_amd.bucket_mul`` too, where
``ColumnShardedGroups._launch`` imports it).  No multiply runs.  One token step then leaves a list of records: the entry point and
its operands BY NAME -- a Decoder attribute (``kCache[1]``), a model tensor (``L0.attnNorm``, ``L1.w2.core``), a bundle (``L0.wq``, its
column shard ``L0.wq[1/2]``), and ``[base, offset, length]`` for a view, found through the storage pointer and the storage offset.

tests/golden/decode_launches.json holds these lists for every configuration below.  It was recorded by this recorder from the five
hand-written loops the step consisted of, before they became one layer walk, with COMM edit by hand: the second ``effort_fetch_row``
of a step on a model with Q4 / core-only bundles is removed.  It is never regenerated from later code: the captured graphs are these
sequences, so a difference here is a different graph.
"""
import ctypes as C
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "decode_launches.json")
EFFORT = 0.25
BUNDLES = ("wq", "wk", "wv", "wo", "w1", "w2", "w3")


# ---------------------------------------------------------------- stand-ins for the model
class Bundle:
    """What decode.py and ColumnShardedGroups read of an ExpertWeights."""

    def __init__(self, name, outSize, inSize, q4=False, bucketsLoaded=True, core=None):
        self.name, self.outSize, self.inSize, self.q4, self.bucketsLoaded, self.core = name, outSize, inSize, q4, bucketsLoaded, core

    def column_shard(self, r, world):
        return Bundle(f"{self.name}[{r}/{world}]", self.outSize // world, self.inSize, self.q4, self.bucketsLoaded)


# kinds: "f" FP16 bucketed, "q" Q4 bucketed, "c" core-only -- in the order of BUNDLES
LAYOUTS = {
    "fp16": "fffffff",
    "q4ref": "qcccqqq",           # the reference's Q4 model: wq, w1, w2, w3 in Q4; wk, wv, wo their cores alone
    "q4all": "qqqqqqq",
    "f16ref": "fcccfff",          # the same split with FP16 buckets
    "kinds": "qfqfqff",           # both kinds among the bundles that share an input
}


def make_model(layout="fp16", experts=1):
    from effort_amd.decode import Layer, MistralConfig, Model
    cfg = MistralConfig(stateDim=64, hiddenDim=128, numLayers=2, numHeads=4, numHeadsKV=2, headDim=16, vocab=32, numExperts=experts)
    m = Model(cfg)
    half = lambda *shape: torch.zeros(shape, dtype=torch.float16)               # noqa: E731
    kv = cfg.numHeadsKV * cfg.headDim
    shapes = {"wq": (cfg.stateDim, cfg.stateDim), "wk": (kv, cfg.stateDim), "wv": (kv, cfg.stateDim), "wo": (cfg.stateDim, cfg.stateDim),
              "w1": (cfg.hiddenDim, cfg.stateDim), "w2": (cfg.stateDim, cfg.hiddenDim), "w3": (cfg.hiddenDim, cfg.stateDim)}
    for n in range(cfg.numLayers):
        L = Layer()
        L.attnNorm, L.ffnNorm = half(cfg.stateDim), half(cfg.stateDim)
        L.ffnGate = half(experts, cfg.stateDim) if experts > 1 else None
        for w, kind in zip(BUNDLES, LAYOUTS[layout]):
            o, i = shapes[w]
            core = half(experts, o, i) if experts > 1 and w in ("w1", "w2", "w3") else half(o, i)
            setattr(L, w, Bundle(f"L{n}.{w}", o, i, q4=kind in "qc", bucketsLoaded=kind != "c", core=core))
        m.layers.append(L)
    m.norm, m.output, m.tokEmbeddings = half(cfg.stateDim), half(cfg.vocab, cfg.stateDim), half(cfg.vocab, cfg.stateDim)
    return m


# ---------------------------------------------------------------- the recorder
class EffortError(RuntimeError):
    def __init__(self, code=0):
        super().__init__(code)
        self.code = code


class Recorder:
    def __init__(self, has_comm=False, comm_world=1, comm_rank=0):
        self.records, self.bases, self.dec = [], {}, None       # bases: storage pointer -> (name, elements, bytes, tensor)
        rec = self

        class Gpu:                                               # the device context: effort_amd.runtime.gpu(index)
            ctx = "ctx"
            dense_rocblas = False

            def __init__(self):
                self.has_comm, self.comm_world, self.comm_rank = has_comm, comm_world, comm_rank

            def _bind_stream(self):
                pass

            def check(self, rc, what):
                assert rc == 0, what

            def allgather_outputs(self, send, recv, count):
                rec.records.append(["allgather_outputs", rec.name(send), rec.name(recv), int(count)])

        class Lib:                                               # effort_amd._lib.lib()
            def __getattr__(self, fn):
                def call(*args):
                    rec.records.append([fn] + [rec.name(a) for a in args])
                    return 0
                return call

        class LibModule:                                         # effort_amd._lib
            EffortError = globals()["EffortError"]
            lib = staticmethod(lambda lib=Lib(): lib)

        self.gpu, self.lib_module = Gpu(), LibModule

    def install(self, monkeypatch):
        import effort_amd.bucket_mul
        import effort_amd.decode as d
        monkeypatch.setattr(d, "_gpu", lambda index=None: self.gpu)
        monkeypatch.setattr(d, "_lib", self.lib_module)
        for fn, params in (("basicMul", "v by out"), ("basicMulExpert", "v cores expNo out"), ("bucketMul", "v by expNo out effort"),
                           ("bucketMulQ4", "v by expNo out effort")):
            monkeypatch.setattr(d, fn, self.multiply(fn, len(params.split())))
        monkeypatch.setattr(d, "bucketMulGroup", self.group)
        monkeypatch.setattr(effort_amd.bucket_mul, "bucketMulGroup", self.group)
        return self

    def multiply(self, fn, nargs):
        def call(*args):
            assert len(args) == nargs, (fn, len(args))
            self.records.append([fn] + [self.name(a) for a in args])
        return call

    def group(self, calls, gpu=None):
        """Every call is written with six elements, the sixth null where it folds nothing: a call of five, one with None and one with
        an empty dict are the same call to bucketMulGroup (bucket_mul._marshal), and which entry point a group takes depends on
        whether ANY of its calls folds something."""
        r = ["bucketMulGroup", [[self.name(a) for a in call[:5]] + [self.name((call[5] if len(call) > 5 else None) or None)] for call in calls]]
        if gpu is not None:
            r.append({"gpu": self.name(gpu.ctx)})
        self.records.append(r)

    # -- operands by name
    def add(self, name, t):
        st = t.untyped_storage()
        self.bases[st.data_ptr()] = (name, t.numel(), st.nbytes(), t)             # (the tensor is held: its address stays its own)

    def watch(self, dec):
        """Name the model's tensors and every tensor the Decoder holds."""
        self.dec, m = dec, dec.model
        for n, L in enumerate(m.layers):
            for a in ("attnNorm", "ffnNorm", "ffnGate"):
                if getattr(L, a) is not None:
                    self.add(f"L{n}.{a}", getattr(L, a))
            for w in BUNDLES:
                self.add(f"L{n}.{w}.core", getattr(L, w).core)
        for a in ("norm", "output", "tokEmbeddings"):
            self.add(a, getattr(m, a))
        for a, v in vars(dec).items():
            if torch.is_tensor(v):
                self.add(a, v)
            elif isinstance(v, list) and v and all(torch.is_tensor(t) for t in v):
                for n, t in enumerate(v):
                    self.add(f"{a}[{n}]", t)

    def staging(self):
        """The send / receive buffers ColumnShardedGroups makes on first use, named by the local output sizes of their group."""
        for (_, los), (send, recv) in self.dec.groups._bufs.items():
            tag = "+".join(str(lo) for lo in los)
            self.add(f"send<{tag}>", send)
            self.add(f"recv<{tag}>", recv)

    def name(self, a):
        if a is None or isinstance(a, (bool, int, float, str)):
            return a
        if isinstance(a, C.c_float):
            return float(a.value)
        if isinstance(a, Bundle):
            return a.name
        if isinstance(a, dict):
            return {k: self.name(v) for k, v in a.items()}
        if isinstance(a, C.c_void_p):                            # a whole buffer, or [base, offset in bytes]
            for base, (nm, _, nbytes, _) in self.bases.items():
                if base <= a.value < base + nbytes:
                    return nm if a.value == base else [nm, a.value - base]
            raise AssertionError("a pointer into no known buffer")
        assert torch.is_tensor(a) and a.is_contiguous(), type(a)
        key = a.untyped_storage().data_ptr()
        if key not in self.bases and self.dec is not None and self.dec.groups is not None:
            self.staging()
        if key not in self.bases:                                # (the gathered cores of the dense Mixtral fallback: index_select's result)
            return {"temporary": list(a.shape)}
        nm, numel = self.bases[key][:2]
        return nm if a.storage_offset() == 0 and a.numel() == numel else [nm, a.storage_offset(), a.numel()]


# ---------------------------------------------------------------- the cases
# name: (layout, experts, Decoder arguments, token_step arguments, communicator of the context, rocBLAS dense backend, records per step)
COMM, NO_COMM = dict(has_comm=True, comm_world=1), dict(has_comm=False)      # (a communicator of one rank; none)
CASES = {
    "fp16-default":                ("fp16", 1, {}, {}, NO_COMM, False, 14),
    "fp16-unfolded":               ("fp16", 1, dict(fused_glue=False), {}, NO_COMM, False, 20),
    "fp16-unfolded-two-attention": ("fp16", 1, dict(fused_glue=False, fused_attention=False), {}, NO_COMM, False, 22),
    "fp16-norm":                   ("fp16", 1, dict(fused_glue=("norm",)), {}, NO_COMM, False, 19),
    "fp16-gate":                   ("fp16", 1, dict(fused_glue=("gate",)), {}, NO_COMM, False, 18),
    "fp16-norm-resid":             ("fp16", 1, dict(fused_glue=("norm", "resid")), {}, NO_COMM, False, 16),
    "fp16-resid":                  ("fp16", 1, dict(fused_glue=("resid",)), {}, NO_COMM, False, None),
    "fp16-gate-resid":             ("fp16", 1, dict(fused_glue=("gate", "resid")), {}, NO_COMM, False, None),
    "fp16-default-two-attention":  ("fp16", 1, dict(fused_attention=False), {}, NO_COMM, False, 14),
    "fp16-sharded-world1":         ("fp16", 1, dict(sharded=True, world=1), {}, COMM, False, 22),
    "fp16-emulated-world2":        ("fp16", 1, dict(world=2, emulate_world=True), {}, NO_COMM, False, 22),
    "fp16-dense":                  ("fp16", 1, {}, dict(dense=True), NO_COMM, False, 26),
    "fp16-dense-two-attention":    ("fp16", 1, dict(fused_attention=False), dict(dense=True), NO_COMM, False, 28),
    "fp16-sampled":                ("fp16", 1, {}, dict(sampling=True), NO_COMM, False, 14),
    "fp16-folded":                 ("fp16", 1, dict(fused_glue=True), {}, NO_COMM, False, 14),
    "q4ref-default":               ("q4ref", 1, {}, {}, NO_COMM, False, 24),
    "q4ref-folded":                ("q4ref", 1, dict(fused_glue=True), {}, NO_COMM, False, 22),
    "q4ref-gate":                  ("q4ref", 1, dict(fused_glue=("gate",)), {}, NO_COMM, False, None),
    "q4ref-dense":                 ("q4ref", 1, {}, dict(dense=True), NO_COMM, False, 26),
    "q4ref-default-two-attention": ("q4ref", 1, dict(fused_attention=False), {}, NO_COMM, False, 24),
    "q4ref-dense-two-attention":   ("q4ref", 1, dict(fused_attention=False), dict(dense=True), NO_COMM, False, 28),
    "q4all-folded":                ("q4all", 1, dict(fused_glue=True), {}, NO_COMM, False, 14),
    "f16ref-folded":               ("f16ref", 1, dict(fused_glue=True), {}, NO_COMM, False, None),
    "f16ref-default":              ("f16ref", 1, {}, {}, NO_COMM, False, None),
    "kinds-folded":                ("kinds", 1, dict(fused_glue=True), {}, NO_COMM, False, None),
    "kinds-default":               ("kinds", 1, {}, {}, NO_COMM, False, None),
    "mixtral-default":             ("fp16", 4, {}, {}, NO_COMM, False, 28),
    "mixtral-folded":              ("fp16", 4, dict(fused_glue=True), {}, NO_COMM, False, 18),
    "mixtral-dense":               ("fp16", 4, {}, dict(dense=True), NO_COMM, False, 40),
    "mixtral-dense-rocblas":       ("fp16", 4, {}, dict(dense=True), NO_COMM, True, None),
}


def trace(monkeypatch, case):
    from effort_amd.decode import Decoder
    layout, experts, ctor, step, comm, rocblas, _ = CASES[case]
    rec = Recorder(**comm).install(monkeypatch)
    rec.gpu.dense_rocblas = rocblas
    dec = Decoder(make_model(layout, experts), maxTokens=8, **ctor)
    rec.watch(dec)
    dec.token_step(EFFORT, **step)
    first, rec.records = rec.records, []
    dec.token_step(EFFORT, **step)
    assert rec.records == first, "the second step of a Decoder makes the calls of its first"
    return json.loads(json.dumps(first)), dec


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_table_holds_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)
    for case, want in golden.items():
        n = CASES[case][6]
        assert n is None or len(want) == n, case


@pytest.mark.parametrize("case", sorted(CASES))
def test_token_step_makes_the_recorded_calls(monkeypatch, golden, case):
    got, dec = trace(monkeypatch, case)
    want = golden[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"{case}: record {i} of {len(want)}"
    assert len(got) == len(want), f"{case}: {[r[0] for r in got]} against {[r[0] for r in want]}"
    if case.startswith("mixtral-dense"):
        assert dec.dense_expert_gemv is (case == "mixtral-dense")
    assert got[-1][0] == ("effort_sample" if case == "fp16-sampled" else "effort_argmax")


def test_traces_that_are_one_trace(golden):
    """fused_attention=False reaches the unfolded FP16 loop alone; a model of seven bucketed bundles makes the calls of the FP16 default
    whichever kind they are (every call carries extras, so every launch is a group launch)."""
    assert golden["fp16-default-two-attention"] == golden["fp16-default"] == golden["fp16-folded"]
    assert golden["q4all-folded"] == golden["fp16-default"]
    assert golden["fp16-sampled"][:-1] == golden["fp16-default"][:-1]
    names = lambda case: [r[0] for r in golden[case]]                           # noqa: E731
    assert "effort_rope_kv" in names("fp16-unfolded-two-attention") and "effort_rope_kv" not in names("fp16-default-two-attention")
    for case in golden:
        assert names(case).count("effort_fetch_row") == 1, case


# ---------------------------------------------------------------- the constructor's refusals
def refuse(monkeypatch, error, match, layout="fp16", experts=1, comm=NO_COMM, **ctor):
    from effort_amd.decode import Decoder
    Recorder(**comm).install(monkeypatch)
    with pytest.raises(error, match=match):
        Decoder(make_model(layout, experts), maxTokens=8, **ctor)


def test_refusals(monkeypatch):
    fp16_only = "column-sharded decode .* is implemented for FP16 models"
    folded = "needs the glue folded into the multiplies"
    refuse(monkeypatch, ValueError, fp16_only, layout="q4ref", sharded=True)
    refuse(monkeypatch, ValueError, fp16_only, layout="q4ref", world=2, emulate_world=True)
    refuse(monkeypatch, ValueError, fp16_only, layout="q4ref", world=2)
    refuse(monkeypatch, ValueError, "Q4 decode is Mistral only", layout="q4ref", experts=4)
    refuse(monkeypatch, ValueError, folded, fused_glue=("norm", "resid"), world=2, emulate_world=True)
    refuse(monkeypatch, ValueError, folded, fused_glue=False, sharded=True, comm=COMM)
    refuse(monkeypatch, ValueError, folded, experts=4, world=2, emulate_world=True)
    refuse(monkeypatch, ValueError, folded, experts=4, fused_glue=True, sharded=True, comm=COMM)
    refuse(monkeypatch, RuntimeError, "give the device's context its communicator first", sharded=True)
    refuse(monkeypatch, ValueError, "world / rank differ from the context's communicator", sharded=True, world=2, rank=1, comm=COMM)
