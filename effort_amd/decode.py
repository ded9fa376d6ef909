"""The decode loop around bucketMul -- host mirror of ``runNetwork`` (runNetwork.swift:68-316) for Mistral-7B-shaped
models (the caller of the hot path).

One token step = per layer: rmsNorm * attnNorm -> wq | wk | wv (ONE grouped bucketMul launch: three independent calls on
the same input) -> rope + 4x kv repeat + cache -> scores / softmax / weighted sum -> wo -> residual + rmsNorm * ffnNorm
-> w1 | w3 (one grouped launch) -> silu -> w2 -> residual; then the output norm, the dense LM head (``basicMul``,
runNetwork.swift:222) and a greedy or sampled pick.  ``Decoder.token_step`` is that walk, written once for FP16, Q4, Mixtral
and column-sharded models; its docstring says who multiplies, which glue folds into the multiplies and how many launches a
layer makes under which settings, and ``Decoder``'s where ``fused_attention`` applies.  The glue runs in the HIP kernels of
effort_amd/csrc/decode.hip through the C ABI; the token position and the current token id live in device memory, so a whole
step is captured once into a hipGraph and replayed per token -- no host work, no per-kernel launch gaps (the reference
spends ~15 ms/token in such gaps, runNetwork.swift:91-103).  torch is used for buffers and graph capture only.

``dense=True`` routes every projection through ``basicMul`` (rocBLAS GEMV on the f16 cores): the baseline the
reference compares against (``effort`` 100 % vs dense, KL divergence of the logits).

``Decoder.prefill`` / ``run(..., prefill=True)`` ingest a prompt in blocks of up to 64 tokens that share one pass over every
matrix (the MFMA block multiply, effort_amd/csrc/prefill.hip; the block forms of the glue, effort_amd/csrc/decode.hip), eagerly, beside the token step:
the step, its graphs and the cache layout are the same with or without it.
"""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass

import torch

from . import _lib
from .bucket_mul import basicMul, basicMulExpert, bucketMul, bucketMulGroup, bucketMulQ4
from .rules import Rules
from .runtime import gpu as _gpu
from .sampling import Sampling
from .weights import ExpertWeights


@dataclass
class MistralConfig:                      # main.swift:45-77
    stateDim: int = 4096
    hiddenDim: int = 14336
    numLayers: int = 32
    numHeads: int = 32
    numHeadsKV: int = 8
    headDim: int = 128
    vocab: int = 32000
    ropeBase: float = 1e6                 # createFreqsCis2: logspace base 1e-6 (model.swift:700)
    numExperts: int = 1                   # > 1: Mixtral -- a dense gate picks 2 experts per token and layer (runNetwork.swift:185-199)


class Layer:                              # loader.swift Layer: norms + seven ExpertWeights
    __slots__ = ("attnNorm", "ffnNorm", "wq", "wk", "wv", "wo", "w1", "w2", "w3", "ffnGate")


class Model:
    def __init__(self, cfg: MistralConfig):
        self.cfg = cfg
        self.layers: list[Layer] = []
        self.norm = None                  # f16 [stateDim]
        self.output = None                # f16 [vocab, stateDim]  (output.core)
        self.tokEmbeddings = None         # f16 [vocab, stateDim]  (tok_embeddings.core)

    @classmethod
    def random(cls, cfg: MistralConfig, seed: int = 0, device="cuda", scale: float = 0.02, keep_cores: bool = True,
               structured: bool = False, q4: bool = False, q4_perc: float = 0.02) -> "Model":
        """Random-init weights of the architecture (no checkpoints here), converted by the GPU bucketizer.
        ``structured``: the statistics trained transformers show and i.i.d. Gaussians lack -- heavy-tailed weights with
        per-input-channel and per-output scale spread, norm weights with a few outlier channels (so the normalised state
        a multiply sees is heavy-tailed), a peaked output distribution -- see ``structured_matrix``.  The reference's quality
        figures (cos-sim 0.99 at 25 % effort, docs/ryc/ryc0.3.png) are for such weights; on Gaussian ones 25 % gives 0.94.
        ``q4``: the reference's Q4 model (q4_convert.py:48-66) from the SAME matrices the FP16 model of this seed has: wq, w1, w2
        and w3 through the GPU Q4 converter (the top ``q4_perc`` of the weights as outliers, 2 % by default), wk, wv and wo as cores
        only -- they ARE their cores.  With ``keep_cores=False`` the four Q4 bundles drop their cores: the model decodes as ever and
        prefills through ``Decoder.prefill(weights="q4")``."""
        if q4 and cfg.numExperts > 1:
            raise ValueError("Model.random(q4=True): Mistral only (one expert) -- wk, wv and wo ARE their cores")
        m = cls(cfg)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed)

        def mat(o, i, s=scale):
            if structured:
                return structured_matrix(o, i, gen, device, s)
            return (torch.randn((o, i), generator=gen, device=device, dtype=torch.float32) * s).to(torch.float16)

        def vec(n):
            if structured:
                return structured_norm_weights(n, gen, device)
            return (1.0 + 0.1 * torch.randn(n, generator=gen, device=device, dtype=torch.float32)).to(torch.float16)

        kv = cfg.numHeadsKV * cfg.headDim

        def bundle(o, i, experts=1, name=""):
            if q4:
                core = mat(o, i)
                if name in ("wq", "w1", "w2", "w3"):
                    return ExpertWeights.from_core_q4(core, q4_perc, keep_core=keep_cores)
                return ExpertWeights.core_only(core, q4=True)
            ews = []
            for _ in range(experts):
                ew = ExpertWeights.from_core(mat(o, i))
                if not keep_cores:
                    ew.core = None
                ews.append(ew)
            if experts == 1:
                ew = ews[0]
            else:                                         # Mixtral: all experts in one buffer, picked by expNo (loader.swift:113-166)
                ew = ExpertWeights.stack(ews)
                ew.core = torch.stack([e.core for e in ews]) if keep_cores else None      # [E, out, in] for the dense path
            ew.handle
            return ew

        for _ in range(cfg.numLayers):
            L = Layer()
            L.attnNorm, L.ffnNorm = vec(cfg.stateDim), vec(cfg.stateDim)
            for name, (o, i) in (("wq", (cfg.stateDim, cfg.stateDim)), ("wk", (kv, cfg.stateDim)), ("wv", (kv, cfg.stateDim)),
                                 ("wo", (cfg.stateDim, cfg.stateDim))):
                setattr(L, name, bundle(o, i, name=name))
            for name, (o, i) in (("w1", (cfg.hiddenDim, cfg.stateDim)), ("w3", (cfg.hiddenDim, cfg.stateDim)), ("w2", (cfg.stateDim, cfg.hiddenDim))):
                setattr(L, name, bundle(o, i, cfg.numExperts, name=name))
            L.ffnGate = mat(cfg.numExperts, cfg.stateDim) * 10 if cfg.numExperts > 1 else None     # f16 [numExperts, stateDim]
            m.layers.append(L)
        m.norm = vec(cfg.stateDim)
        m.output = mat(cfg.vocab, cfg.stateDim, 0.08 if structured else scale)      # structured: logits a few units wide (a peaked next-token distribution)
        m.tokEmbeddings = (torch.randn((cfg.vocab, cfg.stateDim), generator=gen, device=device, dtype=torch.float32)).to(torch.float16)
        return m

    @classmethod
    def load(cls, loader, cfg: MistralConfig, percentLoad: int = 16, device="cuda", q4: bool = False) -> "Model":
        """From a bucketed model on disk (effort_amd.bucketfile, names of convert.swift:70-105).  ``q4``: a model written by
        ``convertMistral(q4=True)`` (q4_convert.py:48-66): Q4 bundles, and core-only bundles where no buckets were stored."""
        from .bucketfile import loadExpertWeights
        if q4 and cfg.numExperts > 1:
            raise ValueError("Model.load(q4=True): the Q4 converter is Mistral only (one expert)")
        m = cls(cfg)
        for n in range(cfg.numLayers):
            L = Layer()
            L.attnNorm = loader[f"layers.{n}.attention_norm"].to(device=device, dtype=torch.float16)
            L.ffnNorm = loader[f"layers.{n}.ffn_norm"].to(device=device, dtype=torch.float16)
            for s in "qkvo":
                setattr(L, "w" + s, loadExpertWeights(loader, f"layers.{n}.attention.w{s}", device=device, q4=q4, dense_ok=q4))
            for w, (o, i) in (("w1", (cfg.hiddenDim, cfg.stateDim)), ("w3", (cfg.hiddenDim, cfg.stateDim)), ("w2", (cfg.stateDim, cfg.hiddenDim))):
                setattr(L, w, loadExpertWeights(loader, f"layers.{n}.feed_forward.experts.", w, inDim=i, outDim=o, numExperts=cfg.numExperts,
                                                percentLoad=None if q4 else percentLoad, device=device, q4=q4))
            gate = f"layers.{n}.feed_forward.gate"
            L.ffnGate = loader[gate].to(device=device, dtype=torch.float16) if cfg.numExperts > 1 and loader.hasTensor(gate) else None
            m.layers.append(L)
        m.norm = loader["model.norm"].to(device=device, dtype=torch.float16)
        m.output = loader["output.core"].to(device=device, dtype=torch.float16)
        m.tokEmbeddings = loader["tok_embeddings.core"].to(device=device, dtype=torch.float16)
        return m


def structured_matrix(o: int, i: int, gen, device, scale: float = 0.02) -> torch.Tensor:
    """Synthetic f16 [o, i] matrix with the structure of trained weights: heavy-tailed entries (a Gaussian times a
    log-normal, sigma 0.5), a log-normal scale per input channel (sigma 0.7) and per output (sigma 0.3); overall std =
    ``scale``.  With a heavy-tailed input this puts single-multiply cos-sim at 25 % effort near 0.99 (bench.py: sweep_structured)."""
    w = torch.randn((o, i), generator=gen, device=device, dtype=torch.float32)
    w *= torch.exp(0.5 * torch.randn((o, i), generator=gen, device=device, dtype=torch.float32))
    w *= torch.exp(0.7 * torch.randn((1, i), generator=gen, device=device, dtype=torch.float32))
    w *= torch.exp(0.3 * torch.randn((o, 1), generator=gen, device=device, dtype=torch.float32))
    w *= scale / w.std()
    return w.to(torch.float16)


def structured_norm_weights(n: int, gen, device) -> torch.Tensor:
    """rmsNorm weights f16 [n]: log-normal spread (sigma 0.6) with 0.5 % outlier channels eight times larger."""
    w = torch.exp(0.6 * torch.randn(n, generator=gen, device=device, dtype=torch.float32))
    big = torch.rand(n, generator=gen, device=device) < 0.005
    w = torch.where(big, w * 8.0, w)
    return (w / w.pow(2).mean().sqrt()).to(torch.float16)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# What ``Decoder(fused_glue=None)`` folds into the launches of a model with Q4 bundles (see Decoder.__init__): nothing -- folding gate +
# residual into the Q4 w2 launch measured 281 against 299 tokens/s.
Q4_FUSED_DEFAULT = ()


class Decoder:
    """State of one sequence (the globals of main.swift:78-140: h, xq, KV caches, scores ...) + the token step.

    ``fused_attention``: True -- rope, the cache write and the attention of a layer are one launch (effort_rope_attention).  False
    -- two (effort_rope_kv + effort_attention), but ONLY in the steps that fold no glue on an FP16 model, and in every ``dense=True``
    step: a step with any of norm / gate / resid folded, a column-sharded step and every effort step of a model with Q4 or core-only
    bundles keep the one launch whatever this says."""

    def __init__(self, model: Model, maxTokens: int = 256, fused_attention: bool = True, fused_glue=None,
                 world: int = 1, rank: int = 0, sharded: bool | None = None, emulate_world: bool = False):
        cfg = self.cfg = model.cfg
        # A model with Q4 or core-only bundles (Model.random(q4=True) / Model.load(q4=True)).  token_step dispatches every multiply per
        # BUNDLE; an all-FP16 model is the case in which every bundle is a bucketed FP16 one.
        self.mixed = any(ew.q4 or not ew.bucketsLoaded for L in model.layers for ew in (L.wq, L.wk, L.wv, L.wo, L.w1, L.w2, L.w3))
        if self.mixed and (cfg.numExperts > 1 or any(L.ffnGate is not None for L in model.layers)):
            raise ValueError("Decoder: Q4 decode is Mistral only (numExperts == 1; the reference's Q4 converter writes no Mixtral model)")
        if self.mixed and (sharded or emulate_world or int(world) > 1):
            raise ValueError("Decoder: column-sharded decode (sharded / emulate_world) is implemented for FP16 models")
        # fused_glue=None: the default -- everything folded for FP16 models (below); for Q4 models what Q4_FUSED_DEFAULT names: NOTHING.
        # Measured at Mistral-7B shapes, 25 % effort, 64 tokens (tools/bench_extra.py --sections decode_q4): 299 tokens/s with the glue
        # kernels against 281 with gate + residual folded into the Q4 w2 launch (effort_bucketmul_q4_group_fused).  Opt in with
        # fused_glue=True or a tuple of parts; the logits are the same within 2e-3 either way (bit-identical on the test model).
        asked = fused_glue is True                        # (a Mixtral model folds only when asked: its default is decided below)
        if fused_glue is None:
            fused_glue = Q4_FUSED_DEFAULT if self.mixed else True
        # (Round 4's `chain=True` -- a layer's dependent multiplies as ONE launch of resident workgroups -- measured 252 against 308
        #  tokens/s and lives on branch `chain-launch`: DESIGN.md 4.5.)
        self.fused_attention = bool(fused_attention)      # rope + cache + attention in one launch per layer (else two: see the class)
        # rmsNorm, silu and the residual adds folded into the multiplies (effort_bucketmul_group_fused): 5 launches per layer
        # instead of 8.  Dense-FFN models only; the dense baseline keeps the separate glue kernels.  On by default since round 3:
        # with every operand of a prologue asked for at the top of the item (they were two more dependent round trips) and the
        # residual asked for before the slabs, all three folded are 306 against 300 tokens/s at 25 % effort (253 against 247 at
        # 50 %); the gate alone or the residuals alone still lose 1 % (tools/lab/decode_ab.py --fused-glue ...).  Bit-identical logits.
        # fused_glue may also name WHICH steps fold into the multiplies: any of "norm" (rmsNorm into wq|wk|wv and w1|w3), "gate"
        # (silu into w2), "resid" (the residual adds after wo and w2); True = all three
        # Mixtral (a layer with an ffnGate) folds ALL OR NOTHING, and only when asked: fused_glue=True makes a layer 7 launches instead of
        # 12 -- wq|wk|wv with the norm prologue, rope_attention, wo with the residual, effort_moe_route (norm + gate GEMV + top-2 in one
        # launch), both experts' w1|w3 with the norm prologue, both w2 with the gate prologue, effort_mix2_add (mix + residual).  None,
        # False or a tuple of parts keep the separate glue kernels there: the default, until tools/bench_extra.py --sections decode_mixtral
        # (which times both in one process) has a recorded run -- there is none yet, the folded loop's speed is UNMEASURED.
        parts = ("norm", "gate", "resid") if fused_glue is True else tuple(fused_glue or ())
        self.moe = any(L.ffnGate is not None for L in model.layers)
        if self.moe:
            self.fuse = frozenset(parts) if asked and all(L.ffnGate is not None for L in model.layers) else frozenset()
        else:
            self.fuse = frozenset(parts)
        self.fused_glue = bool(self.fuse)
        # Where fused_attention=False applies, by token_step's ``dense``: every dense step; an effort step of an FP16 model that folds nothing.
        self._two_launch_attention = {True: not self.fused_attention, False: not (self.fused_attention or self.mixed or self.fused_glue)}
        self.model, self.maxTokens = model, int(maxTokens)
        dev = model.norm.device
        self.g = _gpu(dev.index)
        # Column-sharded decode (BASELINE config 4: "all 32 layers' Wq/Wk/Wv/Wo + FFN matrices sharded across 8 x MI355X, RCCL
        # all-gather"; the reference is single-device, runNetwork.swift:121-183 is what this wraps): every bundle becomes this rank's
        # column shard, every launch group is followed by ONE effort_allgather_outputs (in place on h for wo / w2), the state vectors
        # stay replicated, and the glue (attention, the LM head) runs replicated on every rank.  ``sharded=True`` with world 1 runs
        # the same path through a communicator of one rank; ``emulate_world`` computes every rank's launches in THIS process (no
        # collective): how the split is validated, and its launches timed, on one GPU.
        self.world, self.rank = int(world), int(rank)
        self.sharded = bool(sharded) if sharded is not None else (self.world > 1)
        self.groups = None
        if self.sharded or emulate_world:
            if self.moe or self.fuse != {"norm", "gate", "resid"}:
                raise ValueError("the column-sharded decode loop needs the glue folded into the multiplies (fused_glue=True, dense FFN)")
            if not emulate_world and not self.g.has_comm:
                raise RuntimeError("Decoder(sharded=True): give the device's context its communicator first (effort_amd.sharded.init_comm / Gpu.comm_create)")
            if not emulate_world and (self.g.comm_world != self.world or self.g.comm_rank != self.rank):
                raise ValueError("Decoder: world / rank differ from the context's communicator")
            from .sharded import ColumnShardedGroups
            self.sharded = True
            self.groups = ColumnShardedGroups(self.world, self.rank, emulate=emulate_world, gpu=self.g)
        f = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)      # noqa: E731
        q, kv = cfg.numHeads * cfg.headDim, cfg.numHeadsKV * cfg.headDim
        self.h, self.h_norm, self.fxn, self.outNormed = f(cfg.stateDim), f(cfg.stateDim), f(cfg.stateDim), f(cfg.stateDim)
        self.xq_temp, self.xk_temp, self.xv_temp, self.xq = f(q), f(kv), f(kv), f(q)
        self.attnOutput, self.attnFfnOut, self.ffnOut = f(q), f(cfg.stateDim), f(cfg.stateDim)
        self.x1, self.x3, self.x2 = f(cfg.hiddenDim), f(cfg.hiddenDim), f(cfg.hiddenDim)
        if cfg.numExperts > 1:                                                      # second routed expert + the gate (runNetwork.swift:185-199)
            self.x1b, self.x3b, self.x2b, self.ffnOutB = f(cfg.hiddenDim), f(cfg.hiddenDim), f(cfg.hiddenDim), f(cfg.stateDim)
            self.ffnMix = f(cfg.stateDim)
            self.gateOut, self.gateVals = f(cfg.numExperts), f(2)
            self.gateIdxs = torch.zeros(2, dtype=torch.int32, device=dev)
        self.logits = f(cfg.vocab)
        self.kCache = [f(self.maxTokens, cfg.numHeads, cfg.headDim) for _ in range(cfg.numLayers)]     # xkLayerTokenHead
        self.vCache = [f(self.maxTokens, cfg.numHeads, cfg.headDim) for _ in range(cfg.numLayers)]     # xvLayerToken
        self.pos = torch.zeros(1, dtype=torch.int32, device=dev)
        self.tokId = torch.zeros(1, dtype=torch.int32, device=dev)
        self.history = torch.zeros(self.maxTokens, dtype=torch.int32, device=dev)
        self.sample_params = Sampling().to_device(device=dev)     # effort_sample_params, 32 bytes: the sampled pick reads its settings HERE
        self._graphs: dict = {}
        self.dense_expert_gemv = None                     # Mixtral dense baseline: whether its last step went through effort_dense_gemv_expert (else: gathered cores)
        self._pf = None                                   # prefill's block buffers: made by the first ``prefill`` (see ``_prefill_buffers``)
        self.last_prefill_s = None                        # run(prefill=True): synchronised wall time of its prefill
        self._rules = False                               # the generation rules' buffers: made by the first ruled step (see ``_rules_buffers``)
        self.stopped_at = None                            # run(rules=...): the step that picked a stop token, or None

    # -- one token: everything between fetching the embedding and picking the next token ----------------------------
    def token_step(self, effort: float = 0.25, dense: bool = False, sampling=None, rules=None):
        """ONE walk serves every model and every setting: the embedding fetch; per layer an attention half (norm -> wq | wk | wv ->
        rope + cache + attention -> wo -> residual) and an FFN half (norm -> w1 | w3 -> silu -> w2 -> residual, or with an ffnGate the
        routed form: gate + top-2 -> both experts' w1 | w3 as one group of four -> both w2 as one group of two -> mix); then the closing
        norm, the LM head and ``_pick``.  What differs between settings is decided per call:

        WHO MULTIPLIES (``muls``: an input vector and the [(bundle, out, extras)] that share it).  ``dense``: ``basicMul`` on every
        core.  Column-sharded: ``self.groups.mul`` (this rank's shards in one launch, one gather).  Otherwise per bundle, as expertMul
        does (expertMul.swift:24-38): the bucketed Q4 bundles of the items share one launch and the bucketed FP16 ones another --
        ``bucketMulQ4`` / ``bucketMul`` for a lone call without extras, ``bucketMulGroup`` otherwise --, and a core-only bundle (wk,
        wv, wo of the reference's Q4 model) goes to ``basicMul``.

        WHAT FOLDS into those launches (``self.fuse``; under ``dense`` nothing is bucketed, so nothing folds).  The norm prologue:
        when "norm" is asked for, no residual is pending (a product not yet added to h is added by effort_add_rmsnorm_mul on its way:
        "norm" folds fully only with "resid") and EVERY consumer of the normalised input is bucketed (a dense neighbour reads it from
        memory).  The gate prologue and the residual epilogue: when asked for and the target bundle (w2; wo / w2) is bucketed.  An
        all-FP16 model is the case "every bundle bucketed", the sharded loop the case "everything folded" with another launcher, and
        the reference's Q4 layout folds gate + resid into w2 only.

        Launches per layer: 5 with norm, gate and resid folded (wq|wk|wv, rope_attention, wo, w1|w3, w2), 8 with nothing folded (two
        norms and the silu back); Mixtral 7 folded (wq|wk|wv, rope_attention, wo, effort_moe_route = norm + gate GEMV + top-2, the
        group of four with the same norm as its prologue -- the same bits: both sum in add_rmsnorm_mul_kernel's order --, the group
        of two, effort_mix2_add) and 12 unfolded.  ``fused_attention=False`` adds one where it applies (see ``Decoder``).

        ``sampling``: None -- the step ends in the greedy pick (effort_argmax); a ``Sampling`` -- its settings are written to
        ``self.sample_params`` and the step ends in effort_sample; True -- effort_sample on what ``self.sample_params`` holds (how the
        step is captured: the graph reads the settings from that tensor at every replay).

        ``rules``: None -- the pick reads ``self.logits``; a ``Rules`` -- its settings are written to the device (``set_rules``) and the
        step makes exactly one more call, effort_logit_rules after the LM head: it records the token this step consumed in ``self.seq``,
        reads ``self.logits`` and writes ``self.logits_ruled``, which the pick (untouched) then reads; ``self.logits`` stays raw.  True
        -- the same on what the device tensors hold (the captured form)."""
        cfg, g, lib, m = self.cfg, self.g, _lib.lib(), self.model
        g._bind_stream()
        sampled = sampling is not None and sampling is not False
        if isinstance(sampling, Sampling):
            self.set_sampling(sampling)
        ruled = rules is not None and rules is not False
        if isinstance(rules, Rules):
            self.set_rules(rules)
        elif ruled:
            self._rules_buffers()
        ck = lambda rc, what: g.check(rc, what)                                     # noqa: E731
        fn, fg, fr = (part in self.fuse and not dense for part in ("norm", "gate", "resid"))
        bucketed = lambda *ews: not dense and all(ew.bucketsLoaded for ew in ews)   # noqa: E731
        delta = None                                       # a product not yet added to h: the next effort_add_rmsnorm_mul adds it

        def muls(v, items):                                # items: [(ew, out, extras)]
            if dense:
                for ew, out, _ in items:
                    basicMul(v, ew.core, out)
                return
            if self.sharded:
                return self.groups.mul(v, items, effort)
            for q4 in (True, False):
                calls = [(v, ew, None, out, effort, x) for ew, out, x in items if ew.bucketsLoaded and ew.q4 == q4]
                if len(calls) == 1 and not calls[0][5]:
                    (bucketMulQ4 if q4 else bucketMul)(v, calls[0][1], None, calls[0][3], effort)
                elif calls:
                    bucketMulGroup(calls)
            for ew, out, x in items:
                if not ew.bucketsLoaded:
                    assert not x, "glue folds into bucketed multiplies only"
                    basicMul(v, ew.core, out)

        def rmsnorm(w, out):                               # h += delta; out = rmsNorm(h) * w
            nonlocal delta
            ck(lib.effort_add_rmsnorm_mul(g.ctx, _p(self.h), _p(delta), _p(w), _p(out), cfg.stateDim), "rmsnorm")
            delta = None

        def normed(w, out, *ews):                          # (input, extras) of the multiplies ``ews`` that read rmsNorm(h) * w
            if fn and delta is None and bucketed(*ews):
                return self.h, {"norm": w}
            rmsnorm(w, out)
            return out, None

        def gated(x1, x3, x2, ew):                         # (input, extras) of the multiply that reads silu(x1) * x3
            if fg and bucketed(ew):
                return x1, {"gate": x3}
            ck(lib.effort_silu_mul(g.ctx, _p(x1), _p(x3), _p(x2), cfg.hiddenDim), "silu")
            return x2, {}

        def add_product(ew, v, extras, out):               # h += ew(v): the launch's epilogue, in place on h -- else pending in out
            nonlocal delta
            if fr and bucketed(ew):
                muls(v, [(ew, self.h, dict(extras, resid=self.h))])
            else:
                muls(v, [(ew, out, extras or None)])
                delta = out

        def attention(n):                                  # xq_temp, xk_temp, xv_temp -> attnOutput, the caches at pos written
            kc, vc, rope = _p(self.kCache[n]), _p(self.vCache[n]), C.c_float(cfg.ropeBase)
            if self._two_launch_attention[bool(dense)]:
                ck(lib.effort_rope_kv(g.ctx, _p(self.xq_temp), _p(self.xk_temp), _p(self.xv_temp), _p(self.xq), kc, vc, _p(self.pos),
                                      cfg.numHeads, cfg.numHeadsKV, cfg.headDim, self.maxTokens, rope), "rope_kv")
                ck(lib.effort_attention(g.ctx, _p(self.xq), kc, vc, _p(self.pos), _p(self.attnOutput), cfg.numHeads, cfg.headDim,
                                        self.maxTokens), "attention")
            else:
                ck(lib.effort_rope_attention(g.ctx, _p(self.xq_temp), _p(self.xk_temp), _p(self.xv_temp), kc, vc, _p(self.pos),
                                             _p(self.attnOutput), cfg.numHeads, cfg.numHeadsKV, cfg.headDim, self.maxTokens, rope), "rope_attention")

        def routed_ffn(L, v, x):
            # Mixtral (:185-199): dense gate -> top-2 experts -> softmax of the two; the expert numbers stay on the device (expNo).
            # Folded (all or nothing, see __init__), the routing reads h and ffnNorm itself and the mix lands on h.
            nonlocal delta
            e0, e1 = self.gateIdxs[0:1], self.gateIdxs[1:2]
            if x:
                ck(lib.effort_moe_route(g.ctx, _p(self.h), _p(L.ffnNorm), _p(L.ffnGate), cfg.stateDim, cfg.numExperts, None,
                                        _p(self.gateIdxs), _p(self.gateVals)), "moe_route")                         # :173-175,185-189
            else:
                basicMul(v, L.ffnGate, self.gateOut)
                ck(lib.effort_top2_softmax(g.ctx, _p(self.gateOut), cfg.numExperts, _p(self.gateIdxs), _p(self.gateVals)), "top2")
            if dense:
                self._dense_experts(L, e0, e1)
            else:
                bucketMulGroup([(v, L.w1, e0, self.x1, effort, x), (v, L.w3, e0, self.x3, effort, x),
                                (v, L.w1, e1, self.x1b, effort, x), (v, L.w3, e1, self.x3b, effort, x)])
                (a, xa), (b, xb) = gated(self.x1, self.x3, self.x2, L.w2), gated(self.x1b, self.x3b, self.x2b, L.w2)
                bucketMulGroup([(a, L.w2, e0, self.ffnOut, effort, xa), (b, L.w2, e1, self.ffnOutB, effort, xb)])
            if fr:
                ck(lib.effort_mix2_add(g.ctx, _p(self.h), _p(self.ffnOut), _p(self.ffnOutB), _p(self.gateVals), cfg.stateDim), "mix2_add")   # :190-199
            else:
                ck(lib.effort_mix2(g.ctx, _p(self.ffnOut), _p(self.ffnOutB), _p(self.gateVals), _p(self.ffnMix), cfg.stateDim), "mix2")
                delta = self.ffnMix

        ck(lib.effort_fetch_row(g.ctx, _p(m.tokEmbeddings), _p(self.tokId), _p(self.h), cfg.stateDim), "fetch_row")
        for n, L in enumerate(m.layers):
            v, x = normed(L.attnNorm, self.h_norm, L.wq, L.wk, L.wv)
            muls(v, [(L.wq, self.xq_temp, x), (L.wk, self.xk_temp, x), (L.wv, self.xv_temp, x)])        # runNetwork.swift:121-134
            attention(n)
            add_product(L.wo, self.attnOutput, {}, self.attnFfnOut)                                      # :170-172
            v, x = normed(L.ffnNorm, self.fxn, L.w1, L.w3)
            if L.ffnGate is not None:
                routed_ffn(L, v, x)
            else:
                muls(v, [(L.w1, self.x1, x), (L.w3, self.x3, x)])                                        # :173-179
                add_product(L.w2, *gated(self.x1, self.x3, self.x2, L.w2), self.ffnOut)                  # :181-183
        rmsnorm(m.norm, self.outNormed)
        basicMul(self.outNormed, m.output, self.logits)                                                  # :222 (sharded: replicated, every rank picks the same token)
        if ruled:                                          # (sharded: after the replicated LM head, on every rank alike)
            ck(lib.effort_logit_rules(g.ctx, _p(self.logits), cfg.vocab, _p(self.rules_params), _p(self.tokId), _p(self.pos), _p(self.seq),
                                      int(self.seq.numel()), _p(self.bias_ids), _p(self.bias_vals), _p(self.stop_pos), _p(self.logits_ruled)), "logit_rules")
        self._pick(sampled, self.logits_ruled if ruled else self.logits)

    def _pick(self, sampled: bool, logits=None):
        """The closing call of every token step: the next token from ``logits`` (``self.logits``, or ``self.logits_ruled`` behind the
        generation rules), written to tokId and history[pos]; pos += 1."""
        g, lib, n, hl = self.g, _lib.lib(), self.cfg.vocab, int(self.history.numel())
        logits = self.logits if logits is None else logits
        if not sampled:
            g.check(lib.effort_argmax(g.ctx, _p(logits), n, _p(self.tokId), _p(self.pos), _p(self.history), hl), "argmax")
        else:
            g.check(lib.effort_sample(g.ctx, _p(logits), n, _p(self.sample_params), _p(self.tokId), _p(self.pos), _p(self.history), hl,
                                      None, None), "sample")

    def _rules_buffers(self):
        """What effort_logit_rules reads and writes, made on first use: a Decoder that never asks for rules holds none.  ``seq`` (the
        token every step consumed, int32 [maxTokens]), ``logits_ruled``, ``rules_params`` (effort_rules_params, 64 bytes), the two
        256-entry bias tables and ``stop_pos`` (-1, i.e. 0xFFFFFFFF, while no stop token has been consumed)."""
        if self._rules:
            return
        dev = self.model.norm.device
        self.seq = torch.zeros(self.maxTokens, dtype=torch.int32, device=dev)
        self.logits_ruled = torch.zeros(self.cfg.vocab, dtype=torch.float32, device=dev)
        self.rules_params, self.bias_ids, self.bias_vals = Rules().to_device(device=dev)
        self.stop_pos = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self._rules = True

    def set_rules(self, rules: "Rules", first_pos: int = 0):
        """Rewrite the device-resident settings of the generation rules and forget an earlier stop (no graph is touched: the captured step
        reads these tensors).  ``first_pos``: positions below it never stop -- the prompt's."""
        self.g._bind_stream()
        self._rules_buffers()
        rules.to_device(first_pos, self.rules_params, self.bias_ids, self.bias_vals)
        self.stop_pos.fill_(-1)

    def set_sampling(self, sampling: "Sampling"):
        """Rewrite the device-resident settings of the sampled pick (no graph is touched: the captured step reads this tensor)."""
        self.g._bind_stream()
        sampling.to_device(self.sample_params)

    def topk(self, k: int = 16):
        """mpsTopK of the current logits (effort_topk): (ids, values) of the k largest, value descending, lowest index first among
        equal values; ids past the number of non-NaN logits are -1 (values -inf).  ids: list of int, values: f32 tensor on the host."""
        g = self.g
        g._bind_stream()
        idx = torch.empty(int(k), dtype=torch.int32, device=self.logits.device)
        val = torch.empty(int(k), dtype=torch.float32, device=self.logits.device)
        g.check(_lib.lib().effort_topk(g.ctx, _p(self.logits), self.cfg.vocab, int(k), _p(idx), _p(val)), "topk")
        g.eval()
        return idx.cpu().tolist(), val.cpu()

    def pick_among(self, limit_ids) -> int:
        """The reference's quiz rule (runNetwork.swift:237-249): the 1-based position in ``limit_ids`` of the first of the top 16
        logits that occurs there, else 99."""
        limit = [int(x) for x in limit_ids]
        for i in self.topk(16)[0]:
            for j, want in enumerate(limit):
                if want == i:
                    return j + 1
        return 99

    def _dense_experts(self, L, e0, e1):
        """Dense baseline of the routed FFN: basicMul on the picked expert of each stack of cores, the expert number read on the device
        (basicMulExpert: nothing is gathered).  Under the rocBLAS dense backend, or for a stack the package's kernel does not serve, the
        picked cores are gathered on the device first (index_select keeps the step graph-capturable: three whole matrices copied per
        expert), then plain basicMul."""
        cfg, g, lib = self.cfg, self.g, _lib.lib()

        def mul(v, cores, e, out):
            if not g.dense_rocblas:
                try:
                    basicMulExpert(v, cores, e, out)
                    self.dense_expert_gemv = True
                    return
                except _lib.EffortError as ex:
                    if ex.code != -2:                      # EFFORT_ERR_SHAPE: the library's own word on what its kernel serves (nothing was enqueued)
                        raise
            self.dense_expert_gemv = False
            basicMul(v, torch.index_select(cores, 0, e)[0], out)
        for e, x1, x3, x2, out in ((e0, self.x1, self.x3, self.x2, self.ffnOut), (e1, self.x1b, self.x3b, self.x2b, self.ffnOutB)):
            mul(self.fxn, L.w1.core, e, x1)
            mul(self.fxn, L.w3.core, e, x3)
            g.check(lib.effort_silu_mul(g.ctx, _p(x1), _p(x3), _p(x2), cfg.hiddenDim), "silu")
            mul(x2, L.w2.core, e, out)

    # -- prompt prefill: a block of tokens per pass over the weights ---------------------------------------------------
    PREFILL_MAX_ROWS = 64                                  # EFFORT_PREFILL_MAX_ROWS

    def _prefill_buffers(self, chunk: int):
        """The block buffers of ``prefill`` ([chunk, stateDim], [chunk, hiddenDim] and the rest), made on first use and again only for a
        larger ``chunk``: a Decoder that never prefills holds none."""
        if self._pf is not None and self._pf >= chunk:
            return
        cfg, dev = self.cfg, self.model.norm.device
        f = lambda n: torch.zeros((chunk, n), dtype=torch.float32, device=dev)      # noqa: E731
        q, kv = cfg.numHeads * cfg.headDim, cfg.numHeadsKV * cfg.headDim
        self.pf_h, self.pf_norm = f(cfg.stateDim), f(cfg.stateDim)
        self.pf_xq_temp, self.pf_xk_temp, self.pf_xv_temp, self.pf_xq = f(q), f(kv), f(kv), f(q)
        self.pf_attnOutput, self.pf_attnFfnOut, self.pf_ffnOut = f(q), f(cfg.stateDim), f(cfg.stateDim)
        self.pf_x1, self.pf_x3, self.pf_x2 = f(cfg.hiddenDim), f(cfg.hiddenDim), f(cfg.hiddenDim)
        self.pf_ids = torch.zeros(chunk, dtype=torch.int32, device=dev)
        if self.moe:
            # ffn="routed": [chunk][2][.] per assignment (token, slot of its top-2); the routing of the LAST block is kept per layer --
            # rows [n][r] of pf_gateIdxs (the expert pair) and pf_gateOut (the gate logits) -- for whoever wants to look at it
            f2 = lambda n: torch.zeros((chunk, 2, n), dtype=torch.float32, device=dev)  # noqa: E731
            self.pf_x1r, self.pf_x3r, self.pf_x2r, self.pf_ffnOutR = f2(cfg.hiddenDim), f2(cfg.hiddenDim), f2(cfg.hiddenDim), f2(cfg.stateDim)
            self.pf_gateVals = torch.zeros((chunk, 2), dtype=torch.float32, device=dev)
            self.pf_gateIdxs = torch.zeros((cfg.numLayers, chunk, 2), dtype=torch.int32, device=dev)
            self.pf_gateOut = torch.zeros((cfg.numLayers, chunk, cfg.numExperts), dtype=torch.float32, device=dev)
        self._pf = chunk

    def _block_multiplies(self, from_buckets: bool, q4: bool = False):
        """The two block multiplies of a ``prefill`` walk, chosen once per call by ``weights``:

        ``mul(x, ew, out, rows)``: out[r] = M * f16(x[r]) for the first ``rows`` rows, ONE pass over the matrix;
        ``mul_routed(x, ew, idx2, out, rows, per_slot)``: out[r][s] = M[idx2[r][s]] * f16(x[r]) -- ``per_slot``: * f16(x[r][s]) --, every
        picked expert's matrix read ONCE for all the tokens that picked it.

        On the cores M is ``ew.core`` (effort_dense_gemm_rows / effort_dense_gemm_rows_routed); a matrix the block kernel refuses
        (EFFORT_ERR_SHAPE: nothing was enqueued) goes to ``basicMul`` row by row, a stack to ``basicMulExpert`` per assignment, as
        ``_dense_experts`` falls back.  On the buckets M is the un-bucketed matrix of ``ew`` (effort_bucket_gemm_rows /
        effort_bucket_gemm_rows_routed): no core is read, and there is no fallback -- every refusal of the library was ruled out by
        ``prefill`` before anything was enqueued, so one is an error.  ``q4`` (``weights="q4"``, dense FFN only) decides per bundle:
        a Q4 bundle multiplies by ``unbucket_q4()`` of its buckets plus its outliers (effort_q4_gemm_rows, expert 0; no core is
        read, no fallback), a core-only bundle goes the way of the cores."""
        g, lib = self.g, _lib.lib()
        if from_buckets:
            def mul(x, ew, out, rows):
                g.check(lib.effort_bucket_gemm_rows(g.ctx, ew.handle, 0, _p(x), _p(out), rows), "bucket_gemm_rows")

            def mul_routed(x, ew, idx2, out, rows, per_slot):
                g.check(lib.effort_bucket_gemm_rows_routed(g.ctx, ew.handle, _p(idx2), _p(x), 1 if per_slot else 0, _p(out), rows), "bucket_gemm_rows_routed")
            return mul, mul_routed

        def mul(x, ew, out, rows):
            core = ew.core
            rc = lib.effort_dense_gemm_rows(g.ctx, _p(core), _p(x), _p(out), int(core.shape[1]), int(core.shape[0]), rows)
            if rc == -2:
                for r in range(rows):
                    basicMul(x[r], core, out[r])
                return
            g.check(rc, "dense_gemm_rows")

        def mul_routed(x, ew, idx2, out, rows, per_slot):
            cores = ew.core
            E, o, i = (int(d) for d in cores.shape)
            rc = lib.effort_dense_gemm_rows_routed(g.ctx, _p(cores), E, _p(idx2), _p(x), 1 if per_slot else 0, _p(out), i, o, rows)
            if rc == -2:
                for r in range(rows):
                    for sl in range(2):
                        basicMulExpert(x[r][sl] if per_slot else x[r], cores, idx2[r][sl:sl + 1], out[r][sl])
                return
            g.check(rc, "dense_gemm_rows_routed")
        if q4:
            core_mul = mul

            def mul(x, ew, out, rows):                     # noqa: F811
                if not ew.bucketsLoaded:
                    return core_mul(x, ew, out, rows)
                g.check(lib.effort_q4_gemm_rows(g.ctx, ew.handle, 0, _p(x), _p(out), rows), "q4_gemm_rows")
            return mul, None
        return mul, mul_routed

    def prefill(self, tokenIds: list[int], pos0: int = 0, chunk: int = 64, attention: str = "rows", ffn: str = "dense",
                weights: str = "cores"):
        """Ingest prompt tokens in bulk: fill ``kCache`` / ``vCache`` rows ``pos0 .. pos0 + T - 1`` of every layer, in blocks of at most
        ``chunk`` (<= 64) tokens that share ONE pass over each matrix, then set ``pos`` to ``pos0 + T``.  No logits, no pick: the next
        ``token_step`` (or graph replay) continues from the caches.  Eager, never captured: ``pos0`` and the block sizes are host values.

        The multiplies are the DENSE ones (``basicMul``'s arithmetic on every bundle's f16 ``core``, effort_dense_gemm_rows): the caches
        hold dense K / V whatever effort the decode then runs at -- against a token-by-token ``dense=True`` ingest they differ by the
        rounding of the f32 sums (another order), against an ingest at an effort by what that effort leaves out.  The glue is the
        token step's, bit for bit per token (the *_rows entry points).  Per block and layer: norm (the pending residual added on its
        way) -> wq, wk, wv -> rope + cache write -> attention over rows 0 .. its own -> wo -> norm -> w1, w3 -> silu -> w2; the last
        layer stops after its cache write, since nothing behind it reaches a cache.

        ``attention``: ``"rows"`` is effort_attention_rows (every query of a block reads its keys and values again; the token step's
        bits); ``"block"`` puts effort_attention_block in its place, same operands -- the block's queries share each K / V tile, f32
        MFMA with an online softmax, within the f32 bar of the same float64 value but not the same bits.  On either path the caches
        do not depend on ``chunk``.

        ``ffn``: ``"dense"``, the default, is the walk above and serves dense-FFN models only.  ``"routed"`` serves a Mixtral model (FP16,
        an ffnGate in every layer, numExperts >= 2, the expert stacks' cores [E, out, in] kept): the second half of a layer becomes
        norm -> effort_moe_route_rows (every token's top-2 and their weights, on the device) -> w1 and w3 as routed block multiplies
        (effort_dense_gemm_rows_routed: the block's tokens grouped by the expert they picked, each picked expert's matrix read once per
        block, out [rows][2][hiddenDim]) -> silu over both slots -> routed w2 -> effort_mix2_add_rows on the block's h; nothing is
        pending afterwards.  Still the dense arithmetic, still chunk-independent bits (a routed product is the block multiply's for
        that token alone).  The last block's routing stays in ``pf_gateIdxs[layer][row]`` / ``pf_gateOut[layer][row]``.

        ``weights``: ``"cores"``, the default, is the walk above on every bundle's f16 core.  ``"buckets"`` multiplies by the bucketed
        weights instead, un-bucketed on the fly (effort_bucket_gemm_rows / effort_bucket_gemm_rows_routed): no core is looked at, so a
        model made with ``keep_cores=False`` -- half the memory -- prefills.  It needs every bundle FP16 with its buckets loaded,
        ``percentLoad`` 16 and un-bucketable (``ExpertWeights.unbucket``: no two entries of a bucket name the same output; asked of the
        library once per handle), and serves ``ffn="dense"`` and ``ffn="routed"`` alike.  The matrix it multiplies is the core with the
        low four mantissa bits of every weight replaced by its position in the bucket: the caches hold the K / V a decode at effort
        1.0 would write (up to the order of the sums and the f16 rounding of the inputs), not the dense path's -- bit for bit those of
        ``weights="cores"`` on a model whose cores are ``unbucket()`` of its buckets.  There is no row-by-row fallback: no core exists
        to fall back to.  ``"q4"`` is the path of a model with Q4 bundles (``Model.random(q4=True, keep_cores=False)``): per bundle, a
        Q4 bundle multiplies by ``unbucket_q4()`` of its buckets -- the sign of every weight times the mean of its bucket row -- plus
        its outliers on the f32 input (effort_q4_gemm_rows), a core-only bundle (wk, wv, wo) by its core.  No core of a Q4 bundle is
        looked at, and the caches hold the K / V a Q4 decode at effort 1.0 would write, not the dense ones: a Q4 weight differs from
        its core by the whole quantisation.  Every Q4 handle is asked once whether it is un-bucketable
        (effort_weights_q4_dense_ok).  Dense FFN only.

        Raises ValueError, before anything is enqueued: a ``weights`` other than ``"cores"`` / ``"buckets"`` / ``"q4"``; under ``"q4"``
        an FP16 bucketed bundle (``"buckets"`` is its path), a core-only bundle without its core, a Q4 bundle that is not
        un-bucketable and ``ffn="routed"``; under ``"buckets"`` a Q4
        or core-only bundle, a bundle truncated below ``percentLoad`` 16 and one that is not un-bucketable; a bundle without its core (FP16 models need ``keep_cores``; Q4 models keep
        them), a Mixtral model under ``ffn="dense"`` and a dense-FFN model under ``ffn="routed"``, a column-sharded decoder,
        ``pos0 + T > maxTokens``, ``chunk`` outside 1 .. 64, an ``attention`` other than ``"rows"`` / ``"block"``, an ``ffn`` other
        than ``"dense"`` / ``"routed"``."""
        cfg, g, lib, m = self.cfg, self.g, _lib.lib(), self.model
        ids, pos0, chunk = [int(t) for t in tokenIds], int(pos0), int(chunk)
        T = len(ids)
        if ffn not in ("dense", "routed"):
            raise ValueError(f"Decoder.prefill: ffn must be 'dense' or 'routed', not {ffn!r}")
        if weights not in ("cores", "buckets", "q4"):
            raise ValueError(f"Decoder.prefill: weights must be 'cores' or 'buckets', not {weights!r} (or 'q4', for a model with Q4 bundles)")
        routed, from_buckets, from_q4 = ffn == "routed", weights == "buckets", weights == "q4"
        if from_q4 and routed:
            raise ValueError("Decoder.prefill: weights='q4' serves ffn='dense' alone (the reference writes no Q4 Mixtral model)")
        if routed and not (cfg.numExperts >= 2 and all(L.ffnGate is not None and L.ffnGate.dtype == torch.float16 for L in m.layers)):
            raise ValueError("Decoder.prefill: ffn='routed' is for Mixtral models (an f16 ffnGate in every layer, numExperts >= 2)")
        if not routed and (self.moe or cfg.numExperts > 1):
            raise ValueError("Decoder.prefill: dense-FFN models only (a Mixtral layer routes per token)")
        if self.sharded:
            raise ValueError("Decoder.prefill: not implemented for the column-sharded decode loop")
        bundles = [getattr(L, w) for L in m.layers for w in ("wq", "wk", "wv", "wo", "w1", "w2", "w3")]
        if from_buckets:
            if any(ew.q4 or not ew.bucketsLoaded for ew in bundles):
                raise ValueError("Decoder.prefill: weights='buckets' needs every bundle FP16 with its buckets loaded (not a Q4 or core-only bundle)")
            if any(ew.percentLoad != 16 for ew in bundles):
                raise ValueError("Decoder.prefill: weights='buckets' needs percentLoad 16 (a truncated bundle does not hold the whole matrix)")
            if routed and any(getattr(L, w).numExperts != cfg.numExperts for L in m.layers for w in ("w1", "w2", "w3")):
                raise ValueError("Decoder.prefill: ffn='routed' needs the expert stacks [numExperts] (w1, w2, w3)")
        elif from_q4:
            if any(ew.bucketsLoaded and not ew.q4 for ew in bundles):
                raise ValueError("Decoder.prefill: weights='q4' is for Q4 and core-only bundles (an FP16 bucketed bundle prefills with weights='buckets')")
            if any(not ew.bucketsLoaded and ew.core is None for ew in bundles):
                raise ValueError("Decoder.prefill: weights='q4' needs the f16 core of every core-only bundle (wk, wv, wo)")
        elif any(ew.core is None for ew in bundles):
            raise ValueError("Decoder.prefill: every bundle needs its f16 core (Model.random(keep_cores=True), or a Q4 model)")
        if routed and not from_buckets and any(getattr(L, w).core.dim() != 3 or int(getattr(L, w).core.shape[0]) != cfg.numExperts for L in m.layers for w in ("w1", "w2", "w3")):
            raise ValueError("Decoder.prefill: ffn='routed' needs the expert stacks' cores [numExperts, out, in] (Model.random(keep_cores=True))")
        if not 1 <= chunk <= self.PREFILL_MAX_ROWS:
            raise ValueError(f"Decoder.prefill: chunk must be 1 .. {self.PREFILL_MAX_ROWS}")
        if T < 1 or pos0 < 0 or pos0 + T > self.maxTokens:
            raise ValueError(f"Decoder.prefill: tokens {pos0} .. {pos0 + T - 1} do not fit maxTokens = {self.maxTokens}")
        if attention not in ("rows", "block"):
            raise ValueError(f"Decoder.prefill: attention must be 'rows' or 'block', not {attention!r}")
        attend, attendName = ((lib.effort_attention_rows, "attention_rows") if attention == "rows" else
                              (lib.effort_attention_block, "attention_block"))
        g._bind_stream()
        if from_buckets:                                   # (the last refusal: the library looks at each handle's buckets once and remembers)
            for ew in bundles:
                ok = C.c_int(0)
                g.check(lib.effort_weights_bucket_dense_ok(ew.handle, C.byref(ok)), "weights_bucket_dense_ok")
                if not ok.value:
                    raise ValueError("Decoder.prefill: weights='buckets' needs un-bucketable bundles (two entries of one bucket name the same output: "
                                     "the converter reported drops)")
        if from_q4:                                        # (as above: each Q4 handle's buckets and means are looked at once)
            for ew in bundles:
                if not ew.bucketsLoaded:
                    continue
                ok = C.c_int(0)
                g.check(lib.effort_weights_q4_dense_ok(ew.handle, C.byref(ok)), "weights_q4_dense_ok")
                if not ok.value:
                    raise ValueError("Decoder.prefill: weights='q4' needs un-bucketable Q4 bundles (the ranks of every bucket name eight different "
                                     "outputs, every row mean is a finite f16 number)")
        self._prefill_buffers(chunk)
        ck = lambda rc, what: g.check(rc, what)                                     # noqa: E731
        rope = C.c_float(cfg.ropeBase)
        mul, mul_routed = self._block_multiplies(from_buckets, from_q4)
        for b0 in range(0, T, chunk):
            rows, p = min(chunk, T - b0), pos0 + b0
            self.pf_ids[:rows].copy_(torch.tensor(ids[b0:b0 + rows], dtype=torch.int32))
            ck(lib.effort_fetch_rows(g.ctx, _p(m.tokEmbeddings), _p(self.pf_ids), _p(self.pf_h), cfg.stateDim, rows), "fetch_rows")
            delta = None                                   # a product not yet added to h, exactly as in token_step
            for n, L in enumerate(m.layers):
                kc, vc = _p(self.kCache[n]), _p(self.vCache[n])
                ck(lib.effort_add_rmsnorm_mul_rows(g.ctx, _p(self.pf_h), _p(delta), _p(L.attnNorm), _p(self.pf_norm), cfg.stateDim, rows), "rmsnorm_rows")
                for ew, out in ((L.wq, self.pf_xq_temp), (L.wk, self.pf_xk_temp), (L.wv, self.pf_xv_temp)):
                    mul(self.pf_norm, ew, out, rows)
                ck(lib.effort_rope_kv_rows(g.ctx, _p(self.pf_xq_temp), _p(self.pf_xk_temp), _p(self.pf_xv_temp), _p(self.pf_xq), kc, vc, p, rows,
                                           cfg.numHeads, cfg.numHeadsKV, cfg.headDim, self.maxTokens, rope), "rope_kv_rows")
                if n == len(m.layers) - 1:
                    break                                  # nothing after the last layer's cache write reaches a cache
                ck(attend(g.ctx, _p(self.pf_xq), kc, vc, p, rows, _p(self.pf_attnOutput), cfg.numHeads, cfg.headDim, self.maxTokens), attendName)
                mul(self.pf_attnOutput, L.wo, self.pf_attnFfnOut, rows)
                ck(lib.effort_add_rmsnorm_mul_rows(g.ctx, _p(self.pf_h), _p(self.pf_attnFfnOut), _p(L.ffnNorm), _p(self.pf_norm), cfg.stateDim, rows), "rmsnorm_rows")
                if routed:
                    idx2 = self.pf_gateIdxs[n]
                    ck(lib.effort_moe_route_rows(g.ctx, _p(self.pf_h), _p(L.ffnNorm), _p(L.ffnGate), cfg.stateDim, cfg.numExperts, _p(self.pf_gateOut[n]),
                                                 _p(idx2), _p(self.pf_gateVals), rows), "moe_route_rows")
                    mul_routed(self.pf_norm, L.w1, idx2, self.pf_x1r, rows, False)
                    mul_routed(self.pf_norm, L.w3, idx2, self.pf_x3r, rows, False)
                    ck(lib.effort_silu_mul(g.ctx, _p(self.pf_x1r), _p(self.pf_x3r), _p(self.pf_x2r), rows * 2 * cfg.hiddenDim), "silu")
                    mul_routed(self.pf_x2r, L.w2, idx2, self.pf_ffnOutR, rows, True)
                    ck(lib.effort_mix2_add_rows(g.ctx, _p(self.pf_h), _p(self.pf_ffnOutR), _p(self.pf_gateVals), cfg.stateDim, rows), "mix2_add_rows")
                    delta = None                           # the mix landed on h
                    continue
                mul(self.pf_norm, L.w1, self.pf_x1, rows)
                mul(self.pf_norm, L.w3, self.pf_x3, rows)
                ck(lib.effort_silu_mul(g.ctx, _p(self.pf_x1), _p(self.pf_x3), _p(self.pf_x2), rows * cfg.hiddenDim), "silu")
                mul(self.pf_x2, L.w2, self.pf_ffnOut, rows)
                delta = self.pf_ffnOut
        self.pos.fill_(pos0 + T)

    def _graph(self, effort: float, dense: bool, sampled: bool = False, ruled: bool = False):
        key = ("dense",) if dense else (float(effort),)
        if sampled:                                              # the ONLY thing sampling adds to the key: its settings are device values
            key += ("sampled",)
        if ruled:                                                # and the ONLY thing the rules add: one more graph, shared by every Rules
            key += ("rules",)
        pick, rules = True if sampled else None, True if ruled else None
        if key not in self._graphs:
            self.reset()
            self.token_step(effort, dense, pick, rules)          # warm (handles, kernel attributes, rocBLAS, the rules' buffers)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, capture_error_mode="thread_local"):
                self.token_step(effort, dense, pick, rules)
            self.g._bind_stream()
            self._graphs[key] = gr
        return self._graphs[key]

    def status(self) -> int:
        """Device-side conditions of the steps since the last call (effort_decode_status): bit 0 = a step ran past the cache or
        the history buffer (it wrote nothing there), bit 1 = argmax over NaN logits.  Reads and clears."""
        st = C.c_int(0)
        self.g._bind_stream()
        self.g.check(_lib.lib().effort_decode_status(self.g.ctx, C.byref(st)), "decode_status")
        return int(st.value)

    def reset(self):
        self.pos.zero_()
        self.tokId.zero_()
        self.history.zero_()
        if self._rules:
            self.seq.zero_()
            self.stop_pos.fill_(-1)                              # 0xFFFFFFFF: no stop token consumed

    def run(self, tokenIds: list[int], numTokens: int, effort: float = 0.25, dense: bool = False, forced: bool = False,
            collect_logits: bool = False, sampling=None, prefill: bool = False, prefill_chunk: int = 64,
            prefill_attention: str = "rows", prefill_ffn: str = "dense", prefill_weights: str = "cores", rules=None, stop_poll: int = 16):
        """runNetwork(tokens:effort:): feed the prompt one token per step, then continue greedily until ``numTokens``
        steps have run.  ``forced``: every step's input comes from ``tokenIds`` (teacher forcing, for the KL measurement).
        ``sampling``: a ``Sampling`` -- every step's pick is the device-side draw (temperature / top-k / top-p, Philox at counter
        (position, stream) under the seed) instead of the greedy one; the step graph is shared by all settings.
        ``prefill``: the first P - 1 prompt tokens go through ``prefill`` (blocks of ``prefill_chunk`` tokens, one pass over the weights
        per block, DENSE K / V in the caches whatever ``effort`` says) instead of P - 1 steps; step P - 1 -- the last prompt token --
        and every later step are the ordinary captured step at the requested ``effort`` / ``dense`` / ``sampling``.  No pick exists
        for the prefilled positions: the returned list has -1 there, ``collect_logits`` starts at step P - 1, and ``last_prefill_s``
        holds the synchronised wall time of the prefill.  Not with ``forced``.  The default is the token-by-token loop.
        ``prefill_attention`` is ``prefill``'s ``attention`` (``"rows"`` / ``"block"``), ``prefill_ffn`` its ``ffn`` (``"dense"`` /
        ``"routed"``: a Mixtral prompt prefills only with ``"routed"``), ``prefill_weights`` its ``weights`` (``"cores"`` / ``"buckets"`` / ``"q4"``: an
        FP16 model without cores prefills only with ``"buckets"``, a Q4 model without the cores of its Q4 bundles only with ``"q4"``,
        and the caches then hold effort-1.0 K / V, not dense ones).
        ``rules``: a ``Rules`` -- every step applies the generation rules on the device (effort_logit_rules between the LM head and the
        pick: penalties over the last ``last_n`` tokens fed, the logit bias, min-p), the step graph is shared by every setting, and
        ``collect_logits`` still returns the RAW logits.  The prompt never stops a run (``first_pos = len(tokenIds)``); prefilled prompt ids
        are copied into ``seq``, since the kernel records only the steps it runs.  With ``stop_ids``, every ``stop_poll`` replays the
        4-byte ``stop_pos`` is read back and the loop ends once it is set; the generated picks are then scanned on the host (a stop token
        picked by the very last step counts), the returned picks end with the stop token, ``stopped_at`` is the step that picked it (else
        None), and ``pos`` / ``tokId`` are set to continue behind it -- what the replays past it wrote is junk that the next steps
        overwrite.  With ``forced`` the window is the forced inputs and nothing stops.
        Returns (token ids picked at every step, seconds per step measured from the 3rd step on like the reference,
        logits per step if asked)."""
        assert 1 <= len(tokenIds) and numTokens <= self.maxTokens
        if prefill and forced:
            raise ValueError("Decoder.run: prefill=True computes no logits for the prompt, forced=True wants them at every step")
        if rules is not None and not isinstance(rules, Rules):
            raise ValueError("Decoder.run: rules is a Rules or None")
        if int(stop_poll) < 1:
            raise ValueError("Decoder.run: stop_poll >= 1")
        gr = self._graph(effort, dense, sampling is not None, *((True,) if rules is not None else ()))    # (a run without rules: today's call)
        self.reset()
        if sampling is not None:
            self.set_sampling(sampling)
        stops = set(int(t) for t in rules.stop_ids) if rules is not None and not forced else set()
        self.stopped_at = None
        if rules is not None:
            self.set_rules(rules, 0xFFFFFFFF if forced else len(tokenIds))
        logits = []
        t0, timed = None, 0
        skip = min(len(tokenIds) - 1, numTokens) if prefill else 0
        if skip:
            torch.cuda.synchronize()
            tp = time.perf_counter()
            self.prefill(tokenIds[:skip], 0, prefill_chunk, prefill_attention, prefill_ffn, prefill_weights)
            torch.cuda.synchronize()
            self.last_prefill_s = time.perf_counter() - tp
            if rules is not None:
                self.seq[:skip].copy_(torch.tensor([int(t) for t in tokenIds[:skip]], dtype=torch.int32))
        ran = skip                                               # steps 0 .. ran - 1 have a cache row (and, from ``skip`` on, a pick)
        for step in range(skip, numTokens):
            if step < len(tokenIds):
                self.tokId.fill_(int(tokenIds[step]))            # prompt (or forced) token; otherwise the previous pick stays
            elif forced:
                break
            if step == max(2, skip):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            gr.replay()
            if collect_logits:
                logits.append(self.logits.clone())
            if step >= 2:
                timed += 1
            ran = step + 1
            if stops and (ran - skip) % int(stop_poll) == 0 and int(self.stop_pos.item()) != -1:
                break                                            # a stop token was consumed: at most stop_poll replays behind the one that picked it
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / timed if t0 is not None and timed else float("nan")
        picked = self.history[:ran].cpu().tolist()
        picked[:skip] = [-1] * skip                              # prefilled positions: nothing was picked there
        first_generated = len(tokenIds) - 1                      # the pick of the last prompt token's step
        hit = next((k for k in range(first_generated, ran) if picked[k] in stops), None) if stops else None
        if hit is not None:
            self.stopped_at = hit
            picked, logits = picked[:hit + 1], logits[:hit + 1 - skip]
            self.pos.fill_(hit + 1)
            self.tokId.fill_(picked[hit])
        st = self.status()
        if st:
            raise RuntimeError(f"decode loop: device status {st} (1: a step past maxTokens / the history buffer, 2: NaN logits)")
        return picked, dt, (torch.stack(logits) if collect_logits else None)


def kl_divergence(logits_ref: torch.Tensor, logits_test: torch.Tensor) -> float:
    """mean over positions of KL(softmax(ref) || softmax(test))."""
    a = torch.log_softmax(logits_ref.double(), -1)
    b = torch.log_softmax(logits_test.double(), -1)
    return float((a.exp() * (a - b)).sum(-1).mean())
