"""The decode loop on the reference's Q4 model (q4_convert.py:48-66: wq, w1, w2, w3 bucketed in Q4; wk, wv, wo cores only):
Decoder.token_step dispatches per bundle as expertMul does -- Q4 multiply, dense basicMul, or FP16 bucketMul."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cfg(**kw):
    from effort_amd.decode import MistralConfig
    return MistralConfig(**dict(dict(stateDim=4096, hiddenDim=4096, numLayers=2, numHeads=32, numHeadsKV=8, headDim=128, vocab=512), **kw))


@pytest.fixture(scope="module")
def q4_model(hip_lib_built):
    from effort_amd.decode import Model
    return Model.random(_cfg(), seed=5, q4=True)


def test_q4_model_layout(q4_model):
    for L in q4_model.layers:
        for name in ("wq", "w1", "w2", "w3"):
            ew = getattr(L, name)
            assert ew.q4 and ew.bucketsLoaded and ew.core is not None and ew.outliers is not None
            assert ew.outliers.shape[0] == int(ew.inSize * ew.outSize * 0.02)
        for name in ("wk", "wv", "wo"):
            ew = getattr(L, name)
            assert ew.q4 and not ew.bucketsLoaded and ew.buckets is None and ew.core is not None


def test_in_graph_multiplies_match_the_oracle(q4_model, oracle_cpu):
    """After four replayed, unfused steps the decoder's buffers hold the last layer's inputs and outputs: wq, w1, w3 and w2 against
    oracle.bucket_mul_q4 on the GPU's own input vectors, wk, wv and wo against the oracle's dense GEMV (2e-3 of max|want|: the bar the
    dense path is held to against its reference; the kernel rounds the input to f16 as basicMul does)."""
    from effort_amd.decode import Decoder
    from tests.test_gpu_parity import close
    L = q4_model.layers[-1]

    def check_q4(ew, vin, out, effort, what):
        want, n, cutoff = oracle_cpu.bucket_mul_q4(vin.cpu().numpy(), ew.buckets[0].contiguous().cpu().numpy().view(np.uint16), ew.stats[0].cpu().numpy(),
                                                   ew.probes[0].cpu().numpy().view(np.uint16), ew.outliers.cpu().numpy(), ew.inSize, ew.outSize, effort)
        assert close(out.cpu().numpy(), want), what
        return n

    def check_dense(ew, vin, out, what):
        want = oracle_cpu.dense_gemv(ew.core.cpu().numpy().view(np.uint16), vin.cpu().numpy(), round_v_to_f16=True)
        err = float(np.abs(out.cpu().numpy() - want).max() / np.abs(want).max())
        assert err < 2e-3, (what, err)
    for effort in (0.25, 0.6):
        dec = Decoder(q4_model, maxTokens=16, fused_glue=False)
        assert dec.mixed and not dec.fused_glue
        dec.run([3, 77, 130, 9], 4, effort=effort, forced=True)
        check_q4(L.wq, dec.h_norm, dec.xq_temp, effort, "wq")
        check_dense(L.wk, dec.h_norm, dec.xk_temp, "wk")
        check_dense(L.wv, dec.h_norm, dec.xv_temp, "wv")
        check_dense(L.wo, dec.attnOutput, dec.attnFfnOut, "wo")
        check_q4(L.w1, dec.fxn, dec.x1, effort, "w1")
        check_q4(L.w3, dec.fxn, dec.x3, effort, "w3")
        n2 = check_q4(L.w2, dec.x2, dec.ffnOut, effort, "w2")
        assert dec.g.last_dispatch_count() == n2                                 # the step's last multiply launch: exact row count


def test_fused_against_unfused(q4_model):
    from effort_amd.decode import Decoder
    prompt, steps = [3, 77, 130], 8
    plain = Decoder(q4_model, maxTokens=16, fused_glue=False)
    ids_p, _, lg_p = plain.run(prompt, steps, effort=0.5, collect_logits=True)
    forced = prompt + ids_p[len(prompt) - 1:-1]
    _, _, lg_pf = plain.run(forced, steps, effort=0.5, forced=True, collect_logits=True)
    fus = Decoder(q4_model, maxTokens=16, fused_glue=True)
    assert fus.fused_glue and fus.mixed
    ids_f, _, lg_f = fus.run(forced, steps, effort=0.5, forced=True, collect_logits=True)
    err = float((lg_f - lg_pf).abs().max() / lg_pf.abs().max())
    print(f"fused vs unfused Q4 decode: max logit difference {err:.3e} of max|logit|")
    assert ids_f == lg_pf.argmax(-1).tolist() and err < 2e-3, err
    ids_f2, _, lg_f2 = fus.run(forced, steps, effort=0.5, forced=True, collect_logits=True)       # replay after reset(): same bits
    assert ids_f2 == ids_f and torch.equal(lg_f2, lg_f)
    assert fus.status() == 0


def test_dense_path_equals_the_fp16_models(q4_model):
    """dense=True multiplies by the cores, which a Q4 model keeps: bit for bit the dense run of the FP16 model of the same seed."""
    from effort_amd.decode import Decoder, Model
    fp16 = Model.random(_cfg(), seed=5)
    for a, b in zip(fp16.layers, q4_model.layers):
        assert all(torch.equal(getattr(a, n).core, getattr(b, n).core) for n in ("wq", "wk", "wv", "wo", "w1", "w2", "w3"))
    prompt, steps = [3, 77, 130], 8
    ids_a, _, lg_a = Decoder(fp16, maxTokens=16).run(prompt, steps, dense=True, collect_logits=True)
    ids_b, _, lg_b = Decoder(q4_model, maxTokens=16).run(prompt, steps, dense=True, collect_logits=True)
    assert ids_a == ids_b and torch.equal(lg_a, lg_b)


def test_more_effort_is_closer_to_dense(q4_model):
    """Ordering only (sign-and-mean quantisation of Gaussian weights is coarse: no absolute quality number)."""
    from effort_amd.decode import Decoder, kl_divergence
    prompt, steps = [3, 77, 130], 10
    dec = Decoder(q4_model, maxTokens=16, fused_glue=False)
    ids_d, _, lg_d = dec.run(prompt, steps, dense=True, collect_logits=True)
    forced = prompt + ids_d[len(prompt) - 1:-1]
    _, _, lg_1 = dec.run(forced, steps, effort=1.0, forced=True, collect_logits=True)
    _, _, lg_q = dec.run(forced, steps, effort=0.25, forced=True, collect_logits=True)
    kl_1, kl_q = kl_divergence(lg_d, lg_1), kl_divergence(lg_d, lg_q)
    print(f"Q4 decode, KL against dense: effort 1.0 {kl_1:.4f}, effort 0.25 {kl_q:.4f}")
    assert 0.0 <= kl_1 < kl_q, (kl_1, kl_q)


def test_model_load_from_q4_bucket_files(hip_lib_built, tmp_path):
    """convertMistral(q4=True) -> shards -> Model.load(q4=True): the same logits, bit for bit, as a model built directly from the same
    matrices (from_core_q4 / core_only)."""
    from effort_amd import bucketfile as bf
    from effort_amd.decode import Decoder, Layer, Model
    from effort_amd.weights import ExpertWeights
    cfg = _cfg(numLayers=1, vocab=64)
    g = torch.Generator().manual_seed(3)
    mat = lambda o, i: (torch.randn(o, i, generator=g) * 0.02).half()                    # noqa: E731
    vec = lambda n: (1 + 0.1 * torch.randn(n, generator=g)).half()                       # noqa: E731
    kv = cfg.numHeadsKV * cfg.headDim
    src = {"model.norm.weight": vec(4096), "lm_head.weight": mat(cfg.vocab, 4096), "model.embed_tokens.weight": torch.randn(cfg.vocab, 4096, generator=g).half(),
           "model.layers.0.input_layernorm.weight": vec(4096), "model.layers.0.post_attention_layernorm.weight": vec(4096),
           "model.layers.0.self_attn.q_proj.weight": mat(4096, 4096), "model.layers.0.self_attn.k_proj.weight": mat(kv, 4096),
           "model.layers.0.self_attn.v_proj.weight": mat(kv, 4096), "model.layers.0.self_attn.o_proj.weight": mat(4096, 4096),
           "model.layers.0.mlp.gate_proj.weight": mat(4096, 4096), "model.layers.0.mlp.up_proj.weight": mat(4096, 4096),
           "model.layers.0.mlp.down_proj.weight": mat(4096, 4096)}
    bf.convertMistral(src, bf.TensorSaver(str(tmp_path), "model", pad_total=False), numLayers=1, q4=True).save()
    loaded = Model.load(bf.TensorLoader(str(tmp_path), "model"), cfg, q4=True)
    direct = Model(cfg)
    L = Layer()
    L.attnNorm, L.ffnNorm, L.ffnGate = src["model.layers.0.input_layernorm.weight"].to(DEV), src["model.layers.0.post_attention_layernorm.weight"].to(DEV), None
    for name, key in (("wq", "self_attn.q_proj"), ("wk", "self_attn.k_proj"), ("wv", "self_attn.v_proj"), ("wo", "self_attn.o_proj"),
                      ("w1", "mlp.gate_proj"), ("w3", "mlp.up_proj"), ("w2", "mlp.down_proj")):
        core = src[f"model.layers.0.{key}.weight"].to(DEV)
        setattr(L, name, ExpertWeights.from_core_q4(core) if name in ("wq", "w1", "w2", "w3") else ExpertWeights.core_only(core))
    direct.layers.append(L)
    direct.norm, direct.output, direct.tokEmbeddings = src["model.norm.weight"].to(DEV), src["lm_head.weight"].to(DEV), src["model.embed_tokens.weight"].to(DEV)
    assert not loaded.layers[0].wk.bucketsLoaded and loaded.layers[0].w2.q4 and loaded.layers[0].w2.bucketsLoaded
    for fg in (False, True):
        a = Decoder(loaded, maxTokens=16, fused_glue=fg).run([1, 2, 3], 8, effort=0.5, collect_logits=True)
        b = Decoder(direct, maxTokens=16, fused_glue=fg).run([1, 2, 3], 8, effort=0.5, collect_logits=True)
        assert a[0] == b[0] and torch.equal(a[2], b[2]), fg


def test_refusals(q4_model):
    from effort_amd.decode import Decoder, Model
    with pytest.raises(ValueError):
        Decoder(q4_model, maxTokens=16, world=2, emulate_world=True)
    with pytest.raises(ValueError):
        Decoder(q4_model, maxTokens=16, sharded=True)
    with pytest.raises(ValueError):
        Model.random(_cfg(numExperts=4), seed=1, q4=True)
    mixtral = Model.random(_cfg(numExperts=2, numLayers=1), seed=1)
    mixtral.layers[0].wq = q4_model.layers[0].wq                                 # a Q4 bundle in a routed model
    with pytest.raises(ValueError):
        Decoder(mixtral, maxTokens=16)
