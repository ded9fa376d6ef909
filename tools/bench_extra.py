#!/usr/bin/env python
"""tools/bench_extra.py -- the sections round 5's bench.py carried behind the headline and the driver's one command no longer runs
(VERDICT r05 item 7): `by_streams`, `shared_matrices`, `four_contexts`, the timeit-protocol variants, the quality sweeps
(heavy-tailed input, a structured matrix, the structured decode model), the other shapes, `shard_projection` (BASELINE config 4's
column split projected on one GPU), the one-GPU `layer_latency` (a world of one through RCCL + projected ranks), `decode_q4` (the
decode loop on the reference's Q4 model beside the FP16 one) and `decode_mixtral` (the routed decode loop at Mixtral-8x7B shapes: dense,
and effort with the glue kernels separate or folded; its record also goes to profiles/r07_decode_mixtral.json) and `decode_sampled` (the
decode loop ending in the device-side top-k / top-p / temperature pick beside the greedy one, and the two closing kernels alone; its
record also goes to profiles/r08_decode_sampled.json) and `decode_prefill` (prompt ingest: the block multiply effort_dense_gemm_rows
beside the dense GEMV on rotating matrices, and a 256-token prompt through `Decoder.prefill` beside the token-by-token loop; its
record also goes to profiles/r09_prefill.json; asked for alone, it skips the headline job and its matrix sets) and `prefill_attention`
(effort_attention_rows beside effort_attention_block on rotating caches, and 256- and 2048-token prompts through `Decoder.prefill` on
both attention paths; its record also goes to profiles/r10_prefill_attention.json; standalone like `decode_prefill`) and
`prefill_mixtral` (a Mixtral prompt: the routed block multiply beside 8 dense block calls, and Decoder.prefill(ffn="routed") beside the
token loop; its record also goes to profiles/r11_prefill_mixtral.json; standalone too) and `prefill_buckets` (prefill straight from the
bucketed weights beside the core kernel in the same run; its record also goes to profiles/r12_prefill_buckets.json; standalone too) and
`prefill_q4` (prefill straight from the Q4 buckets beside the core and the FP16 bucket kernel in the same run, and whose K caches a Q4
decode agrees with; its record also goes to profiles/r13_prefill_q4.json; standalone too) and `decode_rules` (the decode loop with
the generation rules -- penalties, bias, min-p, stop ids: effort_logit_rules -- beside plain greedy decode, and rules_kernel alone beside
argmax_kernel and sample_kernel; its record also goes to profiles/r14_decode_rules.json; standalone too).

    python tools/bench_extra.py [--sections a,b,...] [--steps 20 --warmup 5 ...bench.py's flags]

Same state object as bench.py (`bench.Bench`: S disjoint sets of 32 converted 4096 x 11008 matrices, one context with lanes), same
timing helpers.  Writes gpurun_out/bench_extra.json and prints a short summary line; each section is on its own try / except.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench as B  # noqa: E402

SECTIONS = ("by_streams", "shared_matrices", "four_contexts", "timeit_protocol", "heavy_tailed_input", "sweep_structured", "other_shapes",
            "shard_projection", "decode_quality", "layer_latency", "decode_q4", "decode_mixtral", "decode_sampled", "decode_prefill", "prefill_attention",
            "prefill_mixtral", "prefill_buckets", "prefill_q4", "decode_rules")
STANDALONE = ("decode_prefill", "prefill_attention", "prefill_mixtral", "prefill_buckets", "prefill_q4", "decode_rules")           # sections that read neither the headline nor the matrix sets of bench.Bench


def by_streams(b, res):
    """ONE context, n launches in flight (effort_set_overlap), each step on its own matrices (one long graph, like the headline)."""
    kb = B.mul_kernel_bytes(b.D, B.IN_DIM, B.OUT_DIM)
    torch = b.torch
    while len(b.out_sets) < 4:
        b.out_sets.append(torch.zeros((B.N_MATS, B.OUT_DIM), device=b.dev))
    bs = {}
    for ns in (1, 2, 3, 4):
        jb = b.job if ns == b.S else B.LaneJob(b.ea, b.local, ns, b.tune)
        gn = jb.capture(b.mul_step(b.args.effort, wsets=b.ew_sets[:max(1, min(ns, len(b.ew_sets)))]), 192)
        bs[str(ns)] = b.rate(B.time_graph(gn, None) / 192 / B.N_MATS, kb)
        del gn
    res["by_streams"] = bs
    res["by_streams_note"] = "one effort_ctx, effort_set_overlap(n): the library keeps n launches in flight; every step in flight on its own 32 matrices"


def shared_matrices(b, res):
    """Round 2's job: every step in flight on the SAME 32 matrices (what the Infinity Cache can contribute)."""
    kb = B.mul_kernel_bytes(b.D, B.IN_DIM, B.OUT_DIM)
    gn = b.job.capture(b.mul_step(b.args.effort), 192)
    res["shared_matrices"] = b.rate(B.time_graph(gn, None) / 192 / B.N_MATS, kb)
    # ... and with the row stream's ordinary cache policy, what such a caller asks for (effort_set_row_reuse: the policy is captured with the launch)
    b.job.ctx.set_row_reuse(True)
    try:
        gr = b.job.capture(b.mul_step(b.args.effort), 192)
    finally:
        b.job.ctx.set_row_reuse(False)
    res["shared_matrices_row_reuse"] = b.rate(B.time_graph(gr, None) / 192 / B.N_MATS, kb)


def four_contexts(b, res):
    """The overlap built by the CALLER from four contexts on four streams (round 2's way) instead of the library's lanes."""
    kb = B.mul_kernel_bytes(b.D, B.IN_DIM, B.OUT_DIM)
    four = B.Job(b.ea, b.local, b.S, b.tune)
    gn = four.capture(b.mul_step(b.args.effort, wsets=b.ew_sets), 192)
    res["four_contexts"] = b.rate(B.time_graph(gn, None) / 192 / B.N_MATS, kb)
    del gn, four


def timeit_full(b, res):
    res["timeit_protocol"] = B.timeit_protocol(b.ea, b.ea.Gpu(b.local), b.dev, efforts=(1.0, 0.7, 0.5, 0.25, 0.15),
                                               variants=(("as_written", 1, 1), ("as_written_overlap4", 4, 1), ("four_outputs_overlap4", 4, 4)),
                                               from_graph=True, dense=(("dense_hip_kernel", False), ("dense_rocblas", True)))


def heavy_tailed_input(b, res):
    """A real rms-normed state has outlier channels: v * exp(N(0,1)), same seeds."""
    torch, ea, job, S, G = b.torch, b.ea, b.job, b.S, b.G
    vh = b.v * torch.exp(torch.randn(B.IN_DIM, generator=b.gen, device=b.dev, dtype=torch.float32))
    slotL, last = (24 - 1) % S, B.N_MATS - 1
    ewsL = b.ew_sets[slotL % len(b.ew_sets)]
    dense = torch.zeros(B.OUT_DIM, device=b.dev)
    heavy = {}
    for e in (0.25, 0.5):
        gh = job.capture(b.mul_step(e, vec=vh, wsets=b.ew_sets), 24)
        Dh = job.last_dispatch_count(24, (B.N_MATS - 1) % G)
        th = B.time_graph(gh, None, reps=2) / 24 / B.N_MATS
        ea.basicMul(vh, ewsL[last].core, dense)
        heavy[str(e)] = {"dispatch_rows": Dh, "us_per_call": round(th * 1e6, 3),
                         "achieved_GBps": round(B.algorithmic_bytes(Dh, B.IN_DIM, B.OUT_DIM) / th / 1e9, 1),
                         "frac_of_hbm_peak": round(B.algorithmic_bytes(Dh, B.IN_DIM, B.OUT_DIM) / th / 1e9 / B.HBM_PEAK_GBPS, 4),
                         "cos_vs_dense": round(ea.cosineSimilarityTo(b.out_sets[slotL][last], dense), 5)}
        del gh
    res["heavy_tailed_input"] = heavy


def sweep_structured(b, res):
    """One STRUCTURED matrix (effort_amd.decode.structured_matrix) and a state as a norm layer with outlier channels leaves it: the
    reference's own check (benchmarks/benchmark.swift:166-177: cos-sim of expertMul vs basicMul)."""
    from effort_amd.decode import structured_matrix, structured_norm_weights
    torch, ea = b.torch, b.ea
    Ws = structured_matrix(B.OUT_DIM, B.IN_DIM, b.gen, b.dev)
    es = ea.ExpertWeights.from_core(Ws)
    es.handle
    x = torch.randn(B.IN_DIM, generator=b.gen, device=b.dev, dtype=torch.float32)
    vs_ = (x / x.pow(2).mean().sqrt()) * structured_norm_weights(B.IN_DIM, b.gen, b.dev).float()
    os_, od_ = torch.zeros(B.OUT_DIM, device=b.dev), torch.zeros(B.OUT_DIM, device=b.dev)
    ea.basicMul(vs_, Ws, od_)
    ss = []
    for e in B.SWEEP:
        ea.bucketMul(vs_, es, None, os_, e)
        ss.append({"effort": e, "dispatch_rows": b.g.last_dispatch_count(), "cos_vs_dense": round(ea.cosineSimilarityTo(os_, od_), 5)})
    res["sweep_structured"] = ss


def other_shapes(b, res):
    other = {}
    for name, (iD, oD, seed, efforts) in {"4096x14336 fp16 (the reference's timed shape)": (4096, 14336, 7321, (0.25,)),
                                           "14336x4096 fp16": (14336, 4096, 5321, (0.25,))}.items():
        sets_w = b.make_sets(16, iD, oD, seed)
        other[name] = {}
        for e in efforts:
            other[name].update(b.three(sets_w, oD, iD, e))
        del sets_w
    res["other_shapes"] = other


def shard_times(b, full_sets, inD, outD, effort, per_launch):
    """Per-rank kernel-only time of a bucket-column split over G GPUs, on this one: a launch = the rank's column shards of
    `per_launch` matrices (rank i % G of matrix i); the steps in flight work disjoint matrix sets."""
    from effort_amd.sharded import ShardedExpertWeights
    torch, one, job, S = b.torch, b.one, b.job, b.S
    rows = {}
    for Gw in (1, 2, 4, 8):
        if (outD // 16) % Gw or (outD // Gw) % 32:
            continue
        sh_sets = full_sets if Gw == 1 else [[ShardedExpertWeights.from_full(e, i % Gw, Gw).local for i, e in enumerate(fs)] for fs in full_sets]
        for fs in sh_sets:
            for x in fs:
                x.handle
                if B.ALIGN_ROWS:
                    x.align_rows()
        lo = outD // Gw
        vx = b.v if inD == B.IN_DIM else torch.randn(inD, generator=b.gen, device=b.dev, dtype=torch.float32)
        nm = len(sh_sets[0])
        sets_x = [torch.zeros((nm, lo), device=b.dev) for _ in range(max(S, len(sh_sets)))]
        r = {}
        for nm_, jb, nst in (("1 launch in flight", one, 8), (f"{S} in flight", job, 16)):
            if jb is one:
                one.S = len(sh_sets)
            try:
                gx = jb.capture(b.mul_step(effort, vec=vx, sets=sets_x, group=per_launch, wsets=sh_sets), nst)
            finally:
                one.S = 1
            Dx = jb.last_dispatch_count(nst, (nm - 1) % per_launch)
            est = B.time_graph(gx, None, reps=2)
            tx = B.time_graph(gx, None, reps=max(4, int(0.05 / max(est, 1e-6)) + 1)) / nst     # per step = per rank per step; timed over >= 50 ms like the headline
            del gx
            ab = nm * B.algorithmic_bytes(Dx, inD, lo)
            r[nm_] = {"us_per_step_per_rank": round(tx * 1e6, 2), "frac_of_hbm_peak": round(ab / tx / 1e9 / B.HBM_PEAK_GBPS, 4)}
        r["columns_per_rank"] = outD // 16 // Gw
        r["row_pitch_bytes"] = sh_sets[0][0].align_rows() if B.ALIGN_ROWS else outD // 16 // Gw * 2
        rows[str(Gw)] = r
        del sh_sets
    for Gw, r in rows.items():
        for k2 in list(r):
            if isinstance(r[k2], dict):
                r[k2]["kernel_only_scaling_efficiency"] = round(rows["1"][k2]["us_per_step_per_rank"] / (int(Gw) * r[k2]["us_per_step_per_rank"]), 3)
    return rows


def shard_projection(b, res):
    """BASELINE.json configs[3] projected on ONE GPU (rank r holds columns [r*C/G, (r+1)*C/G) of every matrix, stats /
    probes replicated; its kernel-only work is a launch of column shards.  Strong scaling: efficiency = t(G=1) / (G * t(G)))."""
    sp = {"note": "per-rank kernel-only time of a bucket-column split, measured on one GPU: a launch of `calls per launch` column shards "
                  "(rank i % G of matrix i), 25 % effort, the steps in flight on disjoint matrix sets; efficiency = t(G=1) / (G * t(G)); "
                  "the all-gather of the outputs is not in it"}
    try:
        sp["4096x11008, 32 calls per launch"] = shard_times(b, b.ew_sets, B.IN_DIM, B.OUT_DIM, 0.25, 32)
    except Exception as ex:                                      # noqa: BLE001
        sp["4096x11008, 32 calls per launch"] = {"error": repr(ex)}
    for iD, oD, seed in ((4096, 4096, 4321), (4096, 14336, 7321), (14336, 4096, 5321)):
        sets_w = b.make_sets(16, iD, oD, seed)
        try:
            sp[f"{iD}x{oD}, 16 calls per launch"] = shard_times(b, sets_w, iD, oD, 0.25, 16)
        except Exception as ex:                                  # noqa: BLE001
            sp[f"{iD}x{oD}, 16 calls per launch"] = {"error": repr(ex)}
        del sets_w
    res["shard_projection"] = sp


def decode_quality(b, res):
    """Quality on STRUCTURED synthetic weights (heavy tails, channel scales, outlier norm channels: what trained models have and
    i.i.d. Gaussians lack), the reference's protocol (benchmarks/benchmark.swift:128-156): greedy text at effort 1.0, then
    teacher-forced predictions at every effort against the effort-1.0 ones.  Not evidence of quality on trained weights (no
    checkpoints offline): reported, never headlined."""
    from effort_amd.decode import Decoder, MistralConfig, Model, kl_divergence
    torch = b.torch
    b.g.set_tuning(0, 0, 0)
    torch.cuda.empty_cache()
    prompt = [1, 733, 16289, 28793, 22557]
    model = Model.random(MistralConfig(), seed=2, structured=True)
    ntq = 224
    dec = Decoder(model, maxTokens=ntq + 8)
    B._GRAPHS_FOR_LIFE.append(dec._graphs)                        # (the dict itself: whatever it collects stays alive)
    ids_1, _, _ = dec.run(prompt, ntq, effort=1.0)
    forced = prompt + ids_1[len(prompt) - 1:-1]
    _, _, lg_dn = dec.run(forced, ntq, dense=True, forced=True, collect_logits=True)
    _, _, lg_1 = dec.run(forced, ntq, effort=1.0, forced=True, collect_logits=True)
    control = lg_1.argmax(-1)
    q = {"model": "Mistral-7B shapes, 32 layers, STRUCTURED random weights (effort_amd.decode.structured_matrix)", "tokens": ntq,
         "protocol": "benchmarks/benchmark.swift:128-156: teacher-forced on the effort-1.0 greedy text; agreement = predictions equal to the effort-1.0 predictions",
         "effort": {}}
    for e in (1.0, 0.7, 0.5, 0.35, 0.25, 0.15, 0.1):
        _, dt_e, _ = dec.run(prompt, 40, effort=e)
        _, _, lg_e = dec.run(forced, ntq, effort=e, forced=True, collect_logits=True)
        q["effort"][str(e)] = {"agreement_vs_effort_1.0": round(float((lg_e.argmax(-1) == control).float().mean()), 4),
                               "agreement_vs_dense": round(float((lg_e.argmax(-1) == lg_dn.argmax(-1)).float().mean()), 4),
                               "kl_vs_dense": round(kl_divergence(lg_dn, lg_e), 5), "tokens_per_s": round(1 / dt_e, 1)}
    res["decode_quality_structured"] = q
    del dec, model


def decode_q4(b, res):
    """The decode loop on the reference's Q4 model (q4_convert.py:48-66: wq, w1, w2, w3 in Q4 with 2 % outliers; wk, wv, wo dense)
    beside the FP16 model of the same matrices: tokens/s at Mistral-7B shapes over 64 tokens -- dense, FP16 at 25 %, Q4 at 25 % with
    the glue folded into the Q4 launches (gate + residual into w2) and without -- and the bytes of both models' bucket data."""
    from effort_amd.decode import Decoder, MistralConfig, Model
    torch = b.torch
    b.g.set_tuning(0, 0, 0)
    torch.cuda.empty_cache()
    prompt, nt = [1, 733, 16289, 28793, 22557], 64
    names = ("wq", "wk", "wv", "wo", "w1", "w2", "w3")

    def nbytes(model):
        bk = sum(getattr(L, n).buckets.numel() * 2 for L in model.layers for n in names if getattr(L, n).bucketsLoaded)
        aux = sum(getattr(L, n).stats.numel() * getattr(L, n).stats.element_size() + (0 if getattr(L, n).outliers is None else getattr(L, n).outliers.shape[0] * 4)
                  for L in model.layers for n in names if getattr(L, n).bucketsLoaded)       # (outliers: four bytes each once registered)
        cores = sum(getattr(L, n).core.numel() * 2 for L in model.layers for n in names if not getattr(L, n).bucketsLoaded)
        return {"buckets": bk, "stats_and_outlier_index": aux, "dense_cores_of_core_only_bundles": cores}

    def tps(dec, **kw):
        best = 0.0
        for _ in range(3):
            _, dt, _ = dec.run(prompt, nt, **kw)
            best = max(best, 1 / dt)
        return round(best, 1)
    out = {"model": "Mistral-7B shapes, 32 layers, random weights, seed 1", "tokens": nt, "protocol": "best of 3 runs of 64 tokens, hipGraph replay, timed from the 3rd step"}
    model = Model.random(MistralConfig(), seed=1)
    dec = Decoder(model, maxTokens=nt + 8)
    B._GRAPHS_FOR_LIFE.append(dec._graphs)
    out["dense_tokens_per_s"] = tps(dec, dense=True)
    out["fp16_effort_0.25_tokens_per_s"] = tps(dec, effort=0.25)
    out["fp16_bytes"] = nbytes(model)
    del dec, model
    torch.cuda.empty_cache()
    model = Model.random(MistralConfig(), seed=1, q4=True)
    out["q4_bytes"] = nbytes(model)
    for key, fg in (("q4_effort_0.25_unfused_tokens_per_s", False), ("q4_effort_0.25_fused_gate_resid_tokens_per_s", True)):
        dec = Decoder(model, maxTokens=nt + 8, fused_glue=fg)
        B._GRAPHS_FOR_LIFE.append(dec._graphs)
        out[key] = tps(dec, effort=0.25)
        if not fg:
            out["q4_model_dense_tokens_per_s"] = tps(dec, dense=True)
        del dec
    res["decode_q4"] = out
    del model


def decode_mixtral(b, res):
    """The routed decode loop at Mixtral-8x7B shapes (state 4096, hidden 14336, 8 experts, 32 / 8 heads), structured weights, 8 LAYERS
    (buckets + cores of 8 layers are about 45 GB), 64 tokens: ms per token and us per layer for the dense baseline (the picked experts'
    cores through effort_dense_gemv_expert, nothing gathered), effort 25 % with the separate glue kernels (12 launches per layer),
    25 % folded (Decoder(fused_glue=True): 7 launches) and 50 % folded.  Fused and unfused run in this one process, one after the other."""
    from effort_amd.decode import Decoder, MistralConfig, Model
    torch = b.torch
    b.g.set_tuning(0, 0, 0)
    b.g.set_dense_backend(False)
    torch.cuda.empty_cache()
    prompt, nt, layers = [1, 733, 16289, 28793, 22557], 64, 8
    cfg = MistralConfig(numLayers=layers, numExperts=8)
    model = Model.random(cfg, seed=1, structured=True)

    def timed(dec, **kw):
        best, ids = float("inf"), None
        for _ in range(3):
            ids, dt, _ = dec.run(prompt, nt, **kw)
            best = min(best, dt)
        return {"ms_per_token": round(best * 1e3, 4), "us_per_layer": round(best * 1e6 / layers, 2)}, ids
    out = {"model": "Mixtral-8x7B shapes (4096 / 14336, 8 experts, top-2, 32 / 8 heads), 8 layers, STRUCTURED random weights, seed 1", "tokens": nt,
           "layers": layers, "protocol": "best of 3 runs of 64 tokens, hipGraph replay, timed from the 3rd step; us_per_layer = time per token / 8 "
                                         "(the embedding fetch, the output norm, the LM head and the argmax are in it)",
           "launches_per_layer": {"unfused": 12, "fused": 7}}
    plain = Decoder(model, maxTokens=nt + 8)
    folded = Decoder(model, maxTokens=nt + 8, fused_glue=True)
    assert folded.fused_glue and not plain.fused_glue
    B._GRAPHS_FOR_LIFE.append(plain._graphs)
    B._GRAPHS_FOR_LIFE.append(folded._graphs)
    out["dense_expert_gemv"], _ = timed(plain, dense=True)
    out["effort_0.25_unfused"], ids_u = timed(plain, effort=0.25)
    out["effort_0.25_fused"], ids_f = timed(folded, effort=0.25)
    out["effort_0.25_unfused_again"], _ = timed(plain, effort=0.25)          # (the order of the two is not what separates them)
    out["effort_0.5_fused"], _ = timed(folded, effort=0.5)
    out["effort_0.5_unfused"], _ = timed(plain, effort=0.5)
    out["fused_picks_the_unfused_tokens"] = ids_u == ids_f
    out["fused_over_unfused_0.25"] = round(out["effort_0.25_unfused"]["ms_per_token"] / out["effort_0.25_fused"]["ms_per_token"], 4)
    out["default"] = "unfused (Decoder(mixtral_model).fused_glue is False); fused_glue=True opts in"
    res["decode_mixtral"] = out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r07_decode_mixtral.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del plain, folded, model


CLOSING_KERNEL_PROTOCOL = ("device events around replays of a captured graph, best of 3 windows; one launch per graph x 512 replays "
                           "(graph-launch overhead included, the same for both kernels), and 64 launches per graph x 32 replays")


def us_per_graph_launch(torch, g, fn, per_graph, replays):
    """us per launch of ``fn`` (one launch on the context ``g``), captured ``per_graph`` times into one graph: device events around
    ``replays`` replays, best of 3 windows."""
    g._bind_stream()
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    B._GRAPHS_FOR_LIFE.append(gr)
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        for _ in range(per_graph):
            fn()
    g._bind_stream()
    for _ in range(20):
        gr.replay()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / (replays * per_graph))
    return round(best, 2)


def decode_sampled(b, res):
    """Sampled decode beside greedy decode in ONE process (the yardstick is this process's own greedy figure): Mistral-7B shapes, 25 %
    effort, 64 tokens -- greedy, sampled (top_k 40, temperature 0.8), sampled (top_k 64, top_p 0.9), greedy again -- and the closing
    kernels alone: argmax_kernel and sample_kernel at n = 32000, device events around replays of a captured graph of that ONE launch
    (and of 64 launches in a row: the graph-launch overhead spread over 64)."""
    import ctypes as C

    import effort_amd
    from effort_amd.decode import Decoder, MistralConfig, Model
    from effort_amd.sampling import Sampling
    torch = b.torch
    b.g.set_tuning(0, 0, 0)
    torch.cuda.empty_cache()
    prompt, nt = [1, 733, 16289, 28793, 22557], 64
    model = Model.random(MistralConfig(), seed=1)
    dec = Decoder(model, maxTokens=nt + 8)
    B._GRAPHS_FOR_LIFE.append(dec._graphs)

    def tps(**kw):
        best, ids = 0.0, None
        for _ in range(3):
            ids, dt, _ = dec.run(prompt, nt, effort=0.25, **kw)
            best = max(best, 1 / dt)
        return round(best, 1), ids
    out = {"model": "Mistral-7B shapes, 32 layers, random weights, seed 1", "tokens": nt, "effort": 0.25,
           "protocol": "best of 3 runs of 64 tokens, hipGraph replay, timed from the 3rd step; the four figures in this order, one process"}
    out["greedy_tokens_per_s"], ids_g = tps()
    out["sampled_top_k_40_temperature_0.8_tokens_per_s"], ids_a = tps(sampling=Sampling(temperature=0.8, top_k=40, seed=1))
    out["sampled_top_k_64_top_p_0.9_tokens_per_s"], ids_b = tps(sampling=Sampling(temperature=1.0, top_k=64, top_p=0.9, seed=1))
    out["greedy_again_tokens_per_s"], ids_g2 = tps()
    greedy = (out["greedy_tokens_per_s"] + out["greedy_again_tokens_per_s"]) / 2
    out["greedy_run_to_run"] = round(out["greedy_again_tokens_per_s"] / out["greedy_tokens_per_s"] - 1, 4)
    out["sampled_top_k_40_vs_greedy_mean"] = round(out["sampled_top_k_40_temperature_0.8_tokens_per_s"] / greedy - 1, 4)
    out["sampled_top_k_64_vs_greedy_mean"] = round(out["sampled_top_k_64_top_p_0.9_tokens_per_s"] / greedy - 1, 4)
    out["greedy_runs_agree"] = ids_g == ids_g2
    out["sampled_runs_leave_the_greedy_text"] = ids_a != ids_g and ids_b != ids_g
    # the closing kernels alone, on the last step's logits
    g, lib = dec.g, effort_amd.lib()
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    tok, pos = torch.zeros(1, dtype=torch.int32, device=b.dev), torch.zeros(1, dtype=torch.int32, device=b.dev)
    n = model.cfg.vocab

    def launch_argmax():
        g._bind_stream()                                                         # (inside a capture: the capture's stream)
        g.check(lib.effort_argmax(g.ctx, p(dec.logits), n, p(tok), p(pos), None, 0), "argmax")

    def launch_sample():
        g._bind_stream()
        g.check(lib.effort_sample(g.ctx, p(dec.logits), n, p(dec.sample_params), p(tok), p(pos), None, 0, None, None), "sample")

    us_per_launch = lambda fn, per_graph, replays: us_per_graph_launch(torch, g, fn, per_graph, replays)      # noqa: E731
    k = {"n": n, "protocol": CLOSING_KERNEL_PROTOCOL}
    for name, sm in (("sample_top_k_40_temperature_0.8", Sampling(temperature=0.8, top_k=40, seed=1)),
                     ("sample_top_k_64_top_p_0.9", Sampling(temperature=1.0, top_k=64, top_p=0.9, seed=1))):
        dec.set_sampling(sm)
        k[name] = {"us_per_launch_one_per_graph": us_per_launch(launch_sample, 1, 512), "us_per_launch_64_per_graph": us_per_launch(launch_sample, 64, 32)}
    k["argmax"] = {"us_per_launch_one_per_graph": us_per_launch(launch_argmax, 1, 512), "us_per_launch_64_per_graph": us_per_launch(launch_argmax, 64, 32)}
    out["closing_kernel"] = k
    res["decode_sampled"] = out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r08_decode_sampled.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del dec, model


def decode_rules(b, res):
    """Decode with the generation rules (effort_logit_rules between the LM head and the pick) beside plain greedy decode in ONE process,
    decode_sampled's protocol: Mistral-7B shapes, 25 % effort, 64 tokens -- greedy, Rules(repetition_penalty=1.1) at last_n 64, a full
    load (last_n 1024, 256 biases, min_p 0.05, one stop id that never occurs), greedy again -- and rules_kernel alone at n = 32000 under
    the same three settings, argmax_kernel and sample_kernel beside it in the same run."""
    import ctypes as C

    import effort_amd
    from effort_amd.decode import Decoder, MistralConfig, Model
    from effort_amd.rules import Rules
    from effort_amd.sampling import Sampling
    torch = b.torch
    b.g.set_tuning(0, 0, 0)
    torch.cuda.empty_cache()
    prompt, nt = [1, 733, 16289, 28793, 22557], 64
    model = Model.random(MistralConfig(), seed=1)
    n = model.cfg.vocab
    dec = Decoder(model, maxTokens=nt + 8)
    B._GRAPHS_FOR_LIFE.append(dec._graphs)
    light = Rules(repetition_penalty=1.1, last_n=64)
    full = Rules(repetition_penalty=1.1, presence_penalty=0.1, frequency_penalty=0.1, last_n=1024, min_p=0.05,
                 logit_bias={1000 + 97 * i: (-1.0 if i % 2 else 0.5) for i in range(256)}, stop_ids=(n - 1,))

    def tps(**kw):
        best, ids = 0.0, None
        for _ in range(3):
            ids, dt, _ = dec.run(prompt, nt, effort=0.25, **kw)
            best = max(best, 1 / dt)
        return round(best, 1), ids
    out = {"model": "Mistral-7B shapes, 32 layers, random weights, seed 1", "tokens": nt, "effort": 0.25,
           "protocol": "best of 3 runs of 64 tokens, hipGraph replay, timed from the 3rd step; the four figures in this order, one process; "
                       "the full load polls stop_pos every 16 replays (4 bytes, one synchronisation)",
           "full_load": "last_n 1024 (the window of a 64-token run holds at most 64 ids), 256 biases, min_p 0.05, penalties 1.1 / 0.1 / 0.1, one stop id never picked"}
    out["greedy_tokens_per_s"], ids_g = tps()
    out["rules_repetition_1.1_last_n_64_tokens_per_s"], ids_a = tps(rules=light)
    out["rules_full_load_tokens_per_s"], ids_b = tps(rules=full)
    out["greedy_again_tokens_per_s"], ids_g2 = tps()
    greedy = (out["greedy_tokens_per_s"] + out["greedy_again_tokens_per_s"]) / 2
    out["greedy_run_to_run"] = round(out["greedy_again_tokens_per_s"] / out["greedy_tokens_per_s"] - 1, 4)
    out["rules_repetition_vs_greedy_mean"] = round(out["rules_repetition_1.1_last_n_64_tokens_per_s"] / greedy - 1, 4)
    out["rules_full_load_vs_greedy_mean"] = round(out["rules_full_load_tokens_per_s"] / greedy - 1, 4)
    out["greedy_runs_agree"] = ids_g == ids_g2
    out["ruled_runs_leave_the_greedy_text"] = [ids_a != ids_g, ids_b != ids_g]
    out["full_load_stopped_at"] = dec.stopped_at
    # the kernels alone, on the last step's logits; the window of the rules is FULL there: a seq of its own, 1024 + 8 ids out of a pool
    # of 300, the position at 1024 + 4
    g, lib = dec.g, effort_amd.lib()
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    tok, pos = torch.zeros(1, dtype=torch.int32, device=b.dev), torch.zeros(1, dtype=torch.int32, device=b.dev)
    rpos = torch.full((1,), 1024 + 4, dtype=torch.int32, device=b.dev)           # (effort_logit_rules reads the position and never advances it)
    seq = (torch.arange(1024 + 8, dtype=torch.int64) * 7919 % 300 * 101 % n).to(torch.int32).to(b.dev)

    def launch_argmax():
        g._bind_stream()                                                         # (inside a capture: the capture's stream)
        g.check(lib.effort_argmax(g.ctx, p(dec.logits), n, p(tok), p(pos), None, 0), "argmax")

    def launch_sample():
        g._bind_stream()
        g.check(lib.effort_sample(g.ctx, p(dec.logits), n, p(dec.sample_params), p(tok), p(pos), None, 0, None, None), "sample")

    def launch_rules():
        g._bind_stream()
        g.check(lib.effort_logit_rules(g.ctx, p(dec.logits), n, p(dec.rules_params), p(tok), p(rpos), p(seq), int(seq.numel()), p(dec.bias_ids),
                                       p(dec.bias_vals), p(dec.stop_pos), p(dec.logits_ruled)), "logit_rules")
    us = lambda fn: {"us_per_launch_one_per_graph": us_per_graph_launch(torch, g, fn, 1, 512),       # noqa: E731
                     "us_per_launch_64_per_graph": us_per_graph_launch(torch, g, fn, 64, 32)}
    k = {"n": n, "protocol": CLOSING_KERNEL_PROTOCOL, "rules_position": 1024 + 4}
    k["argmax"] = us(launch_argmax)
    dec.set_sampling(Sampling(temperature=0.8, top_k=40, seed=1))
    k["sample_top_k_40_temperature_0.8"] = us(launch_sample)
    for name, r in (("rules_off", Rules()), ("rules_repetition_1.1_last_n_64", light),
                    ("rules_window_1024_only", Rules(repetition_penalty=1.1, presence_penalty=0.1, frequency_penalty=0.1, last_n=1024)),
                    ("rules_256_biases_only", Rules(last_n=0, logit_bias=full.logit_bias)), ("rules_min_p_only", Rules(last_n=0, min_p=0.05)),
                    ("rules_full_load", full)):
        dec.set_rules(r, 5)
        k[name] = us(launch_rules)
    k["argmax_again"] = us(launch_argmax)
    out["kernel_alone"] = k
    res["decode_rules"] = out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r14_decode_rules.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del dec, model


# ---- what the four prefill sections measure with
def us_per_call(b, fn, calls):
    """us per library call of ``fn`` (``calls`` of them, enqueued on the context's stream): one warm call (the first bucket call of a
    handle runs its check, which synchronises), ``fn`` captured into one graph, 3 warm replays, then device events around 4 replays per
    window, best of 3 windows."""
    torch, g = b.torch, b.g
    g._bind_stream()
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    B._GRAPHS_FOR_LIFE.append(gr)
    with torch.cuda.graph(gr, capture_error_mode="thread_local"):
        fn()
    g._bind_stream()
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(4):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / (4 * calls))
    return best


def timed_prefill(b, dec, prompt, **kw):
    """ms per prompt token of ``dec.prefill(prompt, **kw)``: eager, synchronised wall time over the whole prompt, best of 3 after a warm
    call (it makes the buffers, warms the kernels and runs every handle's check; not timed)."""
    torch = b.torch
    dec.prefill(prompt, **kw)
    best = float("inf")
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.prefill(prompt, **kw)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return round(best * 1e3 / len(prompt), 4)


def token_loop(dec, prompt, **kw):
    """ms per prompt token of the prompt ingested token by token through the captured step, best of 2 runs."""
    best = float("inf")
    for _ in range(2):
        _, dt, _ = dec.run(prompt, len(prompt), **kw)
        best = min(best, dt)
    return round(best * 1e3, 4)


def decode_prefill(b, res):
    """Prompt ingest.  Kernel legs: effort_dense_gemm_rows at rows = 1, 16, 64 beside effort_dense_gemv on the decode loop's four matrix
    shapes -- a pass over ROTATING disjoint matrices (more than 768 MB of them per shape: nothing of a matrix is still cached when its
    turn comes again) captured into one graph, device events around replays, best of 3 windows after a warm-up; us per call and TB/s of
    weight bytes.  Model legs, Mistral-7B shapes, a 256-token prompt, one process: token by token through the captured dense step (how
    a prompt is ingested without prefill: the baseline) and at 25 % effort, and `Decoder.prefill` at chunk 16 and 64 (synchronised wall
    time, best of 3, eager launches: the host's launch work is in it); ms per prompt token each."""
    import ctypes as C

    import effort_amd
    from effort_amd.decode import Decoder, MistralConfig, Model
    torch = b.torch
    g, lib = b.g, effort_amd.lib()
    g.set_tuning(0, 0, 0)
    g.set_dense_backend(False)
    torch.cuda.empty_cache()
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    gen = torch.Generator(device=b.dev)
    gen.manual_seed(77)

    kern = {"protocol": "one pass over the rotating matrices per graph, 4 replays per window, best of 3 windows, device events; TB/s = weight bytes / time"}
    for outD, inD in ((4096, 4096), (14336, 4096), (4096, 14336), (1024, 4096)):
        nbytes = outD * inD * 2
        count = max(4, -(-(768 << 20) // nbytes))
        Ws = [(torch.randn((outD, inD), generator=gen, device=b.dev, dtype=torch.float32) * 0.02).to(torch.float16) for _ in range(count)]
        x = torch.randn((64, inD), generator=gen, device=b.dev, dtype=torch.float32)
        out = torch.zeros((64, outD), device=b.dev)

        def gemv():
            g._bind_stream()
            for W in Ws:
                g.check(lib.effort_dense_gemv(g.ctx, p(W), p(x), p(out), inD, outD), "dense_gemv")

        def gemm(rows):
            def fn():
                g._bind_stream()
                for W in Ws:
                    g.check(lib.effort_dense_gemm_rows(g.ctx, p(W), p(x), p(out), inD, outD, rows), "dense_gemm_rows")
            return fn
        row = {"matrices": count, "weight_bytes": nbytes}
        for name, fn in (("dense_gemv", gemv), ("gemm_rows_1", gemm(1)), ("gemm_rows_16", gemm(16)), ("gemm_rows_64", gemm(64))):
            us = us_per_call(b, fn, count)
            row[name] = {"us_per_call": round(us, 2), "TBps_of_weight_bytes": round(nbytes / us / 1e6, 3)}
        for rows in (1, 16, 64):
            row[f"gemm_rows_{rows}_over_gemv_time"] = round(row[f"gemm_rows_{rows}"]["us_per_call"] / row["dense_gemv"]["us_per_call"], 3)
        kern[f"{inD}->{outD}"] = row
        del Ws, x, out
        torch.cuda.empty_cache()
    out = {"kernel": kern}

    nprompt = 256
    model = Model.random(MistralConfig(), seed=1)
    dec = Decoder(model, maxTokens=nprompt + 8)
    B._GRAPHS_FOR_LIFE.append(dec._graphs)
    prompt = [int(t) for t in torch.randint(0, model.cfg.vocab, (nprompt,), generator=torch.Generator().manual_seed(3))]

    m = {"model": "Mistral-7B shapes, 32 layers, random weights, seed 1", "prompt_tokens": nprompt,
         "protocol": "token loop: hipGraph replay of the step, timed from the 3rd step, best of 2 runs (LM head and pick in it); prefill: eager, "
                     "synchronised wall time of Decoder.prefill over the whole prompt, best of 3 after a warm call (no LM head, the last layer "
                     "stops after its cache write)"}
    m["token_by_token_dense_ms_per_prompt_token"] = token_loop(dec, prompt, dense=True)
    m["token_by_token_effort_0.25_ms_per_prompt_token"] = token_loop(dec, prompt, effort=0.25)
    m["prefill_chunk_16_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, chunk=16)
    m["prefill_chunk_64_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, chunk=64)
    m["prefill_chunk_16_again_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, chunk=16)
    ids, _, _ = dec.run(prompt, nprompt + 4, effort=0.25, prefill=True)
    m["run_prefill_true_last_prefill_s"] = round(dec.last_prefill_s, 5)
    m["run_prefill_true_picks"] = ids[nprompt - 1:]
    base = m["token_by_token_dense_ms_per_prompt_token"]
    for k in ("token_by_token_effort_0.25", "prefill_chunk_16", "prefill_chunk_64"):
        m[f"dense_token_loop_over_{k}"] = round(base / m[f"{k}_ms_per_prompt_token"], 2)
    m["prompt_512_tokens_projected_s"] = {k: round(m[f"{k}_ms_per_prompt_token"] * 512 / 1e3, 4)
                                          for k in ("token_by_token_dense", "token_by_token_effort_0.25", "prefill_chunk_16", "prefill_chunk_64")}
    out["model"] = m
    res["decode_prefill"] = out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r09_prefill.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del dec, model


def prefill_mixtral(b, res):
    """Mixtral prompt ingest.  Kernel legs, decode_prefill's protocol: effort_dense_gemm_rows_routed on 4096 -> 14336 x 8 experts and
    14336 -> 4096 x 8 at 16 and 64 rows under a uniform random routing (two different experts per token), beside effort_dense_gemm_rows
    on every expert's matrix of the same stacks at the same rows -- 8 of those calls stream the bytes one routed call streams when
    every expert is picked.  Two stacks in rotation (1.9 GB).  Model legs, Mixtral-8x7B shapes with decode_mixtral's 8 layers, a
    256-token prompt, one process, in this order: token by token dense, token by token at 25 % effort, prefill(ffn="routed") at chunk
    16 and 64, the first leg again; ms per prompt token each, and the spread of the two dense token-loop legs."""
    import ctypes as C

    import effort_amd
    from effort_amd.decode import Decoder, MistralConfig, Model
    torch = b.torch
    g, lib = b.g, effort_amd.lib()
    g.set_tuning(0, 0, 0)
    g.set_dense_backend(False)
    torch.cuda.empty_cache()
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    gen = torch.Generator(device=b.dev)
    gen.manual_seed(78)
    E = 8

    kern = {"protocol": "one pass over two rotating stacks per graph, 4 replays per window, best of 3 windows, device events; routing: two "
                        "different experts per token, uniform; dense_x8 = 8 x the time of one effort_dense_gemm_rows call on an expert's matrix"}
    for outD, inD in ((14336, 4096), (4096, 14336)):
        stacks = [torch.stack([(torch.randn((outD, inD), generator=gen, device=b.dev, dtype=torch.float32) * 0.02).to(torch.float16) for _ in range(E)])
                  for _ in range(2)]
        x = torch.randn((128, inD), generator=gen, device=b.dev, dtype=torch.float32)
        out = torch.zeros((128, outD), device=b.dev)
        idx2 = torch.stack([torch.randperm(E, generator=gen, device=b.dev)[:2] for _ in range(64)]).to(torch.int32).contiguous()
        row = {"stacks": 2, "stack_bytes": E * outD * inD * 2}
        for rows in (16, 64):
            def routed(rows=rows):
                g._bind_stream()
                for W in stacks:
                    g.check(lib.effort_dense_gemm_rows_routed(g.ctx, p(W), E, p(idx2), p(x), 0, p(out), inD, outD, rows), "dense_gemm_rows_routed")

            def dense(rows=rows):
                g._bind_stream()
                for W in stacks:
                    for e in range(E):
                        g.check(lib.effort_dense_gemm_rows(g.ctx, p(W[e]), p(x), p(out), inD, outD, rows), "dense_gemm_rows")
            picked = len(set(idx2[:rows].reshape(-1).tolist()))
            r_us, d_us = us_per_call(b, routed, 2), 8 * us_per_call(b, dense, 2 * E)
            row[f"rows_{rows}"] = {"experts_picked": picked, "routed_us_per_call": round(r_us, 2), "dense_x8_us": round(d_us, 2),
                                   "routed_over_dense_x8": round(r_us / d_us, 3),
                                   "routed_TBps_of_picked_bytes": round(picked * outD * inD * 2 / r_us / 1e6, 3)}
        kern[f"{inD}->{outD}x{E}"] = row
        del stacks, x, out
        torch.cuda.empty_cache()
    out = {"kernel": kern}

    nprompt, layers = 256, 8
    model = Model.random(MistralConfig(numLayers=layers, numExperts=E), seed=1, structured=True)
    dec = Decoder(model, maxTokens=nprompt + 8)
    B._GRAPHS_FOR_LIFE.append(dec._graphs)
    prompt = [int(t) for t in torch.randint(0, model.cfg.vocab, (nprompt,), generator=torch.Generator().manual_seed(3))]

    m = {"model": "Mixtral-8x7B shapes (4096 / 14336, 8 experts, top-2, 32 / 8 heads), 8 layers, STRUCTURED random weights, seed 1",
         "prompt_tokens": nprompt,
         "protocol": "token loop: hipGraph replay of the step, timed from the 3rd step, best of 2 runs (LM head and pick in it); prefill: eager, "
                     "synchronised wall time of Decoder.prefill(ffn='routed') over the whole prompt, best of 3 after a warm call (no LM head, the "
                     "last layer stops after its cache write)"}
    m["token_by_token_dense_ms_per_prompt_token"] = token_loop(dec, prompt, dense=True)
    m["token_by_token_effort_0.25_ms_per_prompt_token"] = token_loop(dec, prompt, effort=0.25)
    m["prefill_routed_chunk_16_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, chunk=16, ffn="routed")
    m["prefill_routed_chunk_64_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, chunk=64, ffn="routed")
    m["token_by_token_dense_again_ms_per_prompt_token"] = token_loop(dec, prompt, dense=True)
    base, again = m["token_by_token_dense_ms_per_prompt_token"], m["token_by_token_dense_again_ms_per_prompt_token"]
    m["token_loop_legs_spread"] = round(abs(base - again) / min(base, again), 4)
    for k in ("token_by_token_effort_0.25", "prefill_routed_chunk_16", "prefill_routed_chunk_64"):
        m[f"dense_token_loop_over_{k}"] = round(base / m[f"{k}_ms_per_prompt_token"], 2)
    m["routed_chunk_64_faster_than_the_dense_token_loop"] = m["prefill_routed_chunk_64_ms_per_prompt_token"] < min(base, again)
    out["model"] = m
    res["prefill_mixtral"] = out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r11_prefill_mixtral.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del dec, model


def prefill_buckets(b, res):
    """Prefill straight from the bucketed weights (effort_bucket_gemm_rows: the block multiply un-bucketing on the fly) beside the core
    kernel MEASURED IN THE SAME RUN.  Kernel legs, decode_prefill's protocol (rotating disjoint matrices, more than 768 MB of them per
    shape and kernel, one pass per graph, best of 3 windows): us per call at 16 and 64 rows on the decode loop's four shapes, the core
    leg on ``unbucket()`` of the same buckets.  Model legs, Mistral-7B shapes, a 256-token prompt: `Decoder.prefill` ms per prompt token
    with ``weights="cores"`` and ``weights="buckets"`` (eager, synchronised wall time, best of 3), the cosine of the bucket-prefilled K
    caches against the core-prefilled ones (the cores here are the DENSE ones: what the 4-bit perturbation of every weight costs), and
    ``torch.cuda.memory_allocated`` for the model with its cores and after dropping them -- after which the prompt is prefilled once more."""
    import ctypes as C
    import gc

    import effort_amd
    from effort_amd.decode import Decoder, MistralConfig, Model
    from effort_amd.weights import ExpertWeights
    torch = b.torch
    g, lib = b.g, effort_amd.lib()
    g.set_tuning(0, 0, 0)
    g.set_dense_backend(False)
    torch.cuda.empty_cache()
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    gen = torch.Generator(device=b.dev)
    gen.manual_seed(78)

    kern = {"protocol": "one pass over the rotating matrices per graph, 4 replays per window, best of 3 windows, device events; both kernels in this run; "
                        "a workgroup of the bucket kernel owns 32 bucket columns (64 bytes of every bucket row, 512 outputs)"}
    for outD, inD in ((4096, 4096), (14336, 4096), (4096, 14336), (1024, 4096)):
        nbytes = outD * inD * 2
        count = max(4, -(-(768 << 20) // nbytes))
        ews = [ExpertWeights.from_core((torch.randn((outD, inD), generator=gen, device=b.dev, dtype=torch.float32) * 0.02).to(torch.float16))
               for _ in range(count)]
        for ew in ews:
            ew.core = ew.unbucket()[0].contiguous()
            ew.handle
        x = torch.randn((64, inD), generator=gen, device=b.dev, dtype=torch.float32)
        out = torch.zeros((64, outD), device=b.dev)

        def cores(rows):
            def fn():
                g._bind_stream()
                for ew in ews:
                    g.check(lib.effort_dense_gemm_rows(g.ctx, p(ew.core), p(x), p(out), inD, outD, rows), "dense_gemm_rows")
            return fn

        def buckets(rows):
            def fn():
                g._bind_stream()
                for ew in ews:
                    g.check(lib.effort_bucket_gemm_rows(g.ctx, ew.handle, 0, p(x), p(out), rows), "bucket_gemm_rows")
            return fn
        row = {"matrices": count, "weight_bytes": nbytes, "bucket_row_pitch": ews[0].rowPitch}
        for rows in (16, 64):
            for name, fn in ((f"core_rows_{rows}", cores(rows)), (f"bucket_rows_{rows}", buckets(rows))):
                us = us_per_call(b, fn, count)
                row[name] = {"us_per_call": round(us, 2), "TBps_of_weight_bytes": round(nbytes / us / 1e6, 3)}
            row[f"bucket_over_core_time_{rows}"] = round(row[f"bucket_rows_{rows}"]["us_per_call"] / row[f"core_rows_{rows}"]["us_per_call"], 3)
        kern[f"{inD}->{outD}"] = row
        del ews, x, out
        gc.collect()
        torch.cuda.empty_cache()
    out = {"kernel": kern}

    nprompt = 256
    model = Model.random(MistralConfig(), seed=1)
    torch.cuda.synchronize()
    mem_with = torch.cuda.memory_allocated()
    dec = Decoder(model, maxTokens=nprompt + 8)
    prompt = [int(t) for t in torch.randint(0, model.cfg.vocab, (nprompt,), generator=torch.Generator().manual_seed(3))]

    m = {"model": "Mistral-7B shapes, 32 layers, random weights, seed 1", "prompt_tokens": nprompt,
         "protocol": "eager, synchronised wall time of Decoder.prefill(chunk=64) over the whole prompt, best of 3 after a warm call"}
    m["prefill_cores_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, weights="cores")
    k_cores = [k[:nprompt].clone() for k in dec.kCache]
    m["prefill_buckets_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, weights="buckets")
    cos = [float(torch.nn.functional.cosine_similarity(a.double().reshape(1, -1), k[:nprompt].double().reshape(1, -1))) for a, k in zip(k_cores, dec.kCache)]
    m["k_cache_cosine_buckets_vs_dense_cores"] = {"first_layer": cos[0], "last_layer": cos[-1], "min": min(cos), "mean": sum(cos) / len(cos)}
    m["buckets_over_cores_time"] = round(m["prefill_buckets_ms_per_prompt_token"] / m["prefill_cores_ms_per_prompt_token"], 3)
    before = torch.cuda.memory_allocated()
    for L in model.layers:
        for w in ("wq", "wk", "wv", "wo", "w1", "w2", "w3"):
            getattr(L, w).core = None
    gc.collect()
    torch.cuda.synchronize()
    m["model_memory_allocated_with_cores_GB"] = round(mem_with / 1e9, 3)
    m["model_memory_allocated_without_cores_GB"] = round((mem_with - (before - torch.cuda.memory_allocated())) / 1e9, 3)
    m["prefill_buckets_without_cores_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, weights="buckets")
    out["model"] = m
    res["prefill_buckets"] = out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r12_prefill_buckets.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del dec, model


def prefill_q4(b, res):
    """Prefill straight from the Q4 buckets (effort_q4_gemm_rows: the block multiply de-quantising on the fly, then the outlier pass)
    beside the core kernel and the FP16 bucket kernel MEASURED IN THE SAME RUN.  Kernel legs, prefill_buckets' protocol (rotating
    disjoint matrices, more than 768 MB of f16 cores per shape, one pass per graph, best of 3 windows): us per call at 16 and 64 rows
    on the decode loop's four shapes; the Q4 bundles are the converter's (2 % outliers), and the same buckets registered WITHOUT their
    outliers give the multiply alone.  (A Q4 matrix is a quarter of its core: the rotating Q4 set is that much smaller.)  Model legs,
    the reference's Q4 model at Mistral-7B shapes, a 256-token prompt: `Decoder.prefill` ms per prompt token with ``weights="cores"``
    and ``weights="q4"``; the cosine of the layer-0 and last-layer K caches of either prefill against those a token-by-token Q4 decode
    at effort 1.0 writes; ``torch.cuda.memory_allocated`` with and without the Q4 bundles' cores -- after which the prompt is prefilled
    once more."""
    import ctypes as C
    import gc

    import effort_amd
    from effort_amd.decode import Decoder, MistralConfig, Model
    from effort_amd.q4 import convert as q4_convert
    from effort_amd.weights import ExpertWeights
    torch = b.torch
    g, lib = b.g, effort_amd.lib()
    g.set_tuning(0, 0, 0)
    g.set_dense_backend(False)
    torch.cuda.empty_cache()
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    gen = torch.Generator(device=b.dev)
    gen.manual_seed(78)

    kern = {"protocol": "one pass over the rotating matrices per graph, 4 replays per window, best of 3 windows, device events; all kernels in this run; "
                        "a workgroup of the Q4 kernel owns 16 words of every bucket row (32 bytes, 512 outputs); q4 = multiply + outlier pass "
                        "(2 % outliers), q4_no_outliers = the same buckets registered without them"}
    for outD, inD in ((4096, 4096), (14336, 4096), (4096, 14336), (1024, 4096)):
        nbytes = outD * inD * 2
        count = max(4, -(-(768 << 20) // nbytes))
        cores = [(torch.randn((outD, inD), generator=gen, device=b.dev, dtype=torch.float32) * 0.02).to(torch.float16) for _ in range(count)]
        fp16 = [ExpertWeights.from_core(c) for c in cores]
        def q4_bundle(core):                                                     # from_core_q4; a matrix of fewer than 4096 outputs (wk, wv: never
            t = q4_convert(core.t().contiguous(), 0.02)                          # Q4 in the reference's model) gets its probes padded: prefill reads none
            probes = torch.zeros(4096, dtype=torch.float16, device=b.dev)
            probes[:t["probes"].numel()] = t["probes"]
            return ExpertWeights(t["buckets"], t["bucket.stats"], probes, inD, outD, outliers=t["outliers"], q4=True)
        q4 = [q4_bundle(c) for c in cores]
        bare =[ExpertWeights(e.buckets, e.stats, e.probes, inD, outD, None, 1, q4=True) for e in q4]
        for ew in fp16 + q4 + bare:
            ew.handle
        x = torch.randn((64, inD), generator=gen, device=b.dev, dtype=torch.float32)
        out = torch.zeros((64, outD), device=b.dev)

        def leg(kind, rows):
            def fn():
                g._bind_stream()
                for i in range(count):
                    if kind == "core":
                        g.check(lib.effort_dense_gemm_rows(g.ctx, p(cores[i]), p(x), p(out), inD, outD, rows), "dense_gemm_rows")
                    elif kind == "bucket":
                        g.check(lib.effort_bucket_gemm_rows(g.ctx, fp16[i].handle, 0, p(x), p(out), rows), "bucket_gemm_rows")
                    else:
                        g.check(lib.effort_q4_gemm_rows(g.ctx, (q4 if kind == "q4" else bare)[i].handle, 0, p(x), p(out), rows), "q4_gemm_rows")
            return fn
        row = {"matrices": count, "core_bytes": nbytes, "q4_bucket_bytes": nbytes // 4, "outliers": int(q4[0].outliers.shape[0])}
        for rows in (16, 64):
            for kind in ("core", "bucket", "q4", "q4_no_outliers"):
                row[f"{kind}_rows_{rows}"] = {"us_per_call": round(us_per_call(b, leg(kind, rows), count), 2)}
            for kind in ("bucket", "q4", "q4_no_outliers"):
                row[f"{kind}_over_core_time_{rows}"] = round(row[f"{kind}_rows_{rows}"]["us_per_call"] / row[f"core_rows_{rows}"]["us_per_call"], 3)
        kern[f"{inD}->{outD}"] = row
        del cores, fp16, q4, bare, x, out
        gc.collect()
        torch.cuda.empty_cache()
    out = {"kernel": kern}

    nprompt = 256
    model = Model.random(MistralConfig(), seed=1, q4=True)
    torch.cuda.synchronize()
    mem_with = torch.cuda.memory_allocated()
    dec = Decoder(model, maxTokens=nprompt + 8)
    B._GRAPHS_FOR_LIFE.append(dec._graphs)
    prompt = [int(t) for t in torch.randint(0, model.cfg.vocab, (nprompt,), generator=torch.Generator().manual_seed(3))]
    cosine = lambda a, k: float(torch.nn.functional.cosine_similarity(a.double().reshape(1, -1), k.double().reshape(1, -1)))      # noqa: E731
    ends = lambda: [dec.kCache[n][:nprompt].clone() for n in (0, len(dec.kCache) - 1)]                                               # noqa: E731

    m = {"model": "the reference's Q4 model (wq, w1, w2, w3 in Q4 with 2 % outliers; wk, wv, wo cores) at Mistral-7B shapes, 32 layers, random weights, seed 1",
         "prompt_tokens": nprompt,
         "protocol": "eager, synchronised wall time of Decoder.prefill(chunk=64) over the whole prompt, best of 3 after a warm call; the decode: the "
                     "prompt token by token through the captured step at effort 1.0"}
    m["prefill_cores_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, weights="cores")
    k_cores = ends()
    m["prefill_q4_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, weights="q4")
    k_q4 = ends()
    m["q4_over_cores_time"] = round(m["prefill_q4_ms_per_prompt_token"] / m["prefill_cores_ms_per_prompt_token"], 3)
    dec.run(prompt, nprompt, effort=1.0)
    torch.cuda.synchronize()
    k_dec = ends()
    m["k_cache_cosine_against_q4_decode_at_effort_1"] = {
        "q4_prefill": {"first_layer": cosine(k_q4[0], k_dec[0]), "last_layer": cosine(k_q4[1], k_dec[1])},
        "cores_prefill": {"first_layer": cosine(k_cores[0], k_dec[0]), "last_layer": cosine(k_cores[1], k_dec[1])}}
    before = torch.cuda.memory_allocated()
    for L in model.layers:
        for w in ("wq", "w1", "w2", "w3"):
            getattr(L, w).core = None
    gc.collect()
    torch.cuda.synchronize()
    m["model_memory_allocated_with_q4_cores_GB"] = round(mem_with / 1e9, 3)
    m["model_memory_allocated_without_q4_cores_GB"] = round((mem_with - (before - torch.cuda.memory_allocated())) / 1e9, 3)
    m["prefill_q4_without_q4_cores_ms_per_prompt_token"] = timed_prefill(b, dec, prompt, weights="q4")
    out["model"] = m
    res["prefill_q4"] = out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r13_prefill_q4.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    del dec, model


def prefill_attention(b, res):
    """Prefill attention: effort_attention_rows (every query of a block reads K / V again) beside effort_attention_block (the block's
    queries share each K / V tile), one process.  Kernel legs, decode_prefill's protocol: 32 heads, headDim 128, maxTokens 8192, a pass
    over four ROTATING cache pairs (1 GB: a pair is 268 MB, nothing of it is still cached when its turn comes again) captured into one
    graph, device events, best of 3 windows after a warm-up; us per call and the K / V bytes each kernel asks for.  Model legs,
    Mistral-7B shapes: `Decoder.prefill` over a 256-token and a 2048-token prompt at chunk 64 on both paths (synchronised wall time,
    best of 3 after a warm call); ms per prompt token."""
    import ctypes as C

    import effort_amd
    from effort_amd.decode import Decoder, MistralConfig, Model
    torch = b.torch
    g, lib = b.g, effort_amd.lib()
    g.set_tuning(0, 0, 0)
    g.set_dense_backend(False)
    torch.cuda.empty_cache()
    p = lambda t: C.c_void_p(t.data_ptr())                                       # noqa: E731
    gen = torch.Generator(device=b.dev)
    gen.manual_seed(78)
    heads, hd, maxTokens, pairs = 32, 128, 8192, 4

    rnd = lambda *shape: torch.randn(shape, generator=gen, device=b.dev, dtype=torch.float32)      # noqa: E731
    caches = [(rnd(maxTokens, heads, hd), rnd(maxTokens, heads, hd)) for _ in range(pairs)]
    q, out = rnd(64, heads * hd), torch.zeros((64, heads * hd), device=b.dev)
    rowBytes = heads * hd * 4 * 2                                                # K and V of one token, every head

    def leg(entry, what, pos0, rows):
        def fn():
            g._bind_stream()
            for kc, vc in caches:
                g.check(entry(g.ctx, p(q), p(kc), p(vc), pos0, rows, p(out), heads, hd, maxTokens), what)
        return fn
    kern = {"protocol": "one pass over 4 rotating cache pairs per graph, 4 replays per window, best of 3 windows, device events; "
                        "kv_bytes = cache rows each kernel asks for x 32 KB (K + V of a token, 32 heads)",
            "heads": heads, "headDim": hd, "maxTokens": maxTokens}
    for pos0, rows in ((0, 64), (192, 64), (960, 64), (4032, 64), (8128, 64), (4032, 16)):
        asked = {"attention_rows": sum(pos0 + r + 1 for r in range(rows)),
                 "attention_block": sum(min(pos0 + rows, ((pos0 + min(16 * t + 15, rows - 1)) // 16 + 1) * 16) for t in range((rows + 15) // 16))}
        row = {}
        for name, entry in (("attention_rows", lib.effort_attention_rows), ("attention_block", lib.effort_attention_block)):
            us = us_per_call(b, leg(entry, name, pos0, rows), pairs)
            row[name] = {"us_per_call": round(us, 2), "kv_bytes": asked[name] * rowBytes, "TBps_of_kv_bytes": round(asked[name] * rowBytes / us / 1e6, 3)}
        row["rows_over_block_time"] = round(row["attention_rows"]["us_per_call"] / row["attention_block"]["us_per_call"], 2)
        row["rows_over_block_bytes"] = round(asked["attention_rows"] / asked["attention_block"], 2)
        kern[f"pos0_{pos0}_rows_{rows}"] = row
    del caches, q, out
    torch.cuda.empty_cache()
    res_out = {"kernel": kern}

    model = Model.random(MistralConfig(), seed=1)
    m = {"model": "Mistral-7B shapes, 32 layers, random weights, seed 1", "chunk": 64,
         "protocol": "eager, synchronised wall time of Decoder.prefill over the whole prompt, best of 3 after a warm call"}
    for nprompt in (256, 2048):
        dec = Decoder(model, maxTokens=nprompt + 8)
        prompt = [int(t) for t in torch.randint(0, model.cfg.vocab, (nprompt,), generator=torch.Generator().manual_seed(3))]
        for attention in ("rows", "block", "rows"):                              # (the rows path twice: its own run-to-run spread)
            key = f"prompt_{nprompt}_{attention}_ms_per_prompt_token"
            m[key + "_again" if key in m else key] = timed_prefill(b, dec, prompt, chunk=64, attention=attention)
        m[f"prompt_{nprompt}_rows_over_block"] = round(m[f"prompt_{nprompt}_rows_ms_per_prompt_token"] / m[f"prompt_{nprompt}_block_ms_per_prompt_token"], 3)
        del dec
        torch.cuda.empty_cache()
    res_out["model"] = m
    res_out["acceptance"] = {
        "kernel_pos0_4032_rows_64_block_faster_by_more_than_5_percent": kern["pos0_4032_rows_64"]["rows_over_block_time"] > 1.05,
        "model_256_block_no_slower_than_rows_beyond_5_percent": m["prompt_256_rows_over_block"] >= 1.0 / 1.05}
    res["prefill_attention"] = res_out
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "r10_prefill_attention.json"), "w") as f:
        json.dump(res_out, f, indent=1)
        f.write("\n")
    del model


def layer_latency(b, res):
    """BASELINE config 4's latency case on ONE GPU: a world of one through RCCL + projected ranks."""
    b.torch.cuda.empty_cache()
    lg = b.ea.Gpu(b.local)
    lg.comm_create(0, 1, b.ea.Gpu.comm_unique_id())
    try:
        res["layer_latency"] = B.layer_latency(b.ea, lg, b.dev, 0, 1)
    finally:
        lg.comm_destroy()
        del lg


RUN = {"by_streams": by_streams, "shared_matrices": shared_matrices, "four_contexts": four_contexts, "timeit_protocol": timeit_full,
       "heavy_tailed_input": heavy_tailed_input, "sweep_structured": sweep_structured, "other_shapes": other_shapes,
       "shard_projection": shard_projection, "decode_quality": decode_quality, "layer_latency": layer_latency, "decode_q4": decode_q4,
       "decode_mixtral": decode_mixtral, "decode_sampled": decode_sampled, "decode_prefill": decode_prefill, "prefill_attention": prefill_attention,
       "prefill_mixtral": prefill_mixtral, "prefill_buckets": prefill_buckets, "prefill_q4": prefill_q4, "decode_rules": decode_rules}


class Light:
    """What the STANDALONE sections read of bench.Bench: torch, the package, the device and its default context."""

    def __init__(self):
        import effort_amd
        import torch
        self.torch, self.ea, self.dev = torch, effort_amd, "cuda:0"
        self.g = effort_amd.gpu()


def main():
    argv = sys.argv[1:]
    sections = list(SECTIONS)
    if "--sections" in argv:
        i = argv.index("--sections")
        sections = [s for s in argv[i + 1].split(",") if s]
        del argv[i:i + 2]
    args = B.parse_args(argv)
    import torch
    torch.cuda.set_device(0)
    if all(name in STANDALONE for name in sections):
        b = Light()
        res = {"what": "bench.py's auxiliary sections (tools/bench_extra.py)"}
    else:
        b = B.Bench(args)
        b.headline()                                              # (the sections price themselves against the headline's dispatch count)
        res = {"what": "bench.py's auxiliary sections (tools/bench_extra.py)", "headline_us_per_call": round(b.dt / B.N_MATS * 1e6, 3), "dispatch_rows": b.D}
    for name in sections:
        t0 = time.perf_counter()
        try:
            RUN[name](b, res)
        except Exception as ex:                                  # noqa: BLE001
            res[name] = {"error": repr(ex)[:400]}
        B.log(f"bench_extra: {name} {time.perf_counter() - t0:.1f} s")
    os.makedirs(os.path.join(ROOT, "gpurun_out"), exist_ok=True)
    with open(os.path.join(ROOT, "gpurun_out", "bench_extra.json"), "w") as f:
        json.dump(res, f)
        f.write("\n")
    print(json.dumps({k: (v if not isinstance(v, dict) or len(json.dumps(v)) < 300 else "...") for k, v in res.items()}), flush=True)
    sys.stderr.flush()
    os._exit(0)          # (bench.keep(): no captured graph is destroyed, at exit either)


if __name__ == "__main__":
    main()
