"""Every instantiation of the multiply kernel, in every mode it serves, against the CPU oracle (tests/variant_scenarios.py is the table;
tests/test_variants_cpu.py proves on any machine that the table covers the hook's rows).

Each launch states which kernel it ran (Gpu.last_variant) and that must be the prediction.  Every call's dispatch count and cutoff bits
are the oracle's; under a prologue the oracle is fed the input the glue kernels materialise (effort_silu_mul / effort_add_rmsnorm_mul,
pinned to float64 in tests/test_gpu_glue.py).  Outputs sit between guard bands, are prefilled with NaN (or, in place, with the residual)
and pass the project's bar, tests/test_gpu_parity.py close(): 2e-5 of max|want|, cosine >= 0.999999.  Launches repeat bit for bit.

(a) the census: one scenario per (variant, mode);
(b) a cached cutoff under a prologue: one call with more items than workgroups, so a persistent workgroup works a second item of a
    call it has already cut -- mul_item's `else if (fused)` branch, the `!needCut` operand loads, Q4's early LDS copy of the transformed
    input -- three launches in a row, and against the plain grid of the same call: equal bits for FP16 and for Q4 without outliers;
(c) a mixed persistent group of four shapes: prologues, plain, routed experts and a truncated load (FP16), a ragged inDim, efforts 0 and 1; with a
    fifth shape (two launches); with residuals alone (cutoff jobs stay on); and replayed from one captured graph on changed inputs.
"""
import numpy as np
import pytest
import torch

from tests import variant_scenarios as vs
from tests.test_gpu_parity import DEV, close, converted, dev16, devf, gpu_weights
from tests.test_gpu_q4_fused import bundle, layout, norm_weights, rmsnorm, silu
from tests.util import make_v

pytestmark = pytest.mark.gpu

GUARD = 64                      # floats either side of every output
GUARD_VALUE = -555.0
_BANK, _WANT = {}, {}


@pytest.fixture(scope="module")
def ea(hip_lib_built):
    import effort_amd
    assert torch.cuda.is_available()
    effort_amd.gpu(0)
    return effort_amd


def num_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------- weights: (bundle, oracle(v, effort, expert) -> (want, rows, cutoff))
def weights(ea, oracle_cpu, q4, c):
    key = (q4, c["inDim"], c["outDim"], c["load"], c["expert"] is not None, c["outliers"])
    if key in _BANK:
        return key, _BANK[key]
    inDim, outDim = c["inDim"], c["outDim"]
    if not q4:
        if c["expert"] is not None:                 # three experts scaled x1, x1/64, x64 (test_experts_and_percentload's stack)
            mats = [converted(oracle_cpu, outDim, inDim, seed=100 + e, scale=0.02 * m) for e, m in enumerate((1.0, 1.0 / 64.0, 64.0))]
            ew = ea.ExpertWeights.stack([gpu_weights(ea, *m) for m in mats])
            B, S, P = (np.concatenate([m[k] for m in mats]) for k in (1, 2, 3))
            load = 16
        else:
            W, b, s, p = converted(oracle_cpu, outDim, inDim, seed=200 if inDim == vs.RAGGED_FP16 else 1234)
            load = c["load"]
            B, S, P = b[:inDim * load], s[:inDim * load], p
            ew = gpu_weights(ea, W, B, S, P, percentLoad=load)
        fn = lambda v, effort, e: oracle_cpu.bucket_mul(v, B, S, P, inDim, outDim, effort, expNo=e, percentLoad=load)      # noqa: E731
    elif c["outliers"]:                             # a converted Gaussian matrix with its outlier table (tests/test_gpu_q4_fused.py)
        L = layout(ea, inDim, outDim)
        ew = bundle(ea, L, inDim, outDim, True)
        fn = lambda v, effort, e: oracle_cpu.bucket_mul_q4(v, L["buckets"], L["bucket.stats"], L["probes"].view(np.float16), L["outliers"], inDim, outDim, effort)      # noqa: E731
    else:                                           # a synthetic Q4 bundle: any nibble pattern is a valid bucket word (test_q4_outlier_tables)
        assert c["expert"] is None                  # (the reference's Q4 path cannot route: variant_scenarios.mixed)
        rng = np.random.default_rng(inDim + outDim)
        rows, cols = inDim * 8, outDim // 32
        buckets = rng.integers(0, 65536, size=(rows, cols), dtype=np.uint16)
        mean = np.abs(rng.normal(0, 0.02, size=rows)).astype(np.float32)
        stats = np.stack([mean, mean], axis=1)
        probes = rng.normal(0, 0.02, size=4096).astype(np.float16)
        ew = ea.ExpertWeights(dev16(buckets), devf(stats), dev16(probes), inSize=inDim, outSize=outDim, q4=True)
        fn = lambda v, effort, e: oracle_cpu.bucket_mul_q4(v, buckets, stats, probes, None, inDim, outDim, effort)      # noqa: E731
    _BANK[key] = (ew, fn)
    return key, _BANK[key]


# ---------------------------------------------------------------- one call on the device, and what it must give
def host_inputs(c, rep):
    """The call's raw input, gate partner and residual for replay `rep` (rep > 0: other values at another scale)."""
    seed = 1000 + 97 * rep + c["seed"]
    mult = np.float32(1.0 + rep)
    return (make_v(c["inDim"], seed=seed, heavy=bool(c["seed"] & 1)) * mult, make_v(c["inDim"], seed=seed + 5000, heavy=True),
            make_v(c["outDim"], seed=seed + 9000) * mult)


def prepare(ea, oracle_cpu, s):
    """Device tensors of every call of the scenario (allocated once: a captured graph keeps their addresses)."""
    out = []
    for c in s["calls"]:
        wkey, (ew, fn) = weights(ea, oracle_cpu, s["q4"], c)
        buf = torch.empty(c["outDim"] + 2 * GUARD, device=DEV)
        st = {"c": c, "wkey": wkey, "ew": ew, "fn": fn, "buf": buf, "out": buf[GUARD:GUARD + c["outDim"]], "v": torch.empty(c["inDim"], device=DEV),
              "expNo": None if c["expert"] is None else torch.tensor([c["expert"]], dtype=torch.int32, device=DEV), "extras": {}}
        if c["pre"] == "gate":
            st["extras"]["gate"] = st["x3"] = torch.empty(c["inDim"], device=DEV)
        if c["pre"] == "norm":
            st["extras"]["norm"] = norm_weights(c["inDim"])
        if c["resid"]:                              # the gate's residual is the output itself (in place); the others' a vector of its own
            st["resid"] = st["out"] if c["pre"] == "gate" else torch.empty(c["outDim"], device=DEV)
            st["extras"]["resid"] = st["resid"]
        out.append(st)
    set_inputs(ea, oracle_cpu, s, out, 0)
    return out


def set_inputs(ea, oracle_cpu, s, states, rep):
    """Write replay `rep`'s inputs into the calls' tensors IN PLACE and work out what each call must give: the oracle on the
    materialised input (+ the residual)."""
    for st in states:
        c = st["c"]
        v, x3, resid = host_inputs(c, rep)
        st["v"].copy_(devf(v))
        if c["pre"] == "gate":
            st["x3"].copy_(devf(x3))
        st["resid_host"] = resid if c["resid"] else None
        if c["resid"] and st["resid"] is not st["out"]:
            st["resid"].copy_(devf(resid))
        key = (st["wkey"], c["expert"], c["seed"], rep, c["pre"], c["effort"])
        if key not in _WANT:
            vin = st["v"] if c["pre"] == "none" else silu(ea, st["v"], st["x3"]) if c["pre"] == "gate" else rmsnorm(ea, st["v"], st["extras"]["norm"])
            ea.gpu().eval()
            _WANT[key] = st["fn"](vin.cpu().numpy(), c["effort"], c["expert"] or 0)
        want, st["rows"], st["cutoff"] = _WANT[key]
        st["want"] = want if st["resid_host"] is None else st["resid_host"] + want


def refill(states):
    for st in states:
        st["buf"].fill_(GUARD_VALUE)
        if st["c"]["resid"] and st["resid"] is st["out"]:
            st["out"].copy_(devf(st["resid_host"]))
        else:
            st["out"].fill_(float("nan"))


def launch(ea, states):
    refill(states)
    ea.bucketMulGroup([(st["v"], st["ew"], st["expNo"], st["out"], st["c"]["effort"], st["extras"]) for st in states])
    ea.gpu().eval()


def check(g, states, tag):
    """Selection exact, outputs within the bar, guard bands untouched.  Returns the outputs."""
    outs = []
    for i, st in enumerate(states):
        rows, cutoff = g.last_dispatch_count(i), g.last_cutoff(i)
        whole = st["buf"].cpu().numpy()
        got = whole[GUARD:-GUARD].copy()
        scale = float(np.abs(st["want"]).max())
        print(f"{tag} call {i} {st['c']['pre']}{'+resid' if st['c']['resid'] else ''}: rows {rows} (oracle {st['rows']}) cutoff {cutoff!r} (oracle {st['cutoff']!r}) "
              f"max|got - want| / max|want| = {float(np.abs(got - st['want']).max()) / scale if scale else 0.0:.3e}")
        assert rows == st["rows"], (tag, i, rows, st["rows"])
        assert np.float32(cutoff).tobytes() == np.float32(st["cutoff"]).tobytes(), (tag, i, cutoff, st["cutoff"])
        assert (whole[:GUARD] == GUARD_VALUE).all() and (whole[-GUARD:] == GUARD_VALUE).all(), (tag, i)
        assert np.isfinite(got).all() and close(got, st["want"]), (tag, i)
        outs.append(got)
    return outs


def same_bits(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def ran(g, launches):
    return [g.last_variant(l) for l in range(launches)]


def predicted(s, numCU):
    from effort_amd import runtime
    rows, kw = vs.plan_args(s, numCU)
    plan = runtime.plan(rows, **kw)                 # (the planner refusing a scenario raises: a failure, not a skip)
    return plan, [{k: p[k] for k in ("variant", "persistent", "grid", "totalItems")} for p in vs.predict(s, plan, numCU)]


class tuned:
    """The scenario's tuning and persistent setting on the shared context, put back afterwards."""
    def __init__(self, g, s, persistent=None):
        self.g, self.args = g, (s["tuning"], s["persistent"] if persistent is None else persistent)

    def __enter__(self):
        self.g.set_tuning(*self.args[0])
        self.g.set_persistent(self.args[1])

    def __exit__(self, *exc):
        self.g.set_tuning(0, 0, 0)
        self.g.set_persistent(-1)


def by_name(table, name):
    (s,) = [s for s in table if s["name"] == name]
    return s


# ---------------------------------------------------------------- (a) every variant, every mode it serves
@pytest.mark.parametrize("name", [s["name"] for s in vs.census(256)])
def test_census_scenario_runs_its_variant_and_matches_the_oracle(ea, oracle_cpu, name):
    numCU = num_cu()
    s = by_name(vs.census(numCU), name)
    g = ea.gpu()
    plan, want = predicted(s, numCU)
    assert len(want) == 1
    states = prepare(ea, oracle_cpu, s)
    with tuned(g, s):
        launch(ea, states)
        assert ran(g, 1) == want, name
        first = check(g, states, name)
        launch(ea, states)
        assert ran(g, 1) == want and same_bits(check(g, states, name + " again"), first), name


# ---------------------------------------------------------------- (b) a cached cutoff under a prologue
@pytest.mark.parametrize("name", [s["name"] for s in vs.cached_cutoff(256)])
def test_cached_cutoff_under_a_prologue(ea, oracle_cpu, name):
    numCU = num_cu()
    s = by_name(vs.cached_cutoff(numCU), name)
    g = ea.gpu()
    plan, want = predicted(s, numCU)
    R = s["persistent"]
    assert vs.real_items(s, plan) > numCU * R and want[0]["grid"] == numCU * R and want[0]["persistent"] == R      # a workgroup works two items of the call
    states = prepare(ea, oracle_cpu, s)
    runs = []
    with tuned(g, s):
        for k in range(3):                          # the queues rewind between launches
            launch(ea, states)
            assert ran(g, 1) == want, (name, k)
            runs.append(check(g, states, f"{name} launch {k}"))
    assert same_bits(runs[1], runs[0]) and same_bits(runs[2], runs[0]), name
    with tuned(g, s, persistent=0):                 # the same call at the same tuning as a plain grid: every workgroup cuts for itself
        launch(ea, states)
        lv = g.last_variant(0)
        assert lv["persistent"] == 0 and lv["grid"] == lv["totalItems"] == want[0]["totalItems"] and lv["variant"][:3] == want[0]["variant"][:3], (name, lv)
        plain = check(g, states, name + " plain grid")
    if s["calls"][0]["outliers"]:                   # the outlier sums are f32 adds whose split follows the instantiation
        assert close(runs[0][0], plain[0]), name
    else:                                           # integer accumulation, the same geometry: the same bits
        assert same_bits(runs[0], plain), name


# ---------------------------------------------------------------- (c) a mixed persistent group
@pytest.mark.parametrize("q4", [False, True], ids=["fp16", "q4"])
def test_mixed_persistent_group(ea, oracle_cpu, q4):
    numCU = num_cu()
    g = ea.gpu()
    for s in (vs.mixed(q4), vs.mixed(q4, resid_only=True), vs.mixed(q4, fifth=True)):
        plan, want = predicted(s, numCU)
        launches = 2 if s["name"].endswith("five shapes") else 1
        assert len(want) == launches and plan["launch"] == [0] * 9 + [1] * (launches - 1), (s["name"], plan["launch"])
        assert want[0]["persistent"] == 1 and want[0]["variant"] == (8, 1, True, False, False), s["name"]
        assert (plan["cutJobs"][0] > 0) == s["name"].endswith("resid only"), (s["name"], plan["cutJobs"])
        states = prepare(ea, oracle_cpu, s)
        with tuned(g, s):
            launch(ea, states)
            assert ran(g, launches) == want, s["name"]
            first = check(g, states, s["name"])
            launch(ea, states)
            assert same_bits(check(g, states, s["name"] + " again"), first), s["name"]


@pytest.mark.parametrize("q4", [False, True], ids=["fp16", "q4"])
def test_mixed_persistent_group_under_graph_replay(ea, oracle_cpu, q4):
    """The mixed group replayed from ONE captured graph with the inputs changed in place between the replays: every replay sees the
    cutoffs, the prologues and the residuals of ITS inputs (as test_cutoff_jobs_under_graph_replay does for plain calls)."""
    numCU = num_cu()
    g = ea.gpu()
    s = vs.mixed(q4)
    _, want = predicted(s, numCU)
    states = prepare(ea, oracle_cpu, s)
    calls = [(st["v"], st["ew"], st["expNo"], st["out"], st["c"]["effort"], st["extras"]) for st in states]
    with tuned(g, s):
        launch(ea, states)                          # warm
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            ea.bucketMulGroup(calls)
        g._bind_stream()
        assert ran(g, 1) == want
    for rep in (1, 2):
        set_inputs(ea, oracle_cpu, s, states, rep)
        refill(states)
        torch.cuda.synchronize()
        graph.replay()
        g.eval()
        check(g, states, f"{s['name']} replay {rep}")
