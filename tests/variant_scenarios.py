"""The launches that pin every instantiation of the multiply kernel (csrc/bucket_mul.hip: EFFORT_GEOMS x each_variant) in every mode it
serves, as data: pure Python, no torch, no GPU.  tests/test_variants_cpu.py checks the table against the planner hook and the variant
hook on any machine; tests/test_gpu_variants.py runs it on the device.

A *variant* is (W, E, fused, compact, lean) as ``runtime.variants`` and ``Gpu.last_variant`` report it; a *mode* is "plain" (one workgroup
per item) or "persistent" (numCU * R workgroups pulling items from the queues).  Which modes an instantiation serves (``modes_served``):

  lean rows (W = 8 only)            plain: launch_mul_t runs them for plain grids and for nothing else
  generic rows, W = 8               persistent: the shipped library's plain grids at W = 8 are all lean
  generic compact rows, W != 8      persistent: the planner sets the compact bit for lean grids and persistent launches only
  other generic rows                plain and persistent

A *call* is a dict: inDim, outDim, effort, load (percentLoad), pre ("none" | "gate" | "norm"), resid (bool), expert (None, or the device
expNo into a stack of three experts scaled x1, x1/64, x64; FP16 only), outliers (Q4: the bundle carries an outlier table), seed (of its input).
A *scenario* is a dict: name, kind, q4, calls, tuning (W, E, S as effort_set_tuning takes them), persistent (effort_set_persistent).
"""

GEOMS = [(16, 1), (16, 2), (16, 4), (8, 1), (8, 2), (8, 4), (4, 1), (4, 2), (4, 4), (2, 4)]      # EFFORT_GEOMS
SIDE_GEOMS = [(8, 1), (16, 1), (4, 2), (2, 4)]              # where the prologues other than `norm` run their cached-cutoff cases
PRE_CODE = {"none": 0, "gate": 1, "norm": 2}                # EFFORT_PRE_*
EFFORTS = (0.25, 0.1, 0.5, 1.0)
RAGGED_FP16 = 4500                                          # tests/test_gpu_parity.py::test_ragged_input_dimension
RAGGED_Q4 = (14336, 4096)                                   # tests/test_gpu_q4_fused.py SHAPES[1]: no slice count of the tables divides it into powers of two
# the four prologue cases of a cached cutoff, and the mix the census's fused groups cycle through
PROLOGUES = {"norm": ("norm", False), "gate": ("gate", False), "gate+resid": ("gate", True), "norm+resid": ("norm", True)}


def call(inDim, outDim, effort, *, load=None, pre="none", resid=False, expert=None, outliers=False, seed=0, q4=False):
    return {"inDim": inDim, "outDim": outDim, "effort": effort, "load": (8 if q4 else 16) if load is None else load, "pre": pre, "resid": bool(resid),
            "expert": expert, "outliers": bool(outliers), "seed": seed}


def scenario(name, kind, q4, calls, tuning, persistent):
    return {"name": name, "kind": kind, "q4": bool(q4), "calls": list(calls), "tuning": tuple(tuning), "persistent": int(persistent)}


def plan_args(s, numCU):
    """(calls, keywords) for ``runtime.plan``.  (The hook plans every handle as one expert: a stack differs from a lone matrix in
    MulGeom::numExperts only, so the tables below never put a stack and a lone matrix of the same shape and load into one group.)"""
    rows = [(c["inDim"], c["outDim"], c["effort"], c["load"], PRE_CODE[c["pre"]], int(c["resid"])) for c in s["calls"]]
    W, E, S = s["tuning"]
    return rows, dict(q4=s["q4"], numCU=numCU, persistent=s["persistent"], waves=W, elems=E, slices=S)


def predict(s, plan, numCU):
    """What each launch of the scenario must run, from its ``runtime.plan`` result -- launch_mul_t's selection restated: fused when a
    call of the launch has a prologue or a residual, compact as planned, lean for a plain grid of 8-wave workgroups.  Per launch a dict
    shaped like ``Gpu.last_variant``'s plus ``mode``."""
    out = []
    for l in range(len(plan["persistent"])):
        members = [i for i, k in enumerate(plan["launch"]) if k == l]
        fused = any(s["calls"][i]["pre"] != "none" or s["calls"][i]["resid"] for i in members)
        R = plan["persistent"][l]
        items = sum((plan["tiles"][i] * plan["slices"][i] + 7) // 8 * 8 for i in members)
        out.append({"variant": (plan["W"], plan["E"], fused, bool(plan["compact"][l]), plan["W"] == 8 and R == 0),
                    "mode": "persistent" if R else "plain", "persistent": R, "grid": numCU * R if R else items, "totalItems": items})
    return out


def modes_served(variant):
    W, E, fused, compact, lean = variant
    if lean:
        return ("plain",)
    if W == 8 or compact:
        return ("persistent",)
    return ("plain", "persistent")


def real_items(s, plan, i=0):
    return plan["tiles"][i] * plan["slices"][i]


# ---------------------------------------------------------------- (a) the census: every variant, every mode it serves
def _fused_mix(n, inDim, outDim, q4):
    kinds = list(PROLOGUES.values())
    return [call(inDim, outDim, EFFORTS[i % 4], pre=kinds[i % 4][0], resid=kinds[i % 4][1], seed=20 + i, q4=q4) for i in range(n)]


def _enough(numCU, slices, R=1):
    """Calls of one tile x `slices` items each that outnumber numCU * R workgroups (at least 8: a group that takes cutoff jobs)."""
    return max(8, numCU * R // slices + 1)


def census(numCU=256):
    out = []
    for q4 in (False, True):
        f = "q4" if q4 else "fp16"
        for W, E in GEOMS:
            g = f"{f} W{W} E{E}"
            # plain grids of one call: 4096 -> 1024 at 32 slices (128 rows: the most a 2-wave FP16 workgroup stages).  W = 8: the lean
            # kernels, FP16 with compact means (even slices); elsewhere the generic kernel as a plain grid
            out.append(scenario(f"{g} plain", "census", q4, [call(4096, 1024, 0.25, seed=1, q4=q4)], (W, E, 32), 0))
            out.append(scenario(f"{g} plain fused", "census", q4, [call(4096, 1024, 0.5, pre="norm", seed=2, q4=q4),
                                                                  call(4096, 1024, 0.25, pre="gate", resid=True, seed=3, q4=q4)], (W, E, 32), 0))
            if not q4 and W == 8:
                # 4500 inputs at 36 slices: 125 rows per slice, an odd count -- no compact means -- and a ragged last slice
                out.append(scenario(f"{g} plain odd", "census", q4, [call(RAGGED_FP16, 256, 0.25, seed=4)], (W, E, 36), 0))
                out.append(scenario(f"{g} plain odd fused", "census", q4, [call(RAGGED_FP16, 256, 0.5, pre="norm", seed=5),
                                                                          call(RAGGED_FP16, 256, 0.25, pre="gate", resid=True, seed=6)], (W, E, 36), 0))
            # persistent launches, R = 1: calls of 4096 -> 256 (one tile) at 64 slices
            n = _enough(numCU, 64)
            out.append(scenario(f"{g} persistent", "census", q4, [call(4096, 256, EFFORTS[i % 4], seed=10 + i, q4=q4) for i in range(n)], (W, E, 64), 1))
            out.append(scenario(f"{g} persistent fused", "census", q4, _fused_mix(n, 4096, 256, q4), (W, E, 64), 1))
            if not q4:
                n = _enough(numCU, 36)
                out.append(scenario(f"{g} persistent odd", "census", q4, [call(RAGGED_FP16, 256, EFFORTS[i % 4], seed=40 + i) for i in range(n)], (W, E, 36), 1))
    return out


# ---------------------------------------------------------------- (b) a cached cutoff under a prologue
# format cases: (name, q4, inDim, outDim, outliers)
CACHED_FORMATS = [("fp16", False, 4096, 1024, False), ("q4", True, 4096, 1024, False),
                  ("q4 outliers 4096", True, 4096, 4096, True),                     # the early LDS copy of the transformed input (olEarly)
                  ("q4 outliers 14336", True, RAGGED_Q4[0], RAGGED_Q4[1], True)]    # the late copy (4096 < inDim <= 16384)


def cached_cutoff(numCU=256):
    """ONE call per launch with more items than the launch has workgroups: some workgroup works two items of the call, the second
    with the cutoff it cached.  `norm` at every geometry, the other prologues at SIDE_GEOMS; R = 1 and 2."""
    out = []
    for fname, q4, inDim, outDim, outliers in CACHED_FORMATS:
        cols = outDim // (32 if q4 else 16)
        for pname, (pre, resid) in PROLOGUES.items():
            for W, E in (GEOMS if pname == "norm" else SIDE_GEOMS):
                tiles = (cols + 64 * E - 1) // (64 * E)
                for R in (1, 2):
                    S = next(S for S in (512, 1024, 2048) if tiles * S > numCU * R)
                    c = call(inDim, outDim, 0.25, pre=pre, resid=resid, outliers=outliers, seed=7, q4=q4)
                    out.append(scenario(f"{fname} W{W} E{E} {pname} R{R}", "cached", q4, [c], (W, E, S), R))
    return out


# ---------------------------------------------------------------- (c) a mixed persistent group
def mixed(q4, fifth=False, resid_only=False):
    """Four shapes (kMaxGeoms) in one persistent launch: prologues, a plain call, two routed experts and a truncated load (FP16; Q4: two
    tables of outliers), a ragged inDim, efforts 0 and 1.  ``fifth``: one more shape, which opens a second launch.  ``resid_only``: the prologues dropped and every
    call given a residual -- a fused launch that keeps its cutoff jobs."""
    big = (4096, 1024)
    # (Q4 has no stacks to route into: prepareDispatchQ4 reads v[i / 8] with the expert's offset still in i, bucketMulQ4.metal:46 -- past the
    #  input for every expert but the first -- and no Q4 model with experts can be made; its two calls of that shape go to a lone matrix)
    routed = (None, None) if q4 else (1, 2)
    calls = [call(*big, 0.25, pre="norm", seed=61, q4=q4), call(*big, 0.5, pre="gate", resid=True, seed=62, q4=q4), call(*big, 0.25, seed=63, q4=q4),
             call(4096, 256, 0.4, expert=routed[0], seed=64, q4=q4), call(4096, 256, 0.4, expert=routed[1], seed=65, q4=q4)]
    if q4:
        calls += [call(4096, 4096, 0.25, outliers=True, seed=66, q4=True), call(*RAGGED_Q4, 0.25, outliers=True, seed=67, q4=True)]
    else:
        calls += [call(4096, 256, 0.6, load=3, seed=66), call(RAGGED_FP16, 256, 0.3, seed=67)]
    calls += [call(*big, 0.0, seed=68, q4=q4), call(*big, 1.0, seed=69, q4=q4)]
    if fifth:
        calls.append(call(4096, 512, 0.25, seed=70, q4=True) if q4 else call(4096, 256, 0.25, load=8, seed=70))
    if resid_only:
        calls = [dict(c, pre="none", resid=True) for c in calls]
    name = f"{'q4' if q4 else 'fp16'} mixed" + (" five shapes" if fifth else "") + (" resid only" if resid_only else "")
    return scenario(name, "mixed", q4, calls, (8, 1, 64), 1)


def table(numCU=256):
    return census(numCU) + cached_cutoff(numCU) + [mixed(q4, fifth, ro) for q4 in (False, True) for fifth, ro in ((False, False), (True, False), (False, True))]
