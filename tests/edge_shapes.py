"""Synthetic weight bundles at the borders of what registration accepts, and the table of cases that run on them.
TEST INFRASTRUCTURE: numpy only (no torch, no project code), so that the GPU test (tests/test_gpu_edge_shapes.py) and the planner's
CPU test (tests/test_plan_domain_cpu.py) read ONE list.

Registration (csrc/weights.hip: check_bundle) takes any inDim in 4096 .. 65535, odd ones included, any outDim that is a multiple of 32 up to
16384, any percentLoad 1 .. 16, and any stack whose per-row arrays stay below 4 GiB.  The converters reach a small part of that
(effort_convert_fp16: 4096 % outDim == 0 or outDim >= 4096, inDim <= 32000), but the multiply does not care where a layout came from:
the bundles are built directly, as tests/test_gpu_parity.py::test_q4_outlier_tables builds its Q4 bundle.

  FP16  buckets  f16 N(0, 0.02^2) [percentLoad * inDim, outDim / 16], the low 4 bits random (the position inside the bucket: any
                 pattern is a valid layout)
        stats    f16 [rows, 4]: lane 3 = f16 of the f32 mean of |row| -- the only lane that is read; lanes 0 .. 2 hold 60000, which
                 would keep every row if a kernel read them
        probes   f16 N(0, 0.02^2) [4096]
  Q4    buckets  random u16 words [8 * inDim, outDim / 32];  stats f32 |N(0, 0.02)| in both lanes;  probes as above;
        outliers f32 [n, 4] = (an f16 value, input, output, 0)

The reference of a call (``reference``): the cutoff is oracle.cpu.find_cutoff's, the rows oracle.cpu.prepare_dispatch's -- asked for
with ONE column, so that the list's float row offsets are the row numbers themselves, exact below 2^24 rows -- and the product
tests/fixedpoint_reference.product_f64 over exactly those rows.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

from tests import fixedpoint_reference as fr

EFFORTS = (0.0, 0.02, 0.25, 1.0)
GROUP_EFFORTS = (0.25, 1.0, 0.02)            # a group of three on one input

# ---- the case tables -----------------------------------------------------------------------------------------------------------
# deep: also as a persistent group and with the rmsNorm prologue + residual
Fp16Case = namedtuple("Fp16Case", "name inDim outDim percentLoad deep reaches")
FP16_CASES = [
    Fp16Case("odd-2col", 4097, 32, 16, True, "odd inDim: the 8-byte stats path, odd row offsets; 2 columns"),
    Fp16Case("odd-6col", 4099, 96, 16, False, "6 columns: a tile with 6 of 64 lanes live"),
    Fp16Case("odd-widest", 4097, 16384, 16, True, "the widest row (1024 columns) with an odd inDim"),
    Fp16Case("ragged-top", 4096, 16352, 16, False, "a ragged last tile at the top of the range"),
    Fp16Case("largest-odd", 65535, 64, 16, True, "the largest inDim, odd; the largest row numbers"),
    Fp16Case("largest-even", 65534, 32, 16, False, "the largest even inDim: the compact means at the largest offsets"),
    Fp16Case("odd-load3", 16385, 160, 3, False, "odd inDim, truncated load, 10 columns"),
]
# outliers: None, or the name of a table of ``q4_outliers``; fused: also with the rmsNorm prologue
Q4Case = namedtuple("Q4Case", "name inDim outDim outliers fused reaches")
Q4_CASES = [
    Q4Case("q4-one-word", 4097, 32, "ends", False, "one word per row: rows 2 bytes long"),
    Q4Case("q4-three-words", 4099, 96, "ends", False, "three words per row: rows 6 bytes long"),
    Q4Case("q4-largest-odd", 65535, 64, "corners", False, "the 16-bit input field of the packed outlier entry: inputs 0 and 65534, outputs 0 and 63"),
    Q4Case("q4-lds-limit", 16384, 4096, "dense", True, "exactly the largest input the LDS copy of v takes, with outliers and the rmsNorm prologue"),
]
# one small case of each format for the effort boundaries and the refusals
BOUNDARY_FP16, BOUNDARY_Q4 = FP16_CASES[0], Q4_CASES[0]
BOUNDARY_KS = (1, 2048, 4094)                # effort = 1 - k / 4095 and the doubles either side of it
BAD_EFFORTS = (-1e-9, 1.0 + 1e-9, float("nan"), float("inf"))

# the stack next to 2^32: 31 experts of 4096 x 16384 at percentLoad 16 are 31 x 128 MiB of buckets; 32 is the first count refused
STACK = {"inDim": 4096, "outDim": 16384, "percentLoad": 16, "experts": 31}

# ---- the planner's domain (tests/test_plan_domain_cpu.py) ------------------------------------------------------------------------
PLAN_IN_DIMS = (4096, 4097, 4099, 4500, 8191, 16384, 16385, 32767, 65534, 65535)
PLAN_OUT_DIMS = (32, 64, 96, 160, 1024, 4096, 11008, 16352, 16384)
PLAN_LOADS = (1, 3, 15, 16)
PLAN_GROUPS = (1, 2, 3, 8, 9, 17, 32)
PLAN_ENVS = ((64, 1), (256, 1), (304, 1), (256, 4))                  # (CUs, lanes)
PLAN_TUNES = ((0, 0), (2, 4), (4, 0), (8, 0), (16, 0))              # (waves, columns per lane): W 2 exists at E 4 only


# ---- bundles -------------------------------------------------------------------------------------------------------------------
def _probes(rng) -> np.ndarray:
    return (rng.standard_normal(4096, dtype=np.float32) * np.float32(0.02)).astype(np.float16)


def fp16_bundle(inDim: int, outDim: int, percentLoad: int = 16, seed: int = 0) -> dict:
    """One expert's FP16 layout, in the form tests/test_fixedpoint_reference_cpu.py's helpers take (``q4``, ``inDim``, ``outDim``,
    ``percentLoad``, ``expertRows``, ``buckets`` u16 [rows, cols], ``stats`` f16 [rows, 4], ``probes`` f16 [4096])."""
    rng = np.random.default_rng([seed, inDim, outDim, percentLoad])
    rows, cols = percentLoad * inDim, outDim // 16
    w = (rng.standard_normal((rows, cols), dtype=np.float32) * np.float32(0.02)).astype(np.float16).view(np.uint16)
    w &= np.uint16(0xFFF0)
    w |= rng.integers(0, 16, size=(rows, cols), dtype=np.uint16)
    mean = np.abs(w.view(np.float16)).astype(np.float32).mean(axis=1, dtype=np.float32)
    stats = np.full((rows, 4), 60000.0, np.float16)
    stats[:, 3] = mean.astype(np.float16)
    return {"q4": False, "inDim": inDim, "outDim": outDim, "percentLoad": percentLoad, "expertRows": rows, "buckets": w, "stats": stats,
            "probes": _probes(rng)}


def q4_outliers(name: str, inDim: int, outDim: int, rng) -> np.ndarray:
    """f32 [n, 4] = (value, input, output, 0), the values those of an f16 matrix (q4_draft.py:58-67).
    ``ends``: entries on the first and the last output; ``corners``: a few hundred entries whose inputs include 0 and inDim - 1 and whose
    outputs include 0 and outDim - 1, every corner pair present, in shuffled order; ``dense``: 20000 entries all over the matrix with
    duplicates of one pair, on top of ``ends``."""
    def table(n, ins, outs):
        t = np.zeros((n, 4), np.float32)
        t[:, 0] = rng.normal(0, 0.3, size=n).astype(np.float16)
        t[:, 1] = ins
        t[:, 2] = outs
        return t
    ends = np.concatenate([table(300, rng.integers(0, inDim, size=300), 0), table(300, rng.integers(0, inDim, size=300), outDim - 1)])
    if name == "ends":
        return ends
    if name == "corners":
        corner = table(4, [0, 0, inDim - 1, inDim - 1], [0, outDim - 1, 0, outDim - 1])
        t = np.concatenate([corner, table(400, rng.integers(0, inDim, size=400), rng.integers(0, outDim, size=400)),
                            table(50, inDim - 1, rng.integers(0, outDim, size=50)), table(50, 0, rng.integers(0, outDim, size=50))])
        return t[rng.permutation(t.shape[0])]
    assert name == "dense", name
    dup = np.repeat(table(8, rng.integers(0, inDim, size=8), rng.integers(0, outDim, size=8)), 7, axis=0)
    return np.concatenate([ends, dup, table(20000, rng.integers(0, inDim, size=20000), rng.integers(0, outDim, size=20000))])


def q4_bundle(inDim: int, outDim: int, outliers: str | None = None, seed: int = 0) -> dict:
    rng = np.random.default_rng([seed, inDim, outDim, 4])
    rows, cols = inDim * 8, outDim // 32
    buckets = rng.integers(0, 65536, size=(rows, cols), dtype=np.uint16)
    mean = np.abs(rng.normal(0, 0.02, size=rows)).astype(np.float32)
    return {"q4": True, "inDim": inDim, "outDim": outDim, "percentLoad": 8, "expertRows": rows, "buckets": buckets,
            "stats": np.stack([mean, mean], axis=1), "probes": _probes(rng),
            "outliers": None if outliers is None else q4_outliers(outliers, inDim, outDim, rng)}


def bundle(case) -> dict:
    if isinstance(case, Fp16Case):
        return fp16_bundle(case.inDim, case.outDim, case.percentLoad)
    return q4_bundle(case.inDim, case.outDim, case.outliers)


# ---- the reference of one call -------------------------------------------------------------------------------------------------
def oracle_takes(lay: dict) -> bool:
    """The oracle's FULL call asserts the reference's (outDim / 16) % 4 == 0 (bucketMul.swift:76)."""
    return (lay["outDim"] // 16) % 4 == 0


def reference(oracle, lay: dict, v, effort: float) -> dict:
    """``count``, ``cutoff`` (the oracle's, exact), ``rows`` and ``want`` (float64 [outDim]: product_f64 over those rows, Q4 with the
    outlier table) of one call on expert 0 of ``lay``; ``full``: the oracle's own product where its full call takes the shape."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    inDim, outDim = lay["inDim"], lay["outDim"]
    cutoff, _ = oracle.find_cutoff(v, lay["probes"], 0, effort)
    if lay["q4"]:
        disp, n = oracle.prepare_dispatch_q4(v, lay["stats"], 0, cutoff, inDim, 1)
        want = fr.product_f64(v, lay["buckets"], disp[:n, 1].astype(np.int64), outDim, stats=lay["stats"], outliers=lay["outliers"],
                              expertRows=lay["expertRows"])
    else:
        disp, n = oracle.prepare_dispatch(v, lay["stats"], 0, cutoff, inDim, 1, lay["percentLoad"])
        want = fr.product_f64(v, lay["buckets"], disp[:n, 1].astype(np.int64), outDim, expertRows=lay["expertRows"])
    assert lay["expertRows"] < 2 ** 24                                   # (the row numbers came through f32)
    rows = disp[:n, 1].astype(np.int64)
    assert n == 0 or (np.diff(rows) > 0).all()
    ref = {"count": n, "cutoff": cutoff, "rows": rows, "want": want, "full": None}
    if oracle_takes(lay):
        if lay["q4"]:
            full, n2, c2 = oracle.bucket_mul_q4(v, lay["buckets"], lay["stats"], lay["probes"], lay["outliers"], inDim, outDim, effort)
        else:
            full, n2, c2 = oracle.bucket_mul(v, lay["buckets"], lay["stats"], lay["probes"], inDim, outDim, effort, percentLoad=lay["percentLoad"])
        assert (n2, np.float32(c2).tobytes()) == (n, np.float32(cutoff).tobytes())
        ref["full"] = full
    return ref


def boundary_efforts():
    """[(k, effort)] for the k of BOUNDARY_KS: 1 - k / 4095 and the doubles either side of it -- where 1 - effort rounds, all three may
    land on one q -- and, so that both sides of the step are there whatever the rounding, 1 - (k -+ 1e-6) / 4095: q = k - 1 and q = k."""
    out = []
    for k in BOUNDARY_KS:
        e = 1.0 - k / 4095.0
        out += [(k, float(np.nextafter(e, -np.inf))), (k, e), (k, float(np.nextafter(e, np.inf))),
                (k, 1.0 - (k - 1e-6) / 4095.0), (k, 1.0 - (k + 1e-6) / 4095.0)]
    return out
