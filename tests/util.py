"""Shared synthetic-input helpers for the tests (SURVEY.md section 8d inputs)."""
import numpy as np


def make_w(outDim: int, inDim: int, seed: int = 1234, scale: float = 0.02, zeros: int = 0) -> np.ndarray:
    """HF-layout weight matrix f16 [outDim, inDim] ~ N(0, scale^2); optionally plant exact zeros."""
    rng = np.random.default_rng(seed)
    W = (rng.standard_normal((outDim, inDim), dtype=np.float32) * scale).astype(np.float16)
    if zeros:
        r = rng.integers(0, outDim, zeros)
        c = rng.integers(0, inDim, zeros)
        W[r, c] = 0
        W[r[: zeros // 2], c[: zeros // 2]] = np.float16(-0.0)
    return W


def make_v(inDim: int, seed: int = 42, heavy: bool = False) -> np.ndarray:
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(inDim, dtype=np.float32)
    if heavy:
        v = (v * np.exp(rng.standard_normal(inDim, dtype=np.float32))).astype(np.float32)
    return v


# ---- weight / input families that strain the multiply's fixed-point scale (tests/test_gpu_fixedpoint.py and its CPU twin) ----
def structured_w(outDim: int, inDim: int, seed: int = 1234, scale: float = 0.02) -> np.ndarray:
    """numpy restatement of effort_amd.decode.structured_matrix: heavy-tailed entries (a Gaussian times a log-normal, sigma 0.5), a
    log-normal scale per input channel (sigma 0.7) and per output (sigma 0.3), overall std = ``scale``; f16 [outDim, inDim]."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal((outDim, inDim))
    w *= np.exp(0.5 * rng.standard_normal((outDim, inDim)))
    w *= np.exp(0.7 * rng.standard_normal((1, inDim)))
    w *= np.exp(0.3 * rng.standard_normal((outDim, 1)))
    w *= scale / w.std()
    return w.astype(np.float16)


def structured_norm_w(n: int, seed: int = 1234) -> np.ndarray:
    """numpy restatement of effort_amd.decode.structured_norm_weights: log-normal spread (sigma 0.6), 0.5 % of the channels eight
    times larger, unit rms; f16 [n]."""
    rng = np.random.default_rng(seed)
    w = np.exp(0.6 * rng.standard_normal(n))
    w = np.where(rng.random(n) < 0.005, w * 8.0, w)
    return (w / np.sqrt((w * w).mean())).astype(np.float16)


FAMILY_CHANNEL = 1234          # the input channel (and, for `lone`, with FAMILY_ROW the one weight) that is made large
FAMILY_ROW = 77


def family_w(family: str, outDim: int, inDim: int, seed: int = 1234, mult: float = 1.0) -> np.ndarray:
    """f16 [outDim, inDim] of one family, times ``mult``: ``gauss`` (make_w), ``structured``, ``channel`` (gauss, input channel
    FAMILY_CHANNEL x1000), ``lone`` (gauss, the one weight [FAMILY_ROW, FAMILY_CHANNEL] at 3000 sigma), ``subnormal`` (gauss x 2^-12:
    nearly every f16 weight is subnormal), ``large`` (gauss x 2^10), ``flat`` (every weight +0.02: with a positive input an
    output is the sixteenth part of the multiply's bound L, as near to it as a matrix gets)."""
    if family == "structured":
        W = structured_w(outDim, inDim, seed).astype(np.float32)
    elif family == "flat":
        W = np.full((outDim, inDim), 0.02, np.float32)
    else:
        W = make_w(outDim, inDim, seed=seed).astype(np.float32)
        if family == "channel":
            W[:, FAMILY_CHANNEL] *= 1000.0
        elif family == "lone":
            W[FAMILY_ROW, FAMILY_CHANNEL] = np.float32(0.02 * 3000.0) * (1.0 if W[FAMILY_ROW, FAMILY_CHANNEL] >= 0 else -1.0)
        elif family in ("subnormal", "large"):
            W *= {"subnormal": 2.0 ** -12, "large": 2.0 ** 10}[family]
        else:
            assert family == "gauss", family
    return (W * np.float32(mult)).astype(np.float16)


def family_v(inDim: int, seed: int = 42, heavy: bool = False, zero_channel: bool = False, positive: bool = False) -> np.ndarray:
    v = make_v(inDim, seed=seed, heavy=heavy)
    if zero_channel:
        v[FAMILY_CHANNEL] = 0.0
    return np.abs(v) if positive else v


def cos(a, b) -> float:
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(a @ b / (np.linalg.norm(a) * np.linalg.norm(b)))
