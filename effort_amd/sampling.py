"""Sampled decode: the settings of ``effort_sample`` (csrc/sample.hip) and its specification restated on the host.

The pick runs on the device inside the captured token step; its settings live in a 32-byte struct in device memory
(``effort_sample_params``, include/effort_hip.h), so changing the temperature or the seed rewrites that tensor and the graph is reused.
``philox_u`` and ``sample_reference`` restate the generator and the draw in plain Python integers and numpy float64: what the kernel is
tested against, and what a caller can use to reproduce a run from its seed.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass

import numpy as np

MAX_K = 64                                       # EFFORT_SAMPLE_MAX_K
_M32 = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): four 32-bit counter words, two key words -> four output words."""
    c0, c1, c2, c3 = (int(x) & _M32 for x in counter)
    k0, k1 = (int(x) & _M32 for x in key)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & _M32, (p0 >> 32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0, c1, c2, c3


def philox_bits(seed: int, stream: int, pos: int) -> int:
    """Output word 0 at counter (pos, stream, 0, 0) under key (seed & 0xFFFFFFFF, seed >> 32): effort_sample_bits."""
    return philox4x32_10((pos, stream, 0, 0), (seed & _M32, (seed >> 32) & _M32))[0]


def philox_u(seed: int, stream: int, pos: int) -> float:
    """The uniform of the draw at ``pos``: (x0 >> 8) * 2^-24, in [0, 1)."""
    return (philox_bits(seed, stream, pos) >> 8) * 2.0 ** -24


def philox_bits_many(seed: int, stream: int, pos: np.ndarray) -> np.ndarray:
    """``philox_bits`` over an array of positions (numpy uint64 arithmetic: the same integers, vectorised)."""
    m = np.uint64(_M32)
    c0 = np.asarray(pos, dtype=np.uint64) & m
    c1 = np.full_like(c0, stream & _M32)
    c2, c3 = np.zeros_like(c0), np.zeros_like(c0)
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return c0.astype(np.uint32)


@dataclass
class Sampling:
    """temperature <= 0 (or not finite) and top_k == 1 are the greedy pick; top_p outside (0, 1] counts as 1 (the kernel's rules).
    ``seed`` is 64 bits (the Philox key), ``stream`` separates independent sequences under one seed."""
    temperature: float = 1.0
    top_k: int = 40
    top_p: float = 1.0
    seed: int = 0
    stream: int = 0

    def __post_init__(self):
        if not (isinstance(self.top_k, int) and 1 <= self.top_k <= MAX_K):
            raise ValueError(f"Sampling: top_k must be an integer in 1..{MAX_K}, not {self.top_k!r}")
        if not 0 <= int(self.seed) < 1 << 64 or not 0 <= int(self.stream) < 1 << 32:
            raise ValueError("Sampling: seed is 64 bits, stream 32 bits, both unsigned")

    def pack(self) -> bytes:
        """effort_sample_params: f32 temperature, f32 top_p, u32 top_k, seed_lo, seed_hi, stream, reserved[2]; little endian."""
        return struct.pack("<ffIIIIII", float(self.temperature), float(self.top_p), self.top_k, int(self.seed) & _M32, (int(self.seed) >> 32) & _M32,
                           int(self.stream), 0, 0)

    def to_device(self, t=None, device=None):
        """The struct as a 32-byte uint8 tensor.  ``t``: an existing 32-byte tensor to rewrite in place (the decoder's: the captured
        graph reads that address), or None for a new one on ``device``."""
        import torch
        host = torch.frombuffer(bytearray(self.pack()), dtype=torch.uint8)
        if t is None:
            return host.to(device) if device is not None else host
        if t.dtype != torch.uint8 or t.numel() != 32:
            raise ValueError("Sampling.to_device: the target is a 32-byte uint8 tensor")
        t.copy_(host)
        return t


def topk_reference(logits, k: int):
    """The K largest logits, value descending, lowest index first among equal values: a stable sort on (-value, index) with NaN
    removed and the two zeros merged.  Returns (indices int64, values as stored)."""
    x = np.asarray(logits, dtype=np.float32)
    idx = np.flatnonzero(~np.isnan(x))
    v = x[idx] + np.float32(0.0)                 # -0.0 + 0.0 = +0.0: the zeros tie
    order = np.argsort(-v.astype(np.float64), kind="stable")[:k]
    sel = idx[order]
    return sel.astype(np.int64), x[sel]


def _draw(idx, val, sampling: Sampling, u: float):
    """Steps 2-3 of the specification over a selected, sorted candidate list: (picked id, margin)."""
    if idx.size == 0:
        return 0, math.inf
    t = float(np.float32(sampling.temperature))
    top_p = float(np.float32(sampling.top_p))
    if not (0.0 < top_p <= 1.0):
        top_p = 1.0
    if not (t > 0.0) or math.isinf(t) or idx.size == 1 or np.isinf(val[0]):
        return int(idx[0]), math.inf
    v = val.astype(np.float64)
    c = np.cumsum(np.exp((v - v[0]) / t))
    last = int(np.argmax(c >= top_p * c[-1]))    # the nucleus: ranks 0 .. last
    S = float(c[last])
    target = u * S
    hit = np.flatnonzero(c[:last + 1] > target)
    pick = int(hit[0]) if hit.size else last
    margin = float(np.abs(c[:last + 1] - target).min() / S)
    return int(idx[pick]), margin


def sample_reference(logits, sampling: Sampling, pos: int):
    """The specification of effort_sample in numpy, weights and sums in float64.  Returns (picked id, margin): the margin is the
    distance from u * S to the nearest cumulative boundary, divided by S (inf where nothing is drawn: greedy settings, one candidate, an
    infinite largest logit).  Every logit NaN: (0, inf)."""
    n = int(np.asarray(logits).shape[0])
    idx, val = topk_reference(logits, max(1, min(int(sampling.top_k), MAX_K, n)))
    return _draw(idx, val, sampling, philox_u(sampling.seed, sampling.stream, pos))


def sample_reference_many(logits, sampling: Sampling, positions):
    """``sample_reference`` of ONE logit row at many positions (the selection is done once): (ids int64 [P], margins float64 [P])."""
    n = int(np.asarray(logits).shape[0])
    idx, val = topk_reference(logits, max(1, min(int(sampling.top_k), MAX_K, n)))
    us = (philox_bits_many(sampling.seed, sampling.stream, np.asarray(positions)) >> 8).astype(np.float64) * 2.0 ** -24
    out = [_draw(idx, val, sampling, float(u)) for u in us]
    return np.array([o[0] for o in out], dtype=np.int64), np.array([o[1] for o in out], dtype=np.float64)
