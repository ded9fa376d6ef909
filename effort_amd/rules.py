"""Generation rules on the device: the settings of ``effort_logit_rules`` (csrc/rules.hip) and its specification restated on the host.

The rules -- repetition / presence / frequency penalties over the recent tokens, a logit bias table, min-p and the stop tokens -- run
inside the captured token step, between the LM head and the pick.  Their settings live in a 64-byte struct in device memory
(``effort_rules_params``, include/effort_hip.h) and two fixed 256-entry bias tables, so changing them rewrites those tensors and the
graph is reused.  ``rules_reference`` restates the kernel's specification step by step in numpy float32, every arithmetic step one
rounded operation: what the kernel is tested against, bit for bit.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass, field

import numpy as np

MAX_WINDOW, MAX_BIAS, MAX_STOP = 1024, 256, 8    # EFFORT_RULES_MAX_WINDOW / _BIAS / _STOP
NO_STOP = 0xFFFFFFFF                             # *stop_pos_dev while no stop token has been consumed
_FMT = "<ffffIIII8I"                             # effort_rules_params
_M32 = 0xFFFFFFFF
_QNAN = np.array([0x7FC00000], dtype=np.uint32).view(np.float32)[0]


def _is_u32(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, bool) and 0 <= int(x) <= _M32


@dataclass
class Rules:
    """``repetition_penalty`` 1, ``presence_penalty`` 0 and ``frequency_penalty`` 0 are off; they act on the tokens of the last
    ``last_n`` positions (the prompt included), 0 = none.  ``min_p``: logits below max + ln(min_p) are banned, outside (0, 1] = off.
    ``logit_bias``: {token id: value added}, -inf bans a token, a NaN value is an absent entry.  ``stop_ids``: ``Decoder.run`` ends at the
    first of them picked past the prompt."""
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    last_n: int = 64
    min_p: float = 0.0
    logit_bias: dict = field(default_factory=dict)
    stop_ids: tuple = ()

    def __post_init__(self):
        rep = float(self.repetition_penalty)
        if not (math.isfinite(rep) and rep > 0.0):
            raise ValueError(f"Rules: repetition_penalty must be finite and > 0, not {self.repetition_penalty!r}")
        if not (math.isfinite(float(self.presence_penalty)) and math.isfinite(float(self.frequency_penalty))):
            raise ValueError("Rules: presence_penalty and frequency_penalty must be finite")
        if not (_is_u32(self.last_n) and int(self.last_n) <= MAX_WINDOW):
            raise ValueError(f"Rules: last_n must be an integer in 0..{MAX_WINDOW}, not {self.last_n!r}")
        self.logit_bias = dict(self.logit_bias)
        self.stop_ids = tuple(self.stop_ids)
        if len(self.logit_bias) > MAX_BIAS:
            raise ValueError(f"Rules: at most {MAX_BIAS} logit_bias entries, not {len(self.logit_bias)}")
        if len(self.stop_ids) > MAX_STOP:
            raise ValueError(f"Rules: at most {MAX_STOP} stop_ids, not {len(self.stop_ids)}")
        if not all(_is_u32(t) for t in list(self.logit_bias) + list(self.stop_ids)):
            raise ValueError("Rules: token ids are unsigned 32-bit integers")

    def min_p_log(self) -> float:
        """f32(ln(min_p)) for 0 < min_p <= 1, else -inf (off): the host computes the logarithm, the device only adds it."""
        p = float(self.min_p)
        return float(np.float32(math.log(p))) if 0.0 < p <= 1.0 else -math.inf

    def pack(self, first_pos: int = 0) -> bytes:
        """effort_rules_params: f32 repetition_penalty, presence_penalty, frequency_penalty, min_p_log, u32 last_n, n_bias, n_stop,
        first_pos, stop_ids[8]; 64 bytes, little endian."""
        stops = [int(t) for t in self.stop_ids] + [0] * (MAX_STOP - len(self.stop_ids))
        return struct.pack(_FMT, float(self.repetition_penalty), float(self.presence_penalty), float(self.frequency_penalty), self.min_p_log(),
                           int(self.last_n), len(self.logit_bias), len(self.stop_ids), int(first_pos) & _M32, *stops)

    def bias_tables(self):
        """The two fixed tables (uint32 ids [256], float32 values [256]), the entries in the dict's order, zeros behind them."""
        ids, vals = np.zeros(MAX_BIAS, dtype=np.uint32), np.zeros(MAX_BIAS, dtype=np.float32)
        for j, (t, v) in enumerate(self.logit_bias.items()):
            ids[j], vals[j] = int(t), np.float32(v)
        return ids, vals

    def to_device(self, first_pos: int = 0, t=None, bias_ids=None, bias_vals=None, device=None):
        """The struct as a 64-byte uint8 tensor and the bias tables as int32 [256] / float32 [256] tensors: (params, ids, values).  ``t``,
        ``bias_ids``, ``bias_vals``: existing tensors to rewrite in place (the decoder's: the captured graph reads those addresses), or
        None for new ones on ``device``."""
        import torch
        ids, vals = self.bias_tables()
        host = (torch.frombuffer(bytearray(self.pack(first_pos)), dtype=torch.uint8), torch.from_numpy(ids.view(np.int32)), torch.from_numpy(vals))
        want = ((torch.uint8, 64), (torch.int32, MAX_BIAS), (torch.float32, MAX_BIAS))
        out = []
        for h, dst, (dtype, numel) in zip(host, (t, bias_ids, bias_vals), want):
            if dst is None:
                out.append(h.to(device) if device is not None else h)
                continue
            if dst.dtype != dtype or dst.numel() != numel:
                raise ValueError("Rules.to_device: the targets are a 64-byte uint8 tensor, an int32 [256] and a float32 [256] tensor")
            dst.copy_(h)
            out.append(dst)
        return tuple(out)


def _keep_nan(before, after):
    """A NaN logit passes a rule with its bits unchanged; a NaN the rule's arithmetic makes of other values is 0x7FC00000."""
    if np.isnan(before):
        return before
    return _QNAN if np.isnan(after) else after


def rules_reference(logits, packed_params, seq=None, pos: int = 0, tok=None, bias_ids=None, bias_vals=None, stop_pos=None):
    """The specification of effort_logit_rules (include/effort_hip.h) in numpy float32, sanitisation included.  It reads the PACKED
    struct, so host and device judge the same f32 values.  ``seq`` / ``tok``: both or neither (None); ``bias_ids`` / ``bias_vals``
    likewise; ``stop_pos``: the value of *stop_pos_dev before the call, or None for no stop reporting.
    Returns (out float32 [n], seq after the call as uint32 or None, stop_pos after the call or None, status bit 0 raised: 0 / 1)."""
    f32 = np.float32
    out = np.array(logits, dtype=np.float32, copy=True)
    n = int(out.size)
    rep, presence, frequency, min_p_log, last_n, n_bias, n_stop, first_pos, *stops = struct.unpack(_FMT, bytes(packed_params))
    pos = int(pos) & _M32
    # 0. sanitise
    rep = f32(rep) if math.isfinite(rep) and rep > 0.0 else f32(1.0)
    presence = f32(presence) if math.isfinite(presence) else f32(0.0)
    frequency = f32(frequency) if math.isfinite(frequency) else f32(0.0)
    last_n, n_bias, n_stop = min(last_n, MAX_WINDOW), min(n_bias, MAX_BIAS), min(n_stop, MAX_STOP)
    min_p_on = math.isfinite(min_p_log) and min_p_log <= 0.0
    if bias_ids is None or bias_vals is None:
        n_bias = 0
    # 1. record
    status, window = 0, []
    seq_after = None
    if seq is not None and tok is not None:
        seq_after = (np.asarray(seq).astype(np.int64) & _M32).astype(np.uint32)     # (an int32 view of the device buffer is the same ids)
        tok = int(tok) & _M32
        if pos < seq_after.size:
            seq_after[pos] = tok
            W = min(last_n, pos + 1)
            window = seq_after[pos + 1 - W:pos + 1].tolist()
        else:
            status = 1
        # 2. stop
        if stop_pos is not None and pos >= first_pos and tok in stops[:n_stop] and int(stop_pos) == NO_STOP:
            stop_pos = pos
    with np.errstate(all="ignore"):
        # 3. copy: out is in.  4. penalties: every distinct id of the window once
        counts = {}
        for t in window:
            if t < n:
                counts[t] = counts.get(t, 0) + 1
        for t, c in counts.items():
            l0 = out[t]
            l = l0
            if rep != f32(1.0):
                l = f32(l / rep) if l > f32(0.0) else f32(l * rep)
            scaled = f32(f32(c) * frequency)
            sub = f32(scaled + presence)
            out[t] = _keep_nan(l0, f32(l - sub))
        # 5. bias: the present entry with the highest index wins
        winners = {}
        for j in range(n_bias):
            t, v = int(bias_ids[j]) & _M32, f32(bias_vals[j])
            if t < n and not np.isnan(v):
                winners[t] = v
        for t, v in winners.items():
            out[t] = _keep_nan(out[t], f32(out[t] + v))
        # 6. min-p
        if min_p_on:
            real = out[~np.isnan(out)]
            m = real.max() if real.size else f32(-np.inf)
            if np.isfinite(m):
                thr = f32(m + f32(min_p_log))
                out[out < thr] = f32(-np.inf)
    return out, seq_after, (None if stop_pos is None else int(stop_pos)), status
