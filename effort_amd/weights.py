"""``ExpertWeights`` -- the per-matrix weight bundle of the reference (loader.swift:46-167).

Same fields and meaning: ``buckets`` [E, inSize*percentLoad, cols], ``stats`` [E, inSize*percentLoad, 4]
(Q4: f32 [E, inSize*8, 2]), ``probes`` [E, 4096], optional ``outliers`` f32 [n, 4] and dense ``core``
f16 [outSize, inSize]; ``expertSize = percentLoad*inSize`` (loader.swift:50).  Tensors live in HBM as
torch CUDA tensors (device memory plumbing only); the C-ABI handle borrows their pointers.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from .runtime import gpu as _gpu


def _ptr(t: torch.Tensor | None):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def unbucket(buckets: torch.Tensor, inSize: int, outSize: int) -> torch.Tensor:
    """The UN-BUCKETED matrix U of FP16 buckets at ``percentLoad`` 16 -- f16 [E, outSize, inSize] -- in torch ops, on the host or the
    device the buckets live on.  ``buckets`` is [E, 16 * inSize, cols] (or one expert's [16 * inSize, cols]) of 16-bit words, dense or
    a strided view of pitched storage: only the ``cols = outSize / 16`` payload words of a row are read, the padding is ignored.

    For expert e, input j, bucket column c and rank r let w = buckets[e][r * inSize + j][c].  w == 0x0000 is skipped; otherwise
    U[e][16 c + (w & 15)][j] = w: the position bits stay in the value, exactly as bucketMul multiplies them.  Elements no entry names
    are +0.  Raises ValueError when two non-skipped entries of one (e, j, c) name the same position (the converter's literal
    preBucketize path can write that; ``effort_convert_status`` reports drops then): such a bundle holds no matrix to return.

    This is the specification of what ``Decoder.prefill(weights="buckets")`` multiplies by, and the way back from a bucket file
    written without cores: U is the core with the low four mantissa bits of every weight replaced by its position."""
    inSize, outSize = int(inSize), int(outSize)
    if buckets.element_size() != 2:
        raise ValueError("unbucket: buckets of 16-bit words")
    b = buckets.view(torch.int16)
    if b.dim() == 2:
        b = b.unsqueeze(0)
    cols = outSize // 16
    if outSize % 16 or b.dim() != 3 or b.shape[1] != 16 * inSize or b.shape[2] < cols:
        raise ValueError(f"unbucket: buckets [E, {16 * inSize}, >= {cols}] expected (percentLoad 16), got {tuple(b.shape)}")
    out = torch.empty((b.shape[0], outSize, inSize), dtype=torch.int16, device=b.device)
    for e in range(b.shape[0]):                                # (an expert at a time: the scatter works on 4-byte words)
        w = b[e, :, :cols].reshape(16, inSize, cols).to(torch.int32) & 0xFFFF
        w = w.permute(1, 2, 0).contiguous()                    # [j][c][rank]
        pos = (w & 15).to(torch.int64)
        named = torch.zeros((inSize, cols, 16), dtype=torch.int32, device=b.device).scatter_add_(2, pos, (w != 0).to(torch.int32))
        if bool((named > 1).any()):
            raise ValueError("unbucket: two entries of one bucket name the same output position -- the bundle is not un-bucketable")
        # (no two non-zero entries share a slot, and a skipped entry adds 0: the sum IS the entry)
        u = torch.zeros((inSize, cols, 16), dtype=torch.int32, device=b.device).scatter_add_(2, pos, w)
        u = ((u ^ 0x8000) - 0x8000).to(torch.int16)            # the 16-bit pattern as int16
        out[e] = u.reshape(inSize, outSize).t()
    return out.view(torch.float16)


def unbucket_q4(buckets: torch.Tensor, stats: torch.Tensor, inSize: int, outSize: int) -> torch.Tensor:
    """The UN-BUCKETED matrix U4 of Q4 buckets -- f16 [E, outSize, inSize] -- in torch ops, on the host or the device the buckets
    live on.  ``buckets`` is [E, 8 * inSize, outSize / 32] (or one expert's 2-d tensor) of 16-bit words, ``stats`` f32
    [E, 8 * inSize, 2].

    Bucket row i = 8 j + r holds rank r of input j.  Word x of a row holds four nibbles, the first in bits 15 .. 12; nibble n
    (0 = highest) is sign << 3 | pos and names output 32 x + 8 n + pos.  U4[e][32 x + 8 n + pos][j] = +-f16(m), m = stats[e][i][1]
    -- the second lane, the one prepareDispatchQ4 reads --, + for a clear sign bit: a weight that was zero counts as +m, as the
    reference's Metal kernel treats it (its Python draft gives 0).  Raises ValueError when the eight ranks of one (e, j, x, n) do not
    name eight different positions, or when a mean is not a finite f16 number stored as f32: such a bundle holds no matrix to
    return.  The Q4 converter always writes bundles that do.

    This is the specification of what ``Decoder.prefill(weights="q4")`` multiplies a Q4 bundle by, before the outliers."""
    inSize, outSize = int(inSize), int(outSize)
    if buckets.element_size() != 2:
        raise ValueError("unbucket_q4: buckets of 16-bit words")
    b = buckets.view(torch.int16)
    if b.dim() == 2:
        b = b.unsqueeze(0)
    words = outSize // 32
    if outSize % 32 or b.dim() != 3 or b.shape[1] != 8 * inSize or b.shape[2] < words:
        raise ValueError(f"unbucket_q4: buckets [E, {8 * inSize}, >= {words}] expected, got {tuple(b.shape)}")
    E = b.shape[0]
    if stats.dtype != torch.float32 or stats.numel() != E * 8 * inSize * 2:
        raise ValueError(f"unbucket_q4: stats f32 [E, {8 * inSize}, 2] expected, got {stats.dtype} {tuple(stats.shape)}")
    m = stats.reshape(E, inSize, 8, 2)[..., 1].to(b.device)
    m16 = m.to(torch.float16)
    if not bool(torch.isfinite(m).all()) or not bool((m16.to(torch.float32) == m).all()):
        raise ValueError("unbucket_q4: a row mean (stats lane 1) is not a finite f16 number stored as f32 -- the bundle is not un-bucketable")
    mbits = m16.contiguous().view(torch.int16).to(torch.int32) & 0xFFFF                       # [E][j][r]
    out = torch.empty((E, outSize, inSize), dtype=torch.int16, device=b.device)
    for e in range(E):
        w = b[e, :, :words].reshape(inSize, 8, words).to(torch.int32) & 0xFFFF                 # [j][r][x]
        nib = torch.stack([(w >> 12) & 15, (w >> 8) & 15, (w >> 4) & 15, w & 15], dim=-1)      # [j][r][x][n]
        val = mbits[e][:, :, None, None] ^ ((nib >> 3) << 15)
        pos = (nib & 7).permute(0, 2, 3, 1).contiguous().to(torch.int64)                       # [j][x][n][r]
        val = val.permute(0, 2, 3, 1).contiguous()
        named = torch.zeros((inSize, words, 4, 8), dtype=torch.int32, device=b.device).scatter_add_(3, pos, torch.ones_like(val))
        if bool((named != 1).any()):
            raise ValueError("unbucket_q4: the eight ranks of a bucket do not name eight different positions -- the bundle is not un-bucketable")
        u = torch.zeros((inSize, words, 4, 8), dtype=torch.int32, device=b.device).scatter_add_(3, pos, val)
        u = ((u ^ 0x8000) - 0x8000).to(torch.int16)            # the 16-bit pattern as int16
        out[e] = u.reshape(inSize, outSize).t()
    return out.view(torch.float16)


class ExpertWeights:
    def __init__(self, buckets: torch.Tensor, stats: torch.Tensor, probes: torch.Tensor, inSize: int, outSize: int,
                 percentLoad: int | None = None, numExperts: int = 1, outliers: torch.Tensor | None = None,
                 core: torch.Tensor | None = None, q4: bool = False):
        self.q4 = bool(q4)                                    # goQ4 (main.swift:47) per bundle
        self.inSize = int(inSize)
        self.outSize = int(outSize)
        self.percentLoad = int(percentLoad) if percentLoad is not None else (8 if q4 else 16)   # loader.swift:64
        self.numExperts = int(numExperts)
        self.core = core
        self.outliers = outliers
        self.bucketsLoaded = True
        dev = buckets.device
        if dev.type != "cuda":
            raise ValueError("ExpertWeights tensors must be on the GPU")
        cols = self.outSize // 32 if q4 else self.outSize // 16
        rows = self.inSize * self.percentLoad
        # Matrix3D shapes of loader.swift:70,76 (bit-level dtype: 16-bit words / f16x4 or f32x2 stats)
        # ``buckets`` may be a view of PITCHED storage -- rows more than ``cols`` words apart, e.g. on whole 128-byte lines as
        # ``from_core`` / ``bucketize(rowPitch=...)`` write them (effort_weights_fp16_pitched): kept as is, [E, rows, cols]
        # strided; anything else is made dense like the reference's Matrix3D.
        b = buckets.view(torch.int16) if buckets.element_size() == 2 else buckets
        if b.dim() == 2:
            b = b.unsqueeze(0)
        if (not q4 and tuple(b.shape) == (self.numExperts, rows, cols) and b.stride(2) == 1 and b.stride(1) > cols
                and b.stride(1) % 4 == 0 and (self.numExperts == 1 or b.stride(0) == rows * b.stride(1))):
            self.buckets = b
            self.rowPitch = b.stride(1) * 2
        else:
            self.buckets = buckets.contiguous().view(torch.int16).reshape(self.numExperts, rows, cols)
            self.rowPitch = cols * 2
        if q4:
            self.stats = stats.contiguous().to(torch.float32).reshape(self.numExperts, rows, 2)
        else:
            self.stats = stats.contiguous().view(torch.int16).reshape(self.numExperts, rows, 4)
        self.probes = probes.contiguous().view(torch.int16).reshape(self.numExperts, 4096)
        if outliers is not None:
            self.outliers = outliers.contiguous().to(torch.float32).reshape(-1, 4)
        self._gpu = _gpu(dev.index)
        self._handle = None

    @property
    def expertSize(self) -> int:
        return self.percentLoad * self.inSize

    @property
    def handle(self):
        """effort_w* registered with the context (lazily, once)."""
        if not self.bucketsLoaded:
            raise ValueError("a core-only bundle has no buckets to register: it multiplies through basicMul (expertMul.swift:29-31)")
        if self._handle is None:
            g, lib = self._gpu, _lib.lib()
            g._bind_stream()
            if self.q4:
                n = 0 if self.outliers is None else self.outliers.shape[0]
                h = lib.effort_weights_q4(g.ctx, _ptr(self.buckets), _ptr(self.stats), _ptr(self.probes), _ptr(self.outliers),
                                          n, self.inSize, self.outSize, self.numExperts)
            else:
                h = lib.effort_weights_fp16_pitched(g.ctx, _ptr(self.buckets), self.rowPitch, _ptr(self.stats), _ptr(self.probes),
                                                    self.inSize, self.outSize, self.percentLoad, self.numExperts)
            if not h:
                detail = lib.effort_last_error(g.ctx)
                raise _lib.EffortError(-2, "ExpertWeights", detail.decode() if detail else "")
            self._handle = h
        return self._handle

    def __del__(self):
        try:
            if self._handle is not None:
                _lib.lib().effort_weights_free(self._handle)
                self._handle = None
        except Exception:
            pass

    # -- constructors ------------------------------------------------------------------------------
    @classmethod
    def from_core(cls, core: torch.Tensor, aligned: bool = True) -> "ExpertWeights":
        """Dense f16 matrix [outSize, inSize] -> FP16 bundle via the GPU converter (= bucketize()).  ``aligned`` (default):
        the converter writes the bucket rows on whole 128-byte lines (same values, rows ``aligned_row_pitch`` bytes apart; the
        multiply streams them ~10 % faster than the reference's dense rows when HBM is saturated) -- ``buckets`` is then a
        strided view; ``aligned=False`` gives the reference's dense tensor."""
        from .convert import aligned_row_pitch, bucketize
        tensors: dict[str, torch.Tensor] = {}
        bucketize(core, "", tensors, goQ8=False, rowPitch=aligned_row_pitch(core.shape[0]) if aligned else 0)
        return cls(tensors["buckets"], tensors["bucket.stats"], tensors["probes"], inSize=core.shape[1],
                   outSize=core.shape[0], core=core)

    @classmethod
    def core_only(cls, core: torch.Tensor, q4: bool = True) -> "ExpertWeights":
        """A bundle whose buckets were not loaded (loader.swift:105-107): the dense f16 ``core`` [outSize, inSize] alone,
        ``bucketsLoaded = False``, no handle.  ``expertMul`` sends it to ``basicMul`` (expertMul.swift:29-31); it is what wk, wv
        and wo of a Q4 model are (q4_convert.py:53)."""
        if not (core.dim() == 2 and core.element_size() == 2):
            raise ValueError("core must be a 16-bit matrix [outSize, inSize]")
        ew = object.__new__(cls)
        ew.q4 = bool(q4)
        ew.outSize, ew.inSize = int(core.shape[0]), int(core.shape[1])
        ew.percentLoad = 8 if q4 else 16
        ew.numExperts = 1
        ew.core = core.contiguous()
        ew.outliers = None
        ew.bucketsLoaded = False
        ew.buckets = ew.stats = ew.probes = None
        ew.rowPitch = 0
        ew._gpu = _gpu(core.device.index) if core.is_cuda else None      # (a host tensor: a bundle read back for inspection, never multiplied)
        ew._handle = None
        return ew

    @classmethod
    def from_core_q4(cls, core: torch.Tensor, perc: float = 0.02, keep_core: bool = True) -> "ExpertWeights":
        """Dense f16 matrix [outSize, inSize] -> Q4 bundle via the GPU Q4 converter (q4_convert.py:54,63: convert(W.T)), the
        top ``perc`` of the weights kept as outliers.  ``keep_core=False`` drops the f16 core: the bundle then decodes as ever and
        prefills through ``Decoder.prefill(weights="q4")`` alone."""
        from .q4 import convert
        t = convert(core.t().contiguous(), perc)
        outl = t["outliers"] if t["outliers"].shape[0] else None
        return cls(t["buckets"], t["bucket.stats"], t["probes"], inSize=core.shape[1], outSize=core.shape[0], outliers=outl,
                   core=core if keep_core else None, q4=True)

    @classmethod
    def stack(cls, experts: list["ExpertWeights"]) -> "ExpertWeights":
        """Mixtral-style expert stacking: all experts in one buffer, selected by expNo (loader.swift:113-166)."""
        e0 = experts[0]
        return cls(torch.cat([e.buckets for e in experts]), torch.cat([e.stats for e in experts]),
                   torch.cat([e.probes for e in experts]), e0.inSize, e0.outSize, e0.percentLoad,
                   numExperts=sum(e.numExperts for e in experts), outliers=e0.outliers, q4=e0.q4)

    def truncated(self, percentLoad: int) -> "ExpertWeights":
        """Load only the first ``percentLoad`` rank slices (loader.swift:157-159, copyFrom(mySize: true))."""
        assert not self.q4 and 1 <= percentLoad <= self.percentLoad
        rows = self.inSize * percentLoad
        return ExpertWeights(self.buckets[:, :rows].contiguous(), self.stats[:, :rows].contiguous(), self.probes,
                             self.inSize, self.outSize, percentLoad, self.numExperts, core=self.core)

    def unbucket(self) -> torch.Tensor:
        """``unbucket`` of this bundle's buckets: f16 [numExperts, outSize, inSize], the matrix ``Decoder.prefill(weights="buckets")``
        multiplies by.  FP16 bundles with their buckets loaded at ``percentLoad`` 16 only."""
        if self.q4 or not self.bucketsLoaded or self.percentLoad != 16:
            raise ValueError("ExpertWeights.unbucket: an FP16 bundle with its buckets loaded at percentLoad 16")
        return unbucket(self.buckets, self.inSize, self.outSize)

    def unbucket_q4(self) -> torch.Tensor:
        """``unbucket_q4`` of this bundle's buckets and stats: f16 [numExperts, outSize, inSize], the matrix
        ``Decoder.prefill(weights="q4")`` multiplies by before it adds the outliers.  Q4 bundles with their buckets loaded only."""
        if not self.q4 or not self.bucketsLoaded:
            raise ValueError("ExpertWeights.unbucket_q4: a Q4 bundle with its buckets loaded")
        return unbucket_q4(self.buckets, self.stats, self.inSize, self.outSize)

    def align_rows(self) -> int:
        """For bundles held in the reference's dense layout (loaded from a file, ``from_core(aligned=False)``): give the handle
        its own copy of the buckets with every row on a 128-byte line (effort_weights_align_rows).  No-op for bundles that are
        aligned already (``from_core`` writes them so).  Call before capturing launches into a graph.  Returns the row pitch."""
        self._gpu.check(_lib.lib().effort_weights_align_rows(self.handle), "ExpertWeights.align_rows")
        return int(_lib.lib().effort_weights_row_pitch(self.handle))

    def refresh(self):
        """The buffers were rewritten in place: re-read the bound the multiply's fixed-point scale comes from."""
        if self._handle is not None:
            self._gpu.check(_lib.lib().effort_weights_refresh(self._handle), "ExpertWeights.refresh")

    def rank_bound(self) -> list[float]:
        buf = (C.c_float * self.numExperts)()
        self._gpu.check(_lib.lib().effort_weights_get_bound(self.handle, buf), "ExpertWeights.rank_bound")
        return list(buf)

    def set_rank_bound(self, bound):
        buf = (C.c_float * self.numExperts)(*[float(x) for x in bound])
        self._gpu.check(_lib.lib().effort_weights_set_bound(self.handle, buf), "ExpertWeights.set_rank_bound")

    def column_shard(self, rank: int, world: int) -> "ExpertWeights":
        """Bucket-column (output) shard for multi-GPU (effort_weights_column_shard): columns [rank*C/G, (rank+1)*C/G) of every
        bucket row as a VIEW of this bundle's buffers -- no copy --, stats and probes shared (they are row-global, so every rank
        selects the same rows), the full matrix's fixed-point bound (every rank rounds on the same grid), and for Q4 the slice of
        the outlier index on those outputs.  Any split into an even number of columns per rank is valid (the multiply masks a
        ragged last tile: 11008 outputs over 8 ranks = 86 columns each).  Keep the full bundle alive while the shard is used."""
        from .sharded import shard_columns, shard_outliers
        lib = _lib.lib()
        unit = 32 if self.q4 else 16
        if (self.buckets.shape[2] // world) % 2:
            # an ODD number of columns per rank (Q4 only: 11008 outputs over 8 ranks = 43 words): a view would start rows on odd
            # 16-bit words, which the dword row loads cannot take -- this rank gets its own dense copy of its columns instead
            b = shard_columns(self.buckets, rank, world)
            per = b.shape[2]
            sh = ExpertWeights(b, self.stats, self.probes, self.inSize, per * unit, self.percentLoad, self.numExperts,
                               outliers=shard_outliers(self.outliers, rank, world, self.outSize),
                               core=None if self.core is None else self.core[rank * per * unit:(rank + 1) * per * unit], q4=self.q4)
            sh.set_rank_bound(self.rank_bound())
            return sh
        h = lib.effort_weights_column_shard(self.handle, int(rank), int(world))
        if not h:
            detail = lib.effort_last_error(self._gpu.ctx)
            raise _lib.EffortError(-2, "ExpertWeights.column_shard", detail.decode() if detail else "")
        per = self.buckets.shape[2] // world
        sh = object.__new__(ExpertWeights)
        sh.__dict__.update(self.__dict__)
        sh.buckets = self.buckets[:, :, rank * per:(rank + 1) * per]              # (a strided view, like the handle's)
        sh.outSize = per * unit
        sh.outliers = shard_outliers(self.outliers, rank, world, self.outSize)
        sh.core = None if self.core is None else self.core[rank * per * unit:(rank + 1) * per * unit]
        sh._handle = h
        sh._full = self                                                            # the view borrows the full bundle's buffers and index
        return sh
