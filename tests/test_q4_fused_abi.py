"""The Q4 glue-fused launch (effort_bucketmul_q4_group_fused) and the per-bundle dense fallback, as far as a machine without a GPU
reaches: the header and the built library agree on the new entry, a null context is refused, the shipped library holds the
FUSED = true instantiations of the Q4 multiply kernel with the properties every multiply kernel keeps (no scratch segment, no clock
reads, the bucket rows streamed non-temporally), the Python marshalling accepts the extras for Q4 groups, and a Q4 model file's
core-only bundles load as such."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from effort_amd import bucketfile as bf
from tests.test_abi import _header_functions, _multiply_kernel_disassembly
from tests.test_bucketfile import fake_model, fake_q4

LLVM = "/opt/rocm/lib/llvm/bin"
Q4_FUSED = re.compile(r"bucket_mul_kernelILi1ELi(\d+)ELi(\d+)ELb1ELb0ELb([01])E")        # <kQ4, E, W, FUSED = true, COMPACT = false, PERSIST>


def test_header_declares_and_library_exports_the_entry(hip_lib_built):
    assert "effort_bucketmul_q4_group_fused" in _header_functions()
    syms = subprocess.run(["nm", "-D", "--defined-only", hip_lib_built], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT effort_bucketmul_q4_group_fused\b", syms)
    import effort_amd._lib as L
    assert "effort_bucketmul_q4_group_fused" in L._SIGS


def test_null_context_is_an_argument_error(hip_lib_built):
    lib = ctypes.CDLL(hip_lib_built)
    fn = lib.effort_bucketmul_q4_group_fused
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int] + [ctypes.c_void_p] * 8
    EFFORT_ERR_ARG = -1
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "effort_hip.h")).read()
    m = re.search(r"EFFORT_ERR_ARG\s*=?\s*(-?\d+)", hdr)
    if m:
        EFFORT_ERR_ARG = int(m.group(1))
    assert fn(None, 1, None, None, None, None, None, None, None, None) == EFFORT_ERR_ARG


def _kernel_metadata(lib_path, tmp_path):
    """{kernel symbol: (private segment bytes, vgprs)} from the code object's metadata note."""
    import glob
    import shutil
    work = os.path.join(str(tmp_path), "meta_" + os.path.basename(lib_path))
    shutil.copy(lib_path, work)
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", work], capture_output=True, cwd=str(tmp_path), check=True)
    out = {}
    for co in sorted(glob.glob(work + ".*gfx950")):
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count", notes):
            nm = re.search(r"\.name:\s+(\S+)", blk)
            ps = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
            vg = re.search(r"\.vgpr_count:\s+(\d+)", blk)
            if nm and ps and vg:
                out[nm.group(1)] = (int(ps.group(1)), int(vg.group(1)))
    return out


def test_shipped_library_holds_the_q4_fused_kernels(hip_lib_built, tmp_path):
    """bucket_mul_kernel<kQ4, E, W, FUSED = true>: the generic form for every launch geometry and the lean plain form for the 8-wave
    ones; like every multiply kernel they have no scratch segment, read no clock, and stream the bucket rows with `nt` (the kernels
    of group launches -- persistent, or E = 4 -- hold the second, temporal copy of the loop: half their 8-byte row loads)."""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    prod = _multiply_kernel_disassembly(hip_lib_built, tmp_path)
    body, name = {}, None
    for line in prod.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1) if Q4_FUSED.search(m.group(1)) else None
            if name:
                body[name] = []
        elif name:
            body[name].append(line)
    geoms = {(int(Q4_FUSED.search(k).group(1)), int(Q4_FUSED.search(k).group(2)), Q4_FUSED.search(k).group(3) == "1") for k in body}
    for w, e in ((16, 1), (16, 2), (16, 4), (8, 1), (8, 2), (8, 4), (4, 1), (4, 2), (4, 4), (2, 4)):
        assert (e, w, True) in geoms, (e, w)
    for e in (1, 2, 4):
        assert (e, 8, False) in geoms, e                                       # the lean plain instantiations
    meta = _kernel_metadata(hip_lib_built, tmp_path)
    for k, lines in body.items():
        text = "\n".join(lines)
        assert "s_memrealtime" not in text and "HW_REG_XCC_ID" not in text, k
        assert "scratch_" not in text, k
        assert k in meta and meta[k][0] == 0, (k, meta.get(k))                 # no scratch segment
        e, persist = int(Q4_FUSED.search(k).group(1)), Q4_FUSED.search(k).group(3) == "1"
        rows = [l for l in lines if re.search(r"buffer_load_(ushort|dword|dwordx2) ", l) and " lds" not in l and " offen" in l and " sc1" not in l]
        nt = sum(" nt" in l for l in rows)
        assert rows and nt > 0, k
        if e == 4:
            x2 = [l for l in rows if "buffer_load_dwordx2" in l]
            assert x2 and 2 * sum(" nt" in l for l in x2) == len(x2), k           # both policies, chosen per item
        elif not persist:
            width = "buffer_load_ushort" if e == 1 else "buffer_load_dword "
            mine = [l for l in rows if width in l]
            assert mine and all(" nt" in l for l in mine), k                      # lean E = 1 / 2: the non-temporal policy alone


class _Vec:
    """What _marshal asks of a vector, without a GPU: a contiguous f32 (or f16) CUDA vector at an address."""
    is_cuda = True

    def __init__(self, n, addr, dtype=torch.float32):
        self.n, self.value, self.dtype = n, addr, dtype

    def is_contiguous(self):
        return True

    def numel(self):
        return self.n

    def element_size(self):
        return 2 if self.dtype == torch.float16 else 4


class _Bundle:
    q4, inSize, outSize = True, 4096, 4096
    handle = ctypes.c_void_p(0x1000)


def test_marshal_accepts_q4_extras():
    from effort_amd.bucket_mul import _marshal
    v, out, x3, h = _Vec(4096, 0x2000), _Vec(4096, 0x3000), _Vec(4096, 0x4000), _Vec(4096, 0x5000)
    wn = _Vec(4096, 0x6000, torch.float16)
    calls = [(v, _Bundle(), None, out, 0.25, {"gate": x3, "resid": h}), (v, _Bundle(), None, out, 0.5, {"norm": wn}), (v, _Bundle(), None, out, 1.0)]
    n, ws, vs, es, outs, eff, pre, aux, res = _marshal(calls, True)
    assert n == 3 and list(pre) == [1, 2, 0]
    assert list(aux) == [0x4000, 0x6000, None] and list(res) == [0x5000, None, None]
    assert list(eff) == [0.25, 0.5, 1.0]
    assert _marshal(calls[2:], True)[6:] == (None, None, None)                 # a plain Q4 group carries no extras
    with pytest.raises(ValueError):
        _marshal([(v, _Bundle(), None, out, 0.25, {"gate": x3, "norm": wn})], True)
    with pytest.raises(ValueError):
        _marshal([(v, _Bundle(), None, out, 0.25, {"gate": x3, "norm": wn})], False)


def test_core_only_bundles_of_a_q4_model_file(tmp_path):
    """loader.swift:105-107: a bundle stored as a core alone has bucketsLoaded = false.  wk, wv and wo of a convertMistral(q4=True)
    model come back so with dense_ok=True; the default keeps raising."""
    src = fake_model(1)
    bf.convertMistral(src, bf.TensorSaver(str(tmp_path), "model", pad_total=False), numLayers=1, q4=True, device="cpu", bucketize_q4=fake_q4).save()
    L = bf.TensorLoader(str(tmp_path), "model")
    for w, key in (("k", "k_proj"), ("v", "v_proj"), ("o", "o_proj")):
        ew = bf.loadExpertWeights(L, f"layers.0.attention.w{w}", q4=True, device="cpu", dense_ok=True)
        core = src[f"model.layers.0.self_attn.{key}.weight"]
        assert ew.q4 and not ew.bucketsLoaded and ew.buckets is None and torch.equal(ew.core, core)
        assert (ew.outSize, ew.inSize) == tuple(core.shape) and ew.percentLoad == 8
        with pytest.raises(ValueError):
            ew.handle                                                          # nothing to register: expertMul sends it to basicMul
        with pytest.raises(KeyError):
            bf.loadExpertWeights(L, f"layers.0.attention.w{w}", q4=True, device="cpu")
