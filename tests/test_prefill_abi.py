"""CPU tests of the prompt-prefill entry points (effort_dense_gemm_rows and the block forms of the glue): declared in
include/effort_hip.h, bound in effort_amd._lib._SIGS with the argument kinds the header gives them, exported by the library, and
refusing bad arguments with their return codes.  pos0 and rows are host values and are judged before the pointers, so every refusal
here needs neither a context nor a GPU; nothing is computed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I, F = "ptr", "int", "float"
WANT = {
    "effort_dense_gemm_rows": [P, P, P, P, I, I, I],
    "effort_fetch_rows": [P, P, P, P, I, I],
    "effort_add_rmsnorm_mul_rows": [P, P, P, P, P, I, I],
    "effort_rope_kv_rows": [P, P, P, P, P, P, P, I, I, I, I, I, I, F],
    "effort_attention_rows": [P, P, P, P, I, I, P, I, I, I],
}
ERR_ARG, ERR_SHAPE = -1, -2


def _header_src():
    src = open(os.path.join(ROOT, "include", "effort_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", src, flags=re.S)


def _header_params(name):
    m = re.search(r"EFFORT_API\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", _header_src())
    assert m, name + " is not declared in include/effort_hip.h"
    return [P if "*" in p else [w for w in p.split() if w != "const"][0] for p in m.group(1).split(",")]


def test_header_declares_the_prefill_entry_points():
    for name, kinds in WANT.items():
        assert _header_params(name) == kinds, name
    assert re.search(r"#define\s+EFFORT_PREFILL_MAX_ROWS\s+64\b", _header_src())


def test_binding_has_the_prefill_entry_points():
    from effort_amd import _lib
    for name, kinds in WANT.items():
        assert name in _lib._SIGS, name
        res, args = _lib._SIGS[name]
        assert res is C.c_int
        assert [P if a is C.c_void_p else {C.c_int: I, C.c_float: F}[a] for a in args] == kinds, name


def test_null_arguments_are_reported_not_crashed(hip_lib_built):
    import effort_amd
    lib = effort_amd.lib()
    rope = C.c_float(1e6)
    assert lib.effort_dense_gemm_rows(None, None, None, None, 4096, 4096, 16) == ERR_ARG
    assert lib.effort_fetch_rows(None, None, None, None, 4096, 16) == ERR_ARG
    assert lib.effort_add_rmsnorm_mul_rows(None, None, None, None, None, 4096, 16) == ERR_ARG
    assert lib.effort_rope_kv_rows(None, None, None, None, None, None, None, 0, 16, 8, 2, 128, 32, rope) == ERR_ARG
    assert lib.effort_attention_rows(None, None, None, None, 0, 16, None, 8, 128, 32) == ERR_ARG


def test_bad_values_return_their_codes(hip_lib_built):
    """rows outside 1 .. 64 and a block that leaves the cache are argument errors, a shape the block multiply does not serve is a
    shape error -- the word a caller falls back on; none of them looks at a pointer."""
    import effort_amd
    lib = effort_amd.lib()
    rope = C.c_float(1e6)
    for rows in (0, 65, -1):
        assert lib.effort_dense_gemm_rows(None, None, None, None, 4096, 4096, rows) == ERR_ARG
        assert lib.effort_fetch_rows(None, None, None, None, 4096, rows) == ERR_ARG
        assert lib.effort_add_rmsnorm_mul_rows(None, None, None, None, None, 4096, rows) == ERR_ARG
        assert lib.effort_rope_kv_rows(None, None, None, None, None, None, None, 0, rows, 8, 2, 128, 128, rope) == ERR_ARG
        assert lib.effort_attention_rows(None, None, None, None, 0, rows, None, 8, 128, 128) == ERR_ARG
    assert lib.effort_dense_gemm_rows(None, None, None, None, 48, 4096, 16) == ERR_SHAPE          # inDim % 32 != 0
    assert lib.effort_dense_gemm_rows(None, None, None, None, 16, 4096, 16) == ERR_SHAPE
    assert lib.effort_dense_gemm_rows(None, None, None, None, 65536, 32768, 16) == ERR_SHAPE      # W of 4 GiB
    assert lib.effort_dense_gemm_rows(None, None, None, None, 0, 4096, 16) == ERR_ARG
    assert lib.effort_dense_gemm_rows(None, None, None, None, 4096, 0, 16) == ERR_ARG
    for pos0, rows, maxTokens in ((-1, 4, 32), (29, 4, 32), (32, 1, 32), (0, 33, 32), (2147483647, 2, 32)):
        assert lib.effort_rope_kv_rows(None, None, None, None, None, None, None, pos0, rows, 8, 2, 128, maxTokens, rope) == ERR_ARG
        assert lib.effort_attention_rows(None, None, None, None, pos0, rows, None, 8, 128, maxTokens) == ERR_ARG
    assert lib.effort_rope_kv_rows(None, None, None, None, None, None, None, 28, 4, 8, 3, 128, 32, rope) == ERR_SHAPE    # heads % kv heads
    assert lib.effort_attention_rows(None, None, None, None, 28, 4, None, 8, 96, 32) == ERR_SHAPE                       # head size
