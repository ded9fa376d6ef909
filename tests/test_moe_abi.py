"""CPU tests of the Mixtral routing entry points (effort_moe_route, effort_mix2_add, effort_dense_gemv_expert): declared in
include/effort_hip.h, bound in effort_amd._lib._SIGS with the argument kinds the header gives them, exported by the library, and
refusing a null context with a return code.  No compute calls -- there is no GPU here."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, I = "ptr", "int"
WANT = {
    "effort_moe_route": [P, P, P, P, I, I, P, P, P],
    "effort_mix2_add": [P, P, P, P, P, I],
    "effort_dense_gemv_expert": [P, P, P, P, P, I, I, I],
}


def _header_params(name):
    src = open(os.path.join(ROOT, "include", "effort_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    m = re.search(r"EFFORT_API\s+int\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name + " is not declared in include/effort_hip.h"
    return [P if "*" in p else [w for w in p.split() if w != "const"][0] for p in m.group(1).split(",")]


def test_header_declares_the_routing_entry_points():
    for name, kinds in WANT.items():
        assert _header_params(name) == kinds, name


def test_binding_has_the_routing_entry_points():
    from effort_amd import _lib
    for name, kinds in WANT.items():
        assert name in _lib._SIGS, name
        res, args = _lib._SIGS[name]
        assert res is C.c_int
        assert [P if a is C.c_void_p else {C.c_int: I}[a] for a in args] == kinds, name


def test_null_context_is_reported_not_crashed(hip_lib_built):
    import effort_amd
    lib = effort_amd.lib()
    assert lib.effort_moe_route(None, None, None, None, 4096, 8, None, None, None) == -1
    assert lib.effort_mix2_add(None, None, None, None, None, 4096) == -1
    assert lib.effort_dense_gemv_expert(None, None, None, None, None, 4096, 4096, 8) == -1
