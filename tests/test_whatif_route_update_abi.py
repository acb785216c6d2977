"""The what-if route updates' C ABI without a device: the entry points are
declared in include/openr_spf.h with the arguments the Python prototypes bind,
exported by the library, and a NULL plan is refused with the outputs
untouched."""

import ctypes as C
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
# name -> the header's parameter types, pointers as the prototypes spell them
DECLARED = {
    "spf_whatif_route_update": ["spf_whatif_plan*", "uint64_t*", "uint64_t*", "uint64_t*", "double*",
                                "void*"],
    "spf_whatif_route_update_db": ["spf_whatif_plan*", "uint32_t", "uint32_t*", "uint64_t*", "uint64_t*",
                                   "uint64_t*", "uint64_t", "uint64_t", "uint64_t*", "uint64_t*"],
    "spf_whatif_route_update_read": ["spf_whatif_plan*", "uint64_t*", "uint32_t*", "uint64_t*",
                                     "uint64_t*", "uint64_t*"],
    "spf_whatif_route_update_buffers": ["spf_whatif_plan*", "const uint64_t**", "const uint32_t**",
                                        "const uint64_t**", "const uint64_t**", "const uint64_t**",
                                        "uint64_t*", "uint64_t*"],
    "spf_whatif_route_update_base": ["spf_whatif_plan*", "uint64_t*", "uint64_t*"],
    "spf_whatif_route_update_timing": ["const spf_whatif_plan*", "double*"],
    "spf_whatif_route_update_stats": ["spf_whatif_plan*", "uint32_t*", "uint64_t*"],
}


def ctype_of(decl):
    from openr_amd import _native as N

    decl = decl.replace("const ", "")
    return {"spf_whatif_plan*": N._vp, "void*": N._vp, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "uint32_t*": N._u32p, "uint64_t*": N._u64p, "double*": C.POINTER(C.c_double),
            "uint32_t**": C.POINTER(N._vp), "uint64_t**": C.POINTER(N._vp)}[decl]


def test_declared_exported_and_bound():
    from openr_amd import _native as N

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "openr_spf.h").read_text(), flags=re.S)
    lib = C.CDLL(str(N.LIB_PATH))
    for name, want in DECLARED.items():
        m = re.search(r"\bspf_status\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(1).split(",")]
        assert params == want, (name, params)
        assert hasattr(lib, name), name
        res, args = N.PROTOTYPES[name]
        assert res is C.c_int and args == [ctype_of(d) for d in want], name
    from openr_amd import engine

    assert callable(engine.WhatIfRoutes.update) and callable(engine.SpfEngine.whatif_route_update)
    for method in ("of", "base", "timing"):
        assert callable(getattr(engine.WhatIfRouteUpdate, method))
    # the constants the GPU tests cross come from the code
    assert N.lib.spf_whatif_scan_tile() >= 1024 and N.lib.spf_whatif_route_update_sweep_sets() >= 64
    for name in ("spf_whatif_route_update_lds_slots", "spf_whatif_route_update_sweep_sets",
                 "spf_whatif_scan_tile"):
        m = re.search(r"\buint32_t\s+" + name + r"\s*\(\s*void\s*\)\s*;", text)
        assert m and hasattr(lib, name) and N.PROTOTYPES[name] == (C.c_uint32, []), name
    # a staged slot is 16 bytes, and a workgroup may take 64 KB of LDS
    assert 64 <= N.lib.spf_whatif_route_update_lds_slots() <= 4096


def test_null_plan_is_invalid():
    from openr_amd import _native as N

    n, w, ms = C.c_uint64(0xAB), C.c_uint32(0xAB), (C.c_double * 7)(*[7] * 7)
    u = N.lib
    assert u.spf_whatif_route_update(None, C.byref(n), C.byref(n), C.byref(n), ms, None) == N.SPF_E_INVALID
    assert b"NULL plan" in u.spf_global_error()
    assert u.spf_whatif_route_update_db(None, 0, None, None, None, None, 0, 0, C.byref(n),
                                        C.byref(n)) == N.SPF_E_INVALID
    assert u.spf_whatif_route_update_read(None, C.byref(n), None, None, None, None) == N.SPF_E_INVALID
    assert u.spf_whatif_route_update_buffers(None, None, None, None, None, None, C.byref(n),
                                             C.byref(n)) == N.SPF_E_INVALID
    assert u.spf_whatif_route_update_base(None, C.byref(n), None) == N.SPF_E_INVALID
    assert u.spf_whatif_route_update_timing(None, ms) == N.SPF_E_INVALID
    assert u.spf_whatif_route_update_stats(None, C.byref(w), C.byref(n)) == N.SPF_E_INVALID
    assert n.value == 0xAB and w.value == 0xAB and list(ms) == [7] * 7  # outputs untouched
