"""The C ABI of what-if impact by destination without a device: the entry
points are declared in include/openr_spf.h with the arguments the Python
prototypes bind, exported by the library, the summary is the 32-byte struct
both sides agree on, and a NULL plan is refused with the outputs untouched."""

import ctypes as C
import re
from pathlib import Path

import numpy as np

import whatif_impact as I

ROOT = Path(__file__).resolve().parents[1]
PER_FLAVOUR = {
    "": ["spf_whatif_plan*", "uint64_t*", "uint64_t*", "double*", "void*"],
    "_impact": ["spf_whatif_plan*", "spf_whatif_impact*"],
    "_db": ["spf_whatif_plan*", "uint32_t", "uint32_t*", "uint64_t*", "uint64_t", "uint64_t*"],
    "_read": ["spf_whatif_plan*", "uint64_t*", "uint32_t*", "uint64_t*", "spf_whatif_impact*"],
    "_buffers": ["spf_whatif_plan*", "const uint64_t**", "const uint32_t**", "const uint64_t**",
                 "const spf_whatif_impact**", "uint32_t*", "uint64_t*"],
}
# name -> the header's parameter types, pointers as the prototypes spell them
DECLARED = {f"spf_whatif_by_{flavour}{call}": args
            for flavour in ("node", "set") for call, args in PER_FLAVOUR.items()}
DECLARED["spf_whatif_impact_timing"] = ["const spf_whatif_plan*", "uint32_t", "double*"]


def header():
    return re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "openr_spf.h").read_text(), flags=re.S)


def ctype_of(decl):
    from openr_amd import _native as N

    decl = decl.replace("const ", "")
    return {"spf_whatif_plan*": N._vp, "void*": N._vp, "spf_whatif_impact*": N._vp,
            "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
            "uint32_t*": N._u32p, "uint64_t*": N._u64p, "double*": C.POINTER(C.c_double),
            "uint32_t**": C.POINTER(N._vp), "uint64_t**": C.POINTER(N._vp),
            "spf_whatif_impact**": C.POINTER(N._vp)}[decl]


def test_declared_exported_and_bound():
    from openr_amd import _native as N

    text = header()
    lib = C.CDLL(str(N.LIB_PATH))
    assert len(DECLARED) == 11
    for name, want in DECLARED.items():
        m = re.search(r"\bspf_status\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
        assert m, name
        params = [re.sub(r"\s*\w+$", "", " ".join(p.split())) for p in m.group(1).split(",")]
        assert params == want, (name, params)
        assert hasattr(lib, name), name
        res, args = N.PROTOTYPES[name]
        assert res is C.c_int and args == [ctype_of(d) for d in want], name
    from openr_amd import engine

    assert callable(engine.WhatIfChanges.by_node) and callable(engine.WhatIfRoutes.by_set)
    assert callable(engine.SpfEngine.whatif_impact)
    assert callable(engine.WhatIfImpact.of) and callable(engine.WhatIfImpact.timing)


def test_the_summary_is_32_bytes_on_both_sides():
    from openr_amd import engine

    text = header()
    body = re.search(r"typedef\s+struct\s+spf_whatif_impact\s*\{(.*?)\}\s*spf_whatif_impact\s*;", text,
                     re.S).group(1)
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+)\s*;", body)
    kind = {"uint32_t": "<u4", "uint64_t": "<u8"}
    for dtype in (engine.IMPACT_DTYPE, I.DTYPE):
        assert dtype.itemsize == 32
        assert [(n, dtype.fields[n][0].str) for n in dtype.names] == [(n, kind[t]) for t, n in fields]
        assert dtype.fields["max_metric"][1] == 16 and dtype.fields["max_fail"][1] == 24
    assert int(re.search(r"#define\s+SPF_WHATIF_NONE\s+(\w+)", text).group(1).rstrip("u"), 16) \
        == engine.WHATIF_NONE == I.NONE
    which = dict(re.findall(r"#define\s+SPF_WHATIF_BY_(NODE|SET)\s+(\d+)u", text))
    assert which == {"NODE": "0", "SET": "1"}


def test_null_plan_is_invalid():
    from openr_amd import _native as N

    n, k, ms = C.c_uint64(0xAB), C.c_uint32(0xAB), (C.c_double * 3)(7, 7, 7)
    out = np.full(2, 0xAB, np.uint8).repeat(32).view(I.DTYPE)
    before = out.tobytes()
    mem = C.c_void_p(out.ctypes.data)
    for flavour in ("node", "set"):
        call = lambda name: getattr(N.lib, f"spf_whatif_by_{flavour}{name}")
        assert call("")(None, C.byref(n), C.byref(n), ms, None) == N.SPF_E_INVALID
        assert b"NULL plan" in N.lib.spf_global_error()
        assert call("_impact")(None, mem) == N.SPF_E_INVALID
        assert call("_db")(None, 0, C.byref(k), C.byref(n), 1, C.byref(n)) == N.SPF_E_INVALID
        assert call("_read")(None, C.byref(n), C.byref(k), C.byref(n), mem) == N.SPF_E_INVALID
        assert call("_buffers")(None, None, None, None, None, C.byref(k), C.byref(n)) == N.SPF_E_INVALID
        assert b"NULL plan" in N.lib.spf_global_error()
    for which in (0, 1, 2):
        assert N.lib.spf_whatif_impact_timing(None, which, ms) == N.SPF_E_INVALID
    assert b"NULL plan" in N.lib.spf_global_error()
    assert n.value == 0xAB and k.value == 0xAB and list(ms) == [7, 7, 7]  # outputs untouched
    assert out.tobytes() == before
