"""The C-ABI library loads and exports every function include/*.h declares
(no device needed: nothing is computed)."""

import ctypes
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def declared_functions():
    names = set()
    for h in sorted((ROOT / "include").glob("*.h")):
        text = re.sub(r"/\*.*?\*/", "", h.read_text(), flags=re.S)
        for m in re.finditer(r"^\s*[A-Za-z_][\w\s\*]*?\b([a-z][a-z0-9_]*)\s*\(", text, re.M):
            name = m.group(1)
            if name in ("if", "defined", "sizeof"):
                continue
            names.add(name)
    return names


def test_headers_declare_expected_entry_points():
    names = declared_functions()
    for must in ("spf_ctx_create", "spf_graph_load", "spf_plan_execute", "spf_solve",
                 "spf_sssp", "spf_preds", "ls_create", "ls_update_adjacency_databases",
                 "ls_get_spf_result", "ls_get_kth_paths"):
        assert must in names


def test_library_exports_every_declared_symbol():
    from openr_amd import _native

    lib = ctypes.CDLL(str(_native.LIB_PATH))
    missing = [n for n in sorted(declared_functions()) if not hasattr(lib, n)]
    assert not missing, missing
    # the Python binding declares a prototype for each of them
    assert declared_functions() <= set(_native.PROTOTYPES), (
        declared_functions() - set(_native.PROTOTYPES))


def test_ksp2_plan_info_layout_and_null_arguments():
    """spf_ksp2_plan_info: the binding's struct and kind names follow the
    header, and a NULL plan or a NULL output is refused with *out untouched."""
    from openr_amd import _native as N
    from openr_amd import engine

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "openr_spf.h").read_text(), flags=re.S)
    body = re.search(r"struct\s+spf_ksp2_plan_info\s*\{(.*?)\}\s*;", text, re.S).group(1)
    fields = re.findall(r"(uint32_t|uint64_t)\s+(\w+)\s*;", body)
    ctype = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64}
    assert [(n, ctype[t]) for t, n in fields] == list(N.SpfKsp2PlanInfo._fields_)
    assert ctypes.sizeof(N.SpfKsp2PlanInfo) == 32
    kinds = dict(re.findall(r"SPF_KSP2_KIND_(\w+)\s*=\s*(\d+)", text))
    assert [k for k, _ in sorted(kinds.items(), key=lambda kv: int(kv[1]))] == list(N.KSP2_KIND_NAMES)
    assert sorted(int(v) for v in kinds.values()) == [0, 1, 2, 3]

    x = N.SpfKsp2PlanInfo()
    ctypes.memset(ctypes.byref(x), 0xAB, ctypes.sizeof(x))
    before = bytes(x)
    assert N.lib.spf_ksp2_plan_info(None, ctypes.byref(x)) == N.SPF_E_INVALID
    assert bytes(x) == before
    assert N.lib.spf_ksp2_plan_info(None, None) == N.SPF_E_INVALID
    assert callable(engine.Ksp2Plan.info)
    assert [f.name for f in engine.Ksp2PlanInfo.__dataclass_fields__.values()] == [n for _, n in fields]


def test_no_device_is_reported_not_faked():
    """Without a GPU the engine refuses loudly instead of falling back."""
    from helpers import gpu_visible

    if gpu_visible():
        return
    from openr_amd import _native as N

    h = ctypes.c_void_p()
    st = N.lib.spf_ctx_create(0, ctypes.byref(h))
    assert st == N.SPF_E_NO_DEVICE
    assert N.global_error()
