"""KSP2 route databases: snapshot, delta and update payload
(spf_ksp2_route_snapshot / _delta / _update and their companions,
include/openr_spf.h) at the C-ABI and in the Python wrappers: the symbols,
their argument counts and the refusal of NULL plans and NULL snapshots.  Host
only: no device needed."""

import ctypes as C
import re
from pathlib import Path

import numpy as np

from openr_amd import _native as N
from openr_amd import engine, link_state

HEADER = Path(__file__).resolve().parents[1] / "include" / "openr_spf.h"
# name -> (return type, documented argument count)
SYMBOLS = {
    "spf_ksp2_route_snapshot": ("spf_status", 4),
    "spf_ksp2_route_snapshot_destroy": ("void", 1),
    "spf_ksp2_route_snapshot_bytes": ("uint64_t", 1),
    "spf_ksp2_route_delta": ("spf_status", 6),
    "spf_ksp2_route_delta_db": ("spf_status", 5),
    "spf_ksp2_route_delta_buffers": ("spf_status", 4),
    "spf_ksp2_route_delta_timing": ("spf_status", 2),
    "spf_ksp2_route_update": ("spf_status", 4),
    "spf_ksp2_route_update_db": ("spf_status", 10),
    "spf_ksp2_route_update_read": ("spf_status", 8),
    "spf_ksp2_route_update_buffers": ("spf_status", 7),
}


def declared_args(text, ret, name):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(ret + r"\s+" + name + r"\s*\(([^;]*)\)\s*;", text, re.S)
    assert m, name
    return [a for a in (x.strip() for x in m.group(1).split(",")) if a]


def test_header_declares_and_library_exports():
    text = HEADER.read_text()
    for name, (ret, n_args) in SYMBOLS.items():
        args = declared_args(text, ret, name)
        assert len(args) == n_args, (name, args)
        first = r"(const\s+)?spf_ksp2_snapshot\s*\*" if "snapshot_" in name else r"(const\s+)?spf_ksp2_plan\s*\*"
        assert re.match(first, args[0]), (name, args[0])
        assert hasattr(N.lib, name), name
        res, argtypes = N.PROTOTYPES[name]
        assert len(argtypes) == n_args, name
        assert (res is None) == (ret == "void"), name


def test_null_plan_is_refused():
    lh = np.zeros(4, np.uint64)
    out = C.c_void_p()
    assert N.lib.spf_ksp2_route_snapshot(None, N.ptr(lh, C.c_uint64), 4, C.byref(out)) == N.SPF_E_INVALID
    assert not out.value
    fake = C.c_void_p(1)  # never dereferenced: the NULL plan is refused first
    assert N.lib.spf_ksp2_route_delta(None, fake, N.ptr(lh, C.c_uint64), 4, None, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_delta(None, None, N.ptr(lh, C.c_uint64), 4, None, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_delta_db(None, 0, None, 0, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_delta_buffers(None, None, None, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_delta_timing(None, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_update(None, None, None, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_update_db(None, 0, None, None, 0, None, None, None, 0, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_update_read(None, None, None, None, None, None, None, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_update_buffers(None, None, None, None, None, None, None) == N.SPF_E_INVALID


def test_null_snapshot_is_harmless():
    N.lib.spf_ksp2_route_snapshot_destroy(None)
    assert N.lib.spf_ksp2_route_snapshot_bytes(None) == 0


def test_python_wrappers_exist():
    for name in ("route_snapshot", "route_delta", "route_delta_db", "route_delta_timing", "route_update",
                 "route_update_db", "route_update_buffers"):
        assert callable(getattr(engine.Ksp2Plan, name)), name
    assert callable(engine.Ksp2Routes.snapshot) and callable(engine.Ksp2Routes.delta)
    assert issubclass(engine.Ksp2RouteSnapshot, N.NativeHandle)
    assert engine.Ksp2RouteSnapshot._destroy == "spf_ksp2_route_snapshot_destroy"
    for name in ("allSourcesKsp2RouteSnapshot", "allSourcesKsp2RouteDelta", "allSourcesKsp2RouteUpdate"):
        assert callable(getattr(link_state.LinkState, name)), name
