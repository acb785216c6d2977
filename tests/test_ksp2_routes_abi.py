"""Every source's KSP2_ED_ECMP routes (spf_ksp2_routes*, include/openr_spf.h) at
the C-ABI and in the Python wrappers: the symbols, their argument counts and
the refusal of a NULL plan.  Host only: no device needed."""

import re
from pathlib import Path

from openr_amd import _native as N
from openr_amd import engine, link_state

HEADER = Path(__file__).resolve().parents[1] / "include" / "openr_spf.h"
# name -> documented argument count
SYMBOLS = {"spf_ksp2_routes": 12, "spf_ksp2_routes_timing": 2, "spf_ksp2_route_db": 10,
           "spf_ksp2_route_buffers": 7}


def declared_args(text, name):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"spf_status\s+" + name + r"\s*\(([^;]*)\)\s*;", text, re.S)
    assert m, name
    return [a for a in (x.strip() for x in m.group(1).split(",")) if a]


def test_header_declares_and_library_exports():
    text = HEADER.read_text()
    for name, n_args in SYMBOLS.items():
        args = declared_args(text, name)
        assert len(args) == n_args, (name, args)
        assert re.match(r"(const\s+)?spf_ksp2_plan\s*\*", args[0]), (name, args[0])
        assert hasattr(N.lib, name), name
        res, argtypes = N.PROTOTYPES[name]
        assert len(argtypes) == n_args, name


def test_null_plan_is_refused():
    assert N.lib.spf_ksp2_routes(None, None, None, None, None, 0, None, None, None, None, None,
                                 None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_routes_timing(None, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_db(None, 0, None, None, 0, None, None, None, 0, None) == N.SPF_E_INVALID
    assert N.lib.spf_ksp2_route_buffers(None, None, None, None, None, None, None) == N.SPF_E_INVALID


def test_python_wrappers_exist():
    for name in ("routes", "routes_timing", "route_db", "route_buffers"):
        assert callable(getattr(engine.Ksp2Plan, name)), name
    assert callable(engine.SpfEngine.ksp2_routes)
    assert callable(engine.Ksp2Routes.nexthops)
    assert callable(link_state.LinkState.allSourcesKsp2Routes)
    assert callable(link_state.LinkState.allSourcesKsp2NextHops)
