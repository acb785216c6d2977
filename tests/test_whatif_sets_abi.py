"""The set plans' C ABI without a device: both entry points are declared in
include/openr_spf.h, exported by the library and bound in Python, and NULL
arguments are refused with the outputs untouched."""

import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("spf_whatif_plan_create_sets", "spf_whatif_plan_sets")


def test_declared_exported_and_bound():
    from openr_amd import _native as N

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "openr_spf.h").read_text(), flags=re.S)
    lib = C.CDLL(str(N.LIB_PATH))
    for name in NAMES:
        assert re.search(r"\bspf_status\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in N.PROTOTYPES
    assert re.search(r"#define\s+SPF_WHATIF_LINK_SET\s+3u", text)
    assert N.SPF_WHATIF_LINK_SET == 3


def test_null_arguments():
    from openr_amd import _native as N

    h = C.c_void_p(0x1234)
    ptr = np.zeros(2, np.uint32)
    st = N.lib.spf_whatif_plan_create_sets(None, 0, N.ptr(ptr), None, 1, C.byref(h))
    assert st == N.SPF_E_INVALID and h.value == 0x1234  # no ctx: *out untouched
    assert N.lib.spf_whatif_plan_create_sets(None, 0, N.ptr(ptr), None, 1, None) == N.SPF_E_INVALID
    ptr[:] = 77
    assert N.lib.spf_whatif_plan_sets(None, N.ptr(ptr), None) == N.SPF_E_INVALID
    assert list(ptr) == [77, 77]
