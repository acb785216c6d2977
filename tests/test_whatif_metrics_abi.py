"""The metric plans' C ABI without a device: both entry points and the kind are
declared in include/openr_spf.h, exported by the library and bound in Python,
and NULL arguments are refused with the outputs untouched."""

import ctypes as C
import re
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
NAMES = ("spf_whatif_plan_create_metrics", "spf_whatif_plan_metrics")


def test_declared_exported_and_bound():
    from openr_amd import _native as N
    from openr_amd.engine import WHATIF_KINDS

    text = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "openr_spf.h").read_text(), flags=re.S)
    lib = C.CDLL(str(N.LIB_PATH))
    for name in NAMES:
        assert re.search(r"\bspf_status\s+" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in N.PROTOTYPES
    assert re.search(r"#define\s+SPF_WHATIF_LINK_METRIC\s+4u", text)
    assert re.search(r"#define\s+SPF_WHATIF_METRIC_KEEP\s+0u", text)
    assert N.SPF_WHATIF_LINK_METRIC == 4 and N.SPF_WHATIF_METRIC_KEEP == 0
    assert WHATIF_KINDS["metric"] == 4 and sorted(WHATIF_KINDS.values()) == [0, 1, 2, 3, 4]


def test_null_arguments():
    from openr_amd import _native as N

    h = C.c_void_p(0x1234)
    a = np.ones(2, np.uint32)
    st = N.lib.spf_whatif_plan_create_metrics(None, 0, N.ptr(a), N.ptr(a), N.ptr(a), 2, C.byref(h))
    assert st == N.SPF_E_INVALID and h.value == 0x1234  # no ctx: *out untouched
    st = N.lib.spf_whatif_plan_create_metrics(None, 0, N.ptr(a), N.ptr(a), N.ptr(a), 2, None)
    assert st == N.SPF_E_INVALID
    a[:] = 77
    assert N.lib.spf_whatif_plan_metrics(None, N.ptr(a), N.ptr(a), N.ptr(a)) == N.SPF_E_INVALID
    assert list(a) == [77, 77]
