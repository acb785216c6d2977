"""The exactly sized route-database pool (SPF_ROUTE_COMPACT, include/openr_spf.h)
at the C-ABI: the flag's value, the two functions that report on and hand out
the record pools of the last spf_mplan_route_records.  Host only: no device
needed."""

import re
from pathlib import Path

from openr_amd import _native as N

HEADER = Path(__file__).resolve().parents[1] / "include" / "openr_spf.h"
NEW_SYMBOLS = ("spf_mplan_route_record_pool", "spf_mplan_route_record_buffers")


def test_flag_value():
    assert N.SPF_ROUTE_COMPACT == 2
    assert N.SPF_ROUTE_COMPACT & N.SPF_ROUTE_LFA == 0
    text = HEADER.read_text()
    m = re.search(r"#define\s+SPF_ROUTE_COMPACT\s+(\S+)", text)
    assert m and int(m.group(1).rstrip("uU"), 0) == 2


def test_header_declares_and_library_exports():
    text = HEADER.read_text()
    for name in NEW_SYMBOLS:
        assert re.search(r"spf_status\s+" + name + r"\s*\(\s*spf_mplan\s*\*", text), name
        assert hasattr(N.lib, name), name


def test_null_plan_is_refused():
    assert N.lib.spf_mplan_route_record_pool(None, None, None, None) == N.SPF_E_INVALID
    assert N.lib.spf_mplan_route_record_buffers(None, 0, None, None, None, None, None, 0, None) == N.SPF_E_INVALID
