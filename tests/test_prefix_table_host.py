"""The prefix table of spf_mplan_prefix_routes
(openr_amd/csrc/prefix_table_host.cpp) on the CPU, under AddressSanitizer and
UBSan, with no device: tests/host/prefix_table_check.cpp checks the table's
refusals (each names its prefix), the ranks the device compares instead of
PrefixMetrics tuples, and the CPU restatement of the per-me selection on cases
written by hand -- the (0, 0, 0) floor, a preference tie broken by distance,
all / some / me drained, min_nexthop taken from the selected entries only.
The program is compiled into a temporary directory and run as a child
process."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"


def test_prefix_table_check_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "prefix_table_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "prefix_table_check.cpp"),
                    str(CSRC / "prefix_table_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
