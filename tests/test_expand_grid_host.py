"""plan_expand_grid (openr_amd/csrc/plan_host.cpp), the expansion kernel's
grid, on the CPU under AddressSanitizer and UBSan, with no device:
tests/host/expand_grid_check.cpp checks that the workgroups' ranges cover every
row and every piece of the width exactly once for rows in {1, 7, 8, 9, 200,
9976}, widths in {32, 1024, 1056, 2208, 2240, 9984, 10240} and 1 or 256 CUs.
The program is compiled into a temporary directory and run as a child process."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"


def test_expand_grid_check_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "expand_grid_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "expand_grid_check.cpp"), str(CSRC / "plan_host.cpp"),
                    str(CSRC / "graph_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
