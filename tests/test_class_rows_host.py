"""A plan's class-row tables (plan_class_rows, openr_amd/csrc/plan_host.cpp) on
the CPU, under AddressSanitizer and UBSan, with no device:
tests/host/class_rows_check.cpp derives them on a 19-node fabric, a complete
bipartite graph and a ring and checks that every closure row maps to a class
source of its own class, that the class sources are distinct classes, and that
the tables follow a class split after a patched neighbour set.  The program is
compiled into a temporary directory and run as a child process."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"


def test_class_rows_check_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "class_rows_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "class_rows_check.cpp"), str(CSRC / "plan_host.cpp"),
                    str(CSRC / "graph_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
