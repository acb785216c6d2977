"""The graph's host state (openr_amd/csrc/graph_host.cpp) on the CPU, under
AddressSanitizer and UBSan, with no device: tests/host/graph_host_check.cpp
builds small graphs in code and checks that row patches leave every derived
table equal to a fresh load's, and that a refused patch changes nothing.  The
program is compiled into a temporary directory and run as a child process."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"


def test_graph_host_check_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "graph_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "graph_host_check.cpp"), str(CSRC / "graph_host.cpp"),
                    "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
