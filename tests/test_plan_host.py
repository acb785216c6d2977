"""A plan's host tables (openr_amd/csrc/plan_host.cpp) on the CPU, under
AddressSanitizer and UBSan, with no device: tests/host/plan_host_check.cpp
derives them for small graphs built in code and checks the contract the sliced
next-hop kernel relies on (every source, neighbour position and chunk in
exactly one work unit, ...) and that every table is word for word what
build_plan uploaded before the derivations moved out of it.  The program is
compiled into a temporary directory and run as a child process."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"


def test_plan_host_check_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "plan_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "plan_host_check.cpp"), str(CSRC / "plan_host.cpp"),
                    str(CSRC / "graph_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
