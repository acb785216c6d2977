"""The device-free part of the what-if list pools' _db calls
(openr_amd/csrc/whatif_pool_host.cpp: pool_slice, pool_order) without a device:
compiled with its check program into a temporary directory and run as a child
process under the sanitizers, as the plan host tables are."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"


def test_slice_checks_and_order_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "whatif_pool_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{CSRC}", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "host" / "whatif_pool_host_check.cpp"),
                    str(CSRC / "whatif_pool_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
