"""The multi-device plans' host arithmetic (openr_amd/csrc/partition_host.cpp:
the source partition, the label groups, a route delta's label union) on the
CPU, under AddressSanitizer and UBSan, with no device:
tests/host/partition_host_check.cpp pins the partition of a 19-node fabric, a
grid, a star, a graph with an isolated node and a source subset in all three
modes (1, 2, 3 and n_src + 1 parts), and the label groups, to what
spf_partition_sources and spf_label_groups answered before their bodies moved
there, and checks the label union against expectations written by hand.  The
program is compiled into a temporary directory and run as a child process."""

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "openr_amd" / "csrc"


def test_partition_host_check_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = tmp_path / "partition_host_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(ROOT / "tests" / "host" / "partition_host_check.cpp"),
                    str(CSRC / "partition_host.cpp"), "-o", str(exe)], check=True)
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
