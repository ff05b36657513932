"""kernels/row_segments.h (the row segments of a k_tm or k_transport launch: which chunk of which segment a pair or wave takes, and
how many the launch needs) is plain C++ shared by the kernels' entries and the host's chunk count: tests/host/row_segments_check.cpp is compiled
with the host compiler, without HIP, and run -- once as it is and once under the address and undefined-behaviour sanitizers,
as a stand-alone binary."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taichi-2d-vof_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "row_segments_check.cpp")


def host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    raise RuntimeError("no host C++ compiler found")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_row_segments_mapping(tmp_path, flags):
    exe = str(tmp_path / "row_segments_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
