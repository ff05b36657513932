"""runtime/rows.h (a strip's owned rows, edge bands and rest; which of them a launch of one part gets) and the tile
geometry of vof2d_device.h (halo, stride and tile count per kernel family) are plain C++: tests/host/rows_geometry_check.cpp
is compiled with the host compiler, without HIP, and run -- once as it is and once under the address and undefined-behaviour
sanitizers, as a stand-alone binary."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "taichi-2d-vof_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "host", "rows_geometry_check.cpp")


def host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return cxx
    raise RuntimeError("no host C++ compiler found")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_rows_and_tile_geometry(tmp_path, flags):
    exe = str(tmp_path / "rows_geometry_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
