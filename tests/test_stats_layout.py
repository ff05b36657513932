"""What vof_stats_begin lays out on the host is plain C++ (runtime/carve.h: stats_pitch, carve_stats): tests/host/stats_check.cpp
holds the ranges of the accumulator planes to what is written out there over many grids, the three masks and both dtypes --
disjoint, aligned to 16 bytes, inside the total, every lane's vector inside its row -- compiled with the host compiler, without
HIP, and run as a stand-alone binary, once as it is and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_stats_planes_are_disjoint_aligned_and_inside(tmp_path, flags):
    exe = str(tmp_path / "stats_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "host", "stats_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
