"""What vof_frame lays out on the host is plain C++ (runtime/rows.h: frame_geom -- pw, ph, the chunk rule, the launch sizes;
runtime/carve.h: carve_frame): tests/host/frames_check.cpp holds it to the expressions written out there, over many (nx, ny,
bx, by), blocks larger than the grid and blocks that do not divide it included -- compiled with the host compiler, without
HIP, and run as a stand-alone binary, once as it is and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_frame_geometry_chunk_rule_and_arena(tmp_path, flags):
    exe = str(tmp_path / "frames_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "host", "frames_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
