"""What vof_depths lays out on the host is plain C++ (runtime/rows.h: the chunk rule, the partial counts, the launch sizes;
runtime/carve.h: carve_depths): tests/host/depths_check.cpp holds it to the expressions written out there, over grids, both
dtypes, strips and strips that own nothing -- compiled with the host compiler, without HIP, and run as a stand-alone binary,
once as it is and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_depths_chunk_rule_partials_and_arena(tmp_path, flags):
    exe = str(tmp_path / "depths_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "host", "depths_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
