"""The cells a handle reports (runtime/rows.h) and the arenas of the verbs cut into ranges (runtime/carve.h) are plain C++:
tests/host/buffers_check.cpp holds them to the expressions the runtime used before, over grids, both dtypes, strips and
strips that own nothing -- compiled with the host compiler, without HIP, and run as a stand-alone binary, once as it is and
once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_reported_rows_and_arena_layouts(tmp_path, flags):
    exe = str(tmp_path / "buffers_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "host", "buffers_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
