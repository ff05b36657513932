"""runtime/groups.h (step_groups: the loop of every vof_step_<verb> -- steps in groups, something behind every group, the
remainder; the first failure ends it) is plain C++: tests/host/step_groups_check.cpp is compiled with the host compiler,
without HIP, and run -- once as it is and once under the address and undefined-behaviour sanitizers, as a stand-alone binary."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler

SRC = os.path.join(ROOT, "tests", "host", "step_groups_check.cpp")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_step_groups_trace_and_first_failure(tmp_path, flags):
    exe = str(tmp_path / "step_groups_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
