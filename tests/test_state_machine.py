"""runtime/state.h (what a handle's fields and ghost cells hold: a field written from outside, the verbs, the prologue and
epilogue of a step, the phase order) is plain C++: tests/host/state_check.cpp holds it, over every combination of the flags, to
the expressions the runtime held before, restated literally.  Compiled with the host compiler, without HIP, and run -- once as it
is and once under the address and undefined-behaviour sanitizers, as a stand-alone binary."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler

SRC = os.path.join(ROOT, "tests", "host", "state_check.cpp")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_state_machine(tmp_path, flags):
    exe = str(tmp_path / "state_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
