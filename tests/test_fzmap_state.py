"""The zero-map bit of runtime/state.h (FieldState::fzmap_stale: who may have written F or its twin since the last k_tm batch that
keeps the maps) is plain C++: tests/host/fzmap_state_check.cpp holds every transition to the invariant stated there.  Compiled with
the host compiler, without HIP, and run -- once as it is and once under the address and undefined-behaviour sanitizers, as a
stand-alone binary."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler

SRC = os.path.join(ROOT, "tests", "host", "fzmap_state_check.cpp")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_fzmap_state(tmp_path, flags):
    exe = str(tmp_path / "fzmap_state_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
