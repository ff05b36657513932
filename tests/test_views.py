"""runtime/views.h (which buffer each field id names, the four swaps that change it, and the store of the graphs captured against
a view) is plain C++: tests/host/views_check.cpp holds the views, over every sequence of up to six swaps, to the pointer
comparisons the runtime made before, restated literally, and the store to its contract with a destroy functor that counts.
Compiled with the host compiler, without HIP, and run -- once as it is and once under the address and undefined-behaviour
sanitizers, as a stand-alone binary."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler

SRC = os.path.join(ROOT, "tests", "host", "views_check.cpp")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_views_and_graph_store(tmp_path, flags):
    exe = str(tmp_path / "views_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
