"""Every extension header of csrc/kernels/, and the two the marching kernels share (march.h, row_segments.h), stands alone and includes what it uses: a translation unit of one line, the
header itself, passes hipcc -fsyntax-only for gfx950 with the library's flags (host and device pass), and the headers that
once reached a helper through a chain of unrelated families (scene.h -> stats.h -> frames.h -> dye.h -> diag.h) name
kernels/cells.h instead.  Needs hipcc, no GPU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = os.path.join(ROOT, "taichi-2d-vof_amd", "csrc", "kernels")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "-fPIC", "-Wall",
         "-Wno-unused-function"]          # FLAGS of csrc/Makefile
HEADERS = ["march.h", "row_segments.h", "reduce.h", "cells.h", "cg.h", "mg.h", "diag.h", "cell_rows.h", "interface.h", "blobs.h", "tracers.h", "depths.h", "dye.h", "frames.h", "stats.h",
           "scene.h"]


def includes(header):
    return re.findall(r'^#include "([^"]+)"', open(os.path.join(KERNELS, header)).read(), flags=re.M)


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
@pytest.mark.parametrize("header", HEADERS)
def test_header_compiles_alone(tmp_path, header):
    tu = tmp_path / ("only_" + header.replace(".h", ".hip"))
    tu.write_text('#include "%s"\n' % header)
    r = subprocess.run([HIPCC, *FLAGS, "-fsyntax-only", "-I", KERNELS, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("header", ["scene.h", "stats.h", "frames.h"])
def test_no_family_is_included_for_a_helper(header):
    assert not set(includes(header)) & {"stats.h", "frames.h", "dye.h", "diag.h"}, "%s includes %s" % (header, includes(header))


def test_the_shared_helpers_come_from_cells_h():
    for header in ("cg.h", "diag.h", "cell_rows.h", "interface.h", "depths.h", "blobs.h", "frames.h", "stats.h", "scene.h"):
        assert "cells.h" in includes(header), header
    for header in ("diag.h", "cell_rows.h", "interface.h", "depths.h"):
        assert "cg.h" not in includes(header), header
    assert includes("cells.h") == ["reduce.h"] and "tracers.h" in includes("depths.h")


def test_the_marching_helpers_come_from_march_h():
    assert includes("march.h") == ["common.h"] and includes("row_segments.h") == []
    for header in ("verbs.h", "momentum.h", "jacobi.h", "jacobi_pair.h", "transport.h", "fused_tm.h", "dye.h"):
        assert "march.h" in includes(header), header
    assert {"momentum.h", "transport.h", "row_segments.h"} <= set(includes("fused_tm.h")) and "row_segments.h" in includes("transport.h")
