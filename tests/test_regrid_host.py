"""What vof_regrid decides on the host before anything reaches the device is plain C++ (runtime/regrid_check.h: regrid_factors,
regrid_check): tests/host/regrid_check.cpp holds it to a search over all factor pairs and to every refusal include/vof2d.h lists --
compiled with the host compiler, without HIP, and run as a stand-alone binary, once as it is and once under the address and
undefined-behaviour sanitizers.  Beside it: kernels/regrid.h stands alone under the library's flags and includes cells.h and
interface.h only; a null handle is refused without a GPU."""
import os
import subprocess

import pytest

from test_kernel_headers import FLAGS, HIPCC, KERNELS, includes
from test_rows_geometry import CSRC, ROOT, host_compiler
from vof2d import _abi


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_regrid_check_finds_the_factors_and_refuses(tmp_path, flags):
    exe = str(tmp_path / "regrid_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "host", "regrid_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


@pytest.mark.skipif(HIPCC is None, reason="hipcc is not installed")
def test_regrid_header_compiles_alone(tmp_path):
    tu = tmp_path / "only_regrid.hip"
    tu.write_text('#include "regrid.h"\n')
    r = subprocess.run([HIPCC, *FLAGS, "-fsyntax-only", "-I", KERNELS, str(tu)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert includes("regrid.h") == ["cells.h", "interface.h"]


def test_null_handles_are_refused_without_a_gpu(hip_api):
    assert hip_api.regrid(None, None, 0, 0.0, None) == _abi.VOF_EINVAL
    assert hip_api.regrid(None, None, _abi.VOF_REGRID_PLIC, 1e-6, (_abi.C.c_double * _abi.VOF_REGRID_SUM_N)()) == _abi.VOF_EINVAL


def test_the_python_constants_are_the_headers():
    txt = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    for name in ("VOF_REGRID_PLIC", "VOF_REGRID_MAX_FACTOR", "VOF_REGRID_SUM_RX", "VOF_REGRID_SUM_RY", "VOF_REGRID_SUM_DIR", "VOF_REGRID_SUM_PLIC_CELLS",
                 "VOF_REGRID_SUM_DEGENERATE", "VOF_REGRID_SUM_F_SRC", "VOF_REGRID_SUM_F_DST", "VOF_REGRID_SUM_ISTEP", "VOF_REGRID_SUM_N"):
        assert "#define %s %d\n" % (name, getattr(_abi, name)) in txt, name
