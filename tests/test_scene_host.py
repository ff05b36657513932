"""What vof_set_scene does on the host before anything reaches the device is plain C++ (runtime/scene.h: scene_check, scene_pack):
tests/host/scene_check.cpp holds it to every refusal include/vof2d.h lists and to the longest list -- compiled with the host
compiler, without HIP, and run as a stand-alone binary, once as it is and once under the address and undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

from test_rows_geometry import CSRC, ROOT, host_compiler


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_scene_check_refuses_and_packs(tmp_path, flags):
    exe = str(tmp_path / "scene_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "host", "scene_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
