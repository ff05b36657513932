"""Writes tests/golden/curvature/curv_96x130_f64.npz (a directory of its own: tests/test_golden.py replays every *.npz beside this script): the rows and the summary of vof_curvature on the 96 x 130 bubble (-ic 3, Ly = 0.13, f64) after
20 steps, as bytes to hold later libraries to (tests/test_energy_gpu.py: KAPPA_CSF moved into a helper that k_energy shares).  Needs a GPU.

    python tests/golden/make_curv_golden.py [LIBRARY.so [OUT.npz]]

LIBRARY.so: a libvof2d_hip.so built from the commit whose bytes are to be recorded (default: the one in the tree); a library from before
vof_energy lacks those two symbols, which this script does not need.
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "tests")]

from vof2d import _abi, _lib, curvature          # noqa: E402
from vof2d.engine import Engine, make_desc      # noqa: E402

if __name__ == "__main__":
    lib = sys.argv[1] if len(sys.argv) > 1 else _lib.LIB_PATH
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "curvature", "curv_96x130_f64.npz")
    api = _abi.bind(ctypes.CDLL(lib, mode=ctypes.RTLD_GLOBAL), "vof_", optional=("energy", "step_energy"))
    e = Engine(api, make_desc(api, 96, 130, "f64", "f32", Lx=0.1, Ly=0.13))
    e.set_init_F(3)
    e.step(20)
    rows, summ = e.curvature()
    np.savez_compressed(out, rows=rows, summary=np.array([summ[k] for k in curvature.SUMMARY], dtype=np.float64))
    print("wrote %s: %d rows, summary %r" % (out, len(rows), summ))
