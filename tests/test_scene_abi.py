"""vof_set_scene at the C boundary, without a GPU: the constants of include/vof2d.h and of vof2d/_abi.py agree, the symbol is
bound with its signature, and a null handle is refused before anything is touched."""
import ctypes as C
import os
import re

import numpy as np

from vof2d import _abi, scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_of_the_header_equal_the_bindings():
    txt = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define (VOF_(?:SHAPE|SCENE)_[A-Z0-9_]+) (\d+)\s*$", txt, flags=re.M)}
    assert len(defs) == 18 and defs["VOF_SCENE_MAX_SHAPES"] == 1024 and defs["VOF_SCENE_SUM_N"] == 8 and defs["VOF_SHAPE_N"] == 8
    for name, value in defs.items():
        assert getattr(_abi, name) == value, name
    assert sorted(n for n in dir(_abi) if n.startswith(("VOF_SHAPE_", "VOF_SCENE_"))) == sorted(defs)
    assert scene.SUMMARY == ("SHAPES", "SAMPLES", "PAINTED", "MIXED", "ISTEP") and scene.PHASES == {"gas": 0, "liquid": 1}
    assert "set_scene" in _abi.SIGNATURES and "set_scene" in _abi.GPU_ONLY


def test_a_null_handle_is_refused(hip_api):
    recs = scene.pack([scene.disc(0.05, 0.05, 0.01, "liquid")])
    summ = (C.c_double * _abi.VOF_SCENE_SUM_N)(*([-7.0] * _abi.VOF_SCENE_SUM_N))
    ptr = recs.ctypes.data_as(C.POINTER(C.c_double))
    assert hip_api.set_scene(None, ptr, 1, 8, _abi.VOF_SCENE_CLEAR, summ) == _abi.VOF_EINVAL
    assert hip_api.set_scene(None, None, 0, 8, 0, None) == _abi.VOF_EINVAL
    assert list(summ) == [-7.0] * _abi.VOF_SCENE_SUM_N and recs.tobytes() == scene.pack([scene.disc(0.05, 0.05, 0.01, "liquid")]).tobytes()
    assert np.dtype(np.float64).itemsize * _abi.VOF_SHAPE_N == recs.strides[0]


def test_the_oracle_does_not_get_the_verb(oracle_api):
    assert not hasattr(oracle_api, "set_scene")
