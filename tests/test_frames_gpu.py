"""vof_frame, vof_frame_set_lut and vof_step_frames on the GPU (include/vof2d.h).

The device is held byte for byte to the restatement of tests/_frames_np.py (judged on its own in tests/test_frames.py)
applied to the fields vof_get_field returns: the means, the picture and the summary.  The grids are small: what can go wrong
is a matter of tile, chunk and block boundaries, not of size.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import _frames_np as fnp
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, frames, halo_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U8P, DP = C.POINTER(C.c_uint8), C.POINTER(C.c_double)
TILE = 128                                      # 64 V columns of a wave: V = 2 for both dtypes (vof2d_device.h)
QUANTITIES = ("F", "U", "V", "SPEED", "P", "VORT", "DYE")
RANGE_OF = {"F": (0.0, 1.0), "U": (-0.01, 0.02), "V": (-0.02, 0.01), "SPEED": (0.0, 0.02), "P": (-1.0, 30.0), "VORT": (-5.0, 5.0), "DYE": (0.25, 0.5)}


def custom_lut():
    k = np.arange(fnp.LUT_ROWS)
    return np.stack([(k * 7 + 3) % 256, (255 - k) % 256, (k * 13) % 256], axis=1).astype(np.uint8)


def dye_of(e):
    """A dye that differs from F: a ramp along i times a ramp along j, ghost cells included."""
    i, j = np.meshgrid(np.arange(e.nx + 2), np.arange(e.ny + 2), indexing="ij")
    return ((i % 9) / 8.0 * ((j % 5) + 1) / 5.0).astype(e.np_dtype)


def fields_of(e, dye=True):
    f = {n: e.get(n) for n in ("F", "u", "v", "p")}
    if dye:
        f["C"] = e.dye_get()
    return f


def hold(e, f, q, bx, by, ctx, lut=None, **kw):
    """One vof_frame of e against the restatement on the fields f; returns what the device gave."""
    rgb, m, summ = e.frame(q, bx, by, means=True, **kw)
    flags = (fnp.CONTOUR if kw.get("contour") else 0) | (fnp.SYMMETRIC if kw.get("symmetric") else 0)
    wrgb, wm, wsum = fnp.frame(frames.QUANTITIES[q], f, bx, by, flags, kw.get("lo", 0.0), kw.get("hi", 0.0), lut, e.istep,
                               0.5 * e.get_param("dxi"), 0.5 * e.get_param("dyi"))
    got = np.array([summ[k] for k in frames.SUMMARY] + [0.0])
    ctx = "%s %s %dx%d %s" % (ctx, q, bx, by, sorted(kw.items()))
    assert m.shape == wm.shape and rgb.shape == wrgb.shape, ctx
    if m.tobytes() != wm.tobytes():
        bad = np.argwhere(m.view(np.uint64) != wm.view(np.uint64))
        raise AssertionError("%s: %d of %d means differ, first at %s: %r, restated %r" % (ctx, len(bad), m.size, bad[0], m[tuple(bad[0])], wm[tuple(bad[0])]))
    assert got.tobytes() == wsum.tobytes(), "%s: summary %s, restated %s" % (ctx, got, wsum)
    if rgb.tobytes() != wrgb.tobytes():
        bad = np.argwhere((rgb != wrgb).any(axis=2))
        raise AssertionError("%s: %d of %d pixels differ, first at %s: %s, restated %s" % (ctx, len(bad), rgb.shape[0] * rgb.shape[1], bad[0], rgb[tuple(bad[0])],
                                                                                           wrgb[tuple(bad[0])]))
    return rgb, m, summ


# ---------------------------------------------------------------------------- bytes equal the restatement
# nx = 7: the chunk rule gives chunks of two rows at bx = 1 and 2, three of them and a remainder; nx = 33: sixteen and a remainder
@pytest.mark.parametrize("ny", [17, TILE, TILE + 1, TILE + 3])
@pytest.mark.parametrize("nx", [7, 33])
@pytest.mark.parametrize("dtype,ic", [("f64", 1), ("f32", 3), ("f64", 3), ("f32", 1)])
def test_bytes_equal_the_restatement(hip_api, dtype, ic, nx, ny):
    assert fnp.chunking(nx, ny, 1)[:2] == (2, nx // 2 + 1) and fnp.chunking(nx, ny, 2)[:2] == (2, nx // 2 + 1) and nx % 2 == 1
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    e.step(3)
    e.dye_set(dye_of(e))
    f = fields_of(e)
    ctx = "%dx%d %s ic %d" % (nx, ny, dtype, ic)
    tables = (None, custom_lut())
    n = 0
    for bx, by in ((1, 1), (2, 2), (3, 7), (4, 3), (nx + 5, 1), (1, ny + 5)):
        for q in QUANTITIES:
            for contour in (False, True):
                for mode in ("fixed", "auto", "symmetric"):
                    lut = tables[n % 2]
                    e.set_frame_lut(lut)
                    kw = {"contour": contour}
                    if mode == "fixed":
                        kw["lo"], kw["hi"] = RANGE_OF[q]
                    kw["symmetric"] = mode == "symmetric" or (mode == "fixed" and n % 3 == 0)   # (ignored on a fixed range)
                    hold(e, f, q, bx, by, ctx, lut, **kw)
                    n += 1
    assert e.istep == 3 and all(np.array_equal(e.get(k), f[k]) for k in ("F", "u", "v", "p"))


def test_behind_steps_with_virtual_ghosts_and_a_larger_grid(hip_api):
    """300 x 260 f64, three tiles, the last with 4 columns: called first thing behind vof_step, before any vof_get_field settles the
    ghost cells VORT reads at the walls."""
    e = engine(hip_api, 300, 260, "f64", "f32", ic=1)
    e.step(12)
    first = e.frame("VORT", 3, 5, contour=True, symmetric=True, means=True)
    f = fields_of(e, dye=False)
    again = hold(e, f, "VORT", 3, 5, "300x260 behind vof_step", contour=True, symmetric=True)
    assert first[0].tobytes() == again[0].tobytes() and first[1].tobytes() == again[1].tobytes() and first[2] == again[2]
    for q in ("F", "SPEED"):
        hold(e, f, q, 8, 8, "300x260", contour=True)
    # 78 000 pixels at one cell a pixel: more than the 256 blocks of k_frame_fold and k_frame_paint hold at once, so the blocks
    # stride on into a second, partial round
    assert 300 * 260 > 256 * 256
    hold(e, f, "VORT", 1, 1, "300x260", contour=True, symmetric=True)
    hold(e, f, "F", 1, 1, "300x260", contour=True)


# ---------------------------------------------------------------------------- NaN, subnormal values
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_one_nan_cell_and_a_subnormal_p(hip_api, dtype):
    nx, ny = 33, TILE + 3
    e = engine(hip_api, nx, ny, dtype, "f32", ic=3)
    e.step(2)
    F = e.get("F")
    F[20, 100] = np.nan
    e.set("F", F)
    f = fields_of(e, dye=False)
    for bx, by in ((1, 1), (3, 7)):
        for sym in (False, True):
            rgb, m, summ = hold(e, f, "F", bx, by, "a NaN in F[20,100]", contour=True, symmetric=sym)
            a, b = (20 - 1) // bx, (100 - 1) // by
            assert np.argwhere(np.isnan(m)).tolist() == [[a, b]] and summ["NAN_PIXELS"] == 1
            nanpix = (rgb == np.array([255, 0, 255], dtype=np.uint8)).all(axis=2)
            assert np.argwhere(nanpix).tolist() == [[m.shape[1] - 1 - b, a]]
            lo, hi = fnp.auto_range(m, sym)
            assert (summ["LO"], summ["HI"]) == (lo, hi) and np.isfinite([lo, hi]).all()
        hold(e, f, "F", bx, by, "a NaN in F[20,100], the contour off")
    # p made of subnormal numbers of its dtype (and zeros): the means, the auto range and the quotients stay exact operations on them
    tiny = np.finfo(e.np_dtype).smallest_subnormal
    i, j = np.meshgrid(np.arange(nx + 2), np.arange(ny + 2), indexing="ij")
    e.set("p", (((i * 31 + j * 17) % 23 - 11) * tiny).astype(e.np_dtype))
    f = fields_of(e, dye=False)
    assert np.abs(f["p"]).max() < np.finfo(e.np_dtype).tiny and f["p"].any()
    for bx, by in ((1, 1), (2, 2), (3, 7)):
        for sym in (False, True):
            _, m, summ = hold(e, f, "P", bx, by, "a subnormal p", symmetric=sym)
            assert summ["HI"] > summ["LO"] and abs(summ["HI"]) < 1e-30
    # nothing but NaN: lo = hi = 0, every pixel NaN-coloured
    e.set("p", np.full((nx + 2, ny + 2), np.nan, dtype=e.np_dtype))
    rgb, m, summ = hold(e, fields_of(e, dye=False), "P", 4, 3, "p all NaN")
    assert (summ["LO"], summ["HI"], summ["NAN_PIXELS"]) == (0.0, 0.0, m.size)


# ---------------------------------------------------------------------------- vof_step_frames equals the separate calls
@pytest.mark.parametrize("dtype,ic,cycles", [("f64", 1, 0), ("f32", 3, 2), ("f64", 3, 2), ("f32", 1, 0)])
def test_step_frames_equals_step_then_frame(hip_api, dtype, ic, cycles):
    nx, ny, nsteps, every = 64, TILE + 2, 11, 3
    a, b, c = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(3))
    kw = dict(quantity="VORT", bx=3, by=2, contour=True, symmetric=True)
    pics, summs = a.step_frames(nsteps, every, mg_cycles=cycles, **kw)
    assert pics.shape == (3, 65, 22, 3) and len(summs) == 3
    for r in range(3):
        if cycles:
            b.step_mg(every, cycles)
        else:
            b.step(every)
        rgb, _, summ = b.frame(**kw)
        assert summ["ISTEP"] == every * (r + 1) and summs[r] == summ, (r, summs[r], summ)
        assert pics[r].tobytes() == rgb.tobytes(), "frame %d" % r
    assert len({p.tobytes() for p in pics}) == 3            # (the pictures do change from frame to frame)
    if cycles:
        b.step_mg(nsteps % every, cycles); c.step_mg(nsteps, cycles)
    else:
        b.step(nsteps % every); c.step(nsteps)
    assert_same_state(a, c, "vof_step_frames against the steps alone")
    assert_same_state(a, b, "vof_step_frames against step + vof_frame")
    a.step(4); c.step(4)
    assert_same_state(a, c, "a vof_step behind vof_step_frames")
    # no frame due: the steps alone, the outputs not needed
    done = C.c_int64(-1)
    s = frames.spec("F", 2)
    assert hip_api.step_frames(a.handle, 2, 5, 0, 0, C.byref(s), None, None, 0, C.byref(done)) == 0 and done.value == 0 and a.istep == nsteps + 6


# ---------------------------------------------------------------------------- the FMA build
WORKER = """
import sys
import numpy as np
sys.path[:0] = [%r, %r]
from vof2d._lib import hip_api
from vof2d.engine import Engine, make_desc
z = np.load(sys.argv[1])
api = hip_api(fast=True)
out = {}
for dtype in ("f64", "f32"):
    e = Engine(api, make_desc(api, int(z["nx"]), int(z["ny"]), dtype, "f32"))
    for n in ("F", "u", "v", "p"):
        e.set(n, z[n])
    e.dye_set(z["C"])
    for q in %r:
        rgb, m, summ = e.frame(q, 3, 7, contour=True, symmetric=True, means=True)
        out[dtype + q + "rgb"], out[dtype + q + "m"], out[dtype + q + "s"] = rgb, m, np.array([summ[k] for k in sorted(summ)])
    e.close()
np.savez(sys.argv[2], **out)
"""


def test_the_fma_build_gives_the_same_bytes(hip_api, tmp_path):
    """The same fields set into a handle of either build (a process loads one of the two libraries: the FMA build runs in a
    child): every quantity's means, picture and summary are equal byte for byte."""
    nx, ny = 33, TILE + 3
    src = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    src.step(5)
    src.dye_set(dye_of(src))
    z = fields_of(src)
    np.savez(str(tmp_path / "in.npz"), nx=nx, ny=ny, **z)
    code = WORKER % (os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "tests"), QUANTITIES)
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    fast = np.load(str(tmp_path / "out.npz"))
    for dtype in ("f64", "f32"):
        e = engine(hip_api, nx, ny, dtype, "f32")
        for n in ("F", "u", "v", "p"):
            e.set(n, z[n])
        e.dye_set(z["C"])
        for q in QUANTITIES:
            rgb, m, summ = e.frame(q, 3, 7, contour=True, symmetric=True, means=True)
            assert fast[dtype + q + "m"].tobytes() == m.tobytes(), (dtype, q)
            assert fast[dtype + q + "rgb"].tobytes() == rgb.tobytes(), (dtype, q)
            assert fast[dtype + q + "s"].tobytes() == np.array([summ[k] for k in sorted(summ)]).tobytes(), (dtype, q)


# ---------------------------------------------------------------------------- refusals change nothing
UNTOUCHED = -777.25


def raw_frame(api, h, s, cap_bytes, cap_means, want_rgb=True, want_means=True, want_sum=True):
    rgb, m = np.full(max(cap_bytes, 0) + 5, 77, dtype=np.uint8), np.full(max(cap_means, 0) + 2, UNTOUCHED)
    summ = (C.c_double * _abi.VOF_FRAME_SUM_N)(*([UNTOUCHED] * _abi.VOF_FRAME_SUM_N))
    rc = api.frame(h, C.byref(s) if s is not None else None, rgb.ctypes.data_as(U8P) if want_rgb else None, cap_bytes, m.ctypes.data_as(DP) if want_means else None,
                   cap_means, summ if want_sum else None)
    return rc, rgb, m, list(summ)


def test_refusals_change_nothing(hip_api):
    api, EINVAL, ESTATE = hip_api, _abi.VOF_EINVAL, _abi.VOF_ESTATE
    nx, ny, bx, by = 40, 50, 3, 4
    pw, ph = 14, 13
    e = engine(api, nx, ny, "f64", "f32", ic=1)
    e.step(3)
    before = {n: e.get(n) for n in FIELDS}
    good = lambda **kw: frames.spec(**{**dict(quantity="F", bx=bx, by=by, lo=0.0, hi=1.0), **kw})
    rgb0, m0, s0 = e.frame("F", bx, by, 0.0, 1.0, means=True)
    # larger caps: nothing behind the picture and the means is touched; NULL outputs are skipped and the summary is whole
    rc, rgb, m, s = raw_frame(api, e.handle, good(), pw * ph * 3 + 5, pw * ph + 2)
    assert rc == 0 and rgb[:pw * ph * 3].tobytes() == rgb0.tobytes() and (rgb[pw * ph * 3:] == 77).all() and m[:pw * ph].tobytes() == m0.tobytes() and (m[pw * ph:] == UNTOUCHED).all()
    assert s[:7] == [s0[k] for k in frames.SUMMARY] and s[7] == 0.0
    for wr, wm in ((False, False), (True, False), (False, True)):
        rc, rgb2, m2, s2 = raw_frame(api, e.handle, good(), pw * ph * 3 if wr else 0, pw * ph if wm else 0, wr, wm)
        assert rc == 0 and s2 == s and ((rgb2 == 77).all() if not wr else rgb2[:pw * ph * 3].tobytes() == rgb0.tobytes())
        assert (m2 == UNTOUCHED).all() if not wm else m2[:pw * ph].tobytes() == m0.tobytes()
    bad = [good(quantity=7), good(quantity=-1), good(bx=0), good(by=0), good(bx=-3), good(lo=1.0, hi=0.5), good(lo=float("nan")), good(hi=float("inf")),
           good(lo=float("-inf"), hi=0.0), None]
    flagged = good()
    flagged.flags = 4
    bad.append(flagged)
    for s in bad:
        rc, rgb, m, summ = raw_frame(api, e.handle, s, pw * ph * 3, pw * ph)
        assert rc == EINVAL and (rgb == 77).all() and (m == UNTOUCHED).all() and summ == [UNTOUCHED] * 8, s and (s.quantity, s.bx, s.by, s.flags, s.lo, s.hi)
    for cb, cm in ((pw * ph * 3 - 1, pw * ph), (pw * ph * 3, pw * ph - 1), (-1, pw * ph), (pw * ph * 3, -1)):
        rc, rgb, m, summ = raw_frame(api, e.handle, good(), cb, cm)
        assert rc == EINVAL and (rgb == 77).all() and (m == UNTOUCHED).all() and summ == [UNTOUCHED] * 8, (cb, cm)
    assert raw_frame(api, e.handle, good(), pw * ph * 3, pw * ph, want_sum=False)[0] == EINVAL
    assert raw_frame(api, None, good(), pw * ph * 3, pw * ph)[0] == EINVAL
    # the dye without a dye
    rc, rgb, m, summ = raw_frame(api, e.handle, good(quantity="DYE"), pw * ph * 3, pw * ph)
    assert rc == ESTATE and (rgb == 77).all() and (m == UNTOUCHED).all() and summ == [UNTOUCHED] * 8
    # vof_step_frames: the argument errors of vof_step_gauges, and those of the spec
    out, sums, done = np.full(4 * pw * ph * 3, 77, dtype=np.uint8), np.full(4 * 8, UNTOUCHED), C.c_int64(-5)
    call = lambda nsteps, every, cyc, crit, s, cap, o=out, q=sums: api.step_frames(e.handle, nsteps, every, cyc, crit, C.byref(s) if s is not None else None,
                                                                                   o.ctypes.data_as(U8P) if o is not None else None,
                                                                                   q.ctypes.data_as(DP) if q is not None else None, cap, C.byref(done))
    for args in ((4, 0, 0, 0, good(), 4), (-1, 1, 0, 0, good(), 4), (4, 1, -1, 0, good(), 4), (4, 1, 2, 7, good(), 4), (4, 1, 0, 0, good(), 3), (4, 1, 0, 0, None, 4),
                 (4, 1, 0, 0, good(bx=0), 4), (4, 1, 0, 0, good(lo=2.0, hi=1.0), 4)):
        assert call(*args) == EINVAL, args[:4]
    assert call(4, 2, 0, 0, good(), 2, o=None) == EINVAL and call(4, 2, 0, 0, good(), 2, q=None) == EINVAL
    assert call(4, 2, 0, 0, good(quantity="DYE"), 2) == ESTATE
    assert (out == 77).all() and (sums == UNTOUCHED).all() and done.value == -5
    # a phased step in progress
    e.step_phase(0)
    assert raw_frame(api, e.handle, good(), pw * ph * 3, pw * ph)[0] == ESTATE and call(4, 2, 0, 0, good(), 2) == ESTATE
    assert api.frame_set_lut(e.handle, None) == ESTATE
    e.step_phase(1); e.step_phase(2)
    twin = engine(api, nx, ny, "f64", "f32", ic=1)
    twin.step(4)
    assert_same_state(e, twin, "the refusals, then the rest of a phased step")
    assert e.istep == 4
    # a strip
    W = halo_rows(10)
    s = engine(api, 120, 70, "f64", "f32", ic=1, rows=(0, 60 + W), own=(1, 60))
    sb = {n: s.get(n) for n in ("F", "u", "v", "p")}
    assert raw_frame(api, s.handle, good(), 10 ** 6, 10 ** 5)[0] == ESTATE and api.frame_set_lut(s.handle, None) == ESTATE
    assert api.step_frames(s.handle, 4, 2, 0, 0, C.byref(good()), out.ctypes.data_as(U8P), sums.ctypes.data_as(DP), 2, C.byref(done)) == ESTATE
    assert s.istep == 0 and all(np.array_equal(s.get(n), sb[n]) for n in sb) and (out == 77).all() and (sums == UNTOUCHED).all()
    assert api.frame_set_lut(None, None) == EINVAL


def test_equal_bytes_twice_and_a_step_behind(hip_api):
    nx, ny = 96, 130
    e, twin = (engine(hip_api, nx, ny, "f64", "f32", ic=3) for _ in range(2))
    e.step(5); twin.step(5)
    one = e.frame("SPEED", 2, 3, contour=True, means=True)
    for other in (e.frame("SPEED", 2, 3, contour=True, means=True), twin.frame("SPEED", 2, 3, contour=True, means=True)):
        assert other[0].tobytes() == one[0].tobytes() and other[1].tobytes() == one[1].tobytes() and other[2] == one[2]
    e.set_frame_lut(custom_lut())
    e.step(4); twin.step(4)
    assert_same_state(e, twin, "a vof_step behind vof_frame")
