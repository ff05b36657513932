"""Many verbs on one handle, capacities that grow and then shrink (runtime/buffers.h owns every work buffer of a handle):
the per-verb tests give each verb a fresh handle and ask for more and more; here one handle runs diagnostics, step_diag,
the display fields, the raw vof_interface and vof_blobs with capacities below, at and above the need, both solvers and
step_mg, and every read-only verb again.  All comparisons are of bytes: a read-only result against the same single call on
a fresh handle that was given the same F, u, v, p; the solvers against a handle with the same steps that ran only the
solver calls; one result per verb and grid against its NumPy restatement too.
"""
import ctypes as C

import numpy as np
import pytest

import _blobs_np as bnp
from test_blobs_gpu import hold_to_restatement as blobs_restated, set_pattern
from test_diag_gpu import hold_to_restatement as diag_restated, vec
from test_interface_gpu import hold_to_restatement as iface_restated
from test_step_mg_gpu import assert_same_state
from util import STATE, engine
from vof2d import _abi, halo_rows

pytestmark = pytest.mark.gpu
PTR, IPTR = C.POINTER(C.c_double), C.POINTER(C.c_int32)
EPS, UNTOUCHED = 1e-6, -777.25
GRIDS = [(33, 17, "f64"), (130, 260, "f64"), (130, 516, "f32")]   # narrower than one tile and one chunk; several of both; fp32


def given(api, src, nx, ny, dtype, **kw):
    """A fresh handle with the F, u, v, p and istep of src."""
    e = engine(api, nx, ny, dtype, "f32", **kw)
    r = (e.row_lo, e.row_hi)
    for f in STATE:
        e.set(f, src.get(f, r), rows=r)
    e.istep = src.istep
    return e


def iface_raw(api, e, cap):
    rows = np.full((cap + 2, _abi.VOF_IFACE_N), UNTOUCHED)
    summ = (C.c_double * _abi.VOF_IFACE_SUM_N)()
    assert api.interface(e.handle, EPS, rows.ctypes.data_as(PTR) if cap else None, cap, summ) == 0
    n = min(cap, int(summ[_abi.VOF_IFACE_SUM_SEGMENTS]))
    assert np.all(rows[n:] == UNTOUCHED)
    return rows[:n].tobytes(), list(summ)


def blobs_raw(api, e, phase, cap, labels):
    rows = np.full((cap + 2, _abi.VOF_BLOB_N), UNTOUCHED)
    summ = (C.c_double * _abi.VOF_BLOB_SUM_N)()
    lab = np.full((max(min(e.own_hi, e.nx) - max(e.own_lo, 1) + 1, 0), e.ny), -7, dtype=np.int32)
    assert api.blobs(e.handle, phase, 0.5, rows.ctypes.data_as(PTR) if cap else None, cap, lab.ctypes.data_as(IPTR) if labels else None,
                     lab.nbytes if labels else 0, summ) == 0
    n = min(cap, int(summ[_abi.VOF_BLOB_SUM_BLOBS]))
    assert np.all(rows[n:] == UNTOUCHED) and (labels or np.all(lab == -7))
    return rows[:n].tobytes(), list(summ), lab.tobytes()


def call(api, e, key):
    """One read-only call; what it returned, as bytes and lists."""
    if key[0] == "diagnostics":
        return vec(e.diagnostics()).tobytes()
    if key[0] == "interp_velocity":
        return e.interp_velocity().tobytes()
    if key[0] == "vis_field":
        return e.vis_field("vof").tobytes()
    if key[0] == "interface":
        return iface_raw(api, e, key[1])
    return blobs_raw(api, e, *key[1:])


def read_only(api, e, display=True, phases=(0,)):
    """Every read-only verb on e, in the order of the module's docstring: {key: result}.  The scratch of the display fields
    grows from interp_velocity to vis_field; the segments are asked for with capacity 0, exact, exact + 50, 1; the blobs with
    1, exact, 3, with and without labels."""
    out = {}
    keys = [("diagnostics",)] + ([("interp_velocity",), ("vis_field",)] if display else [])
    for key in keys + [("interface", 0)]:
        out[key] = call(api, e, key)
    n = int(out["interface", 0][1][_abi.VOF_IFACE_SUM_SEGMENTS])
    for cap in (n, n + 50, 1):
        out["interface", cap] = call(api, e, ("interface", cap))
    for phase in phases:
        out["blobs", phase, 1, True] = call(api, e, ("blobs", phase, 1, True))
        nb = int(out["blobs", phase, 1, True][1][_abi.VOF_BLOB_SUM_BLOBS])
        for cap in (1, nb, 3):
            for labels in (True, False):
                out["blobs", phase, cap, labels] = call(api, e, ("blobs", phase, cap, labels))
    return out


def hold_read_only(api, e, fresh, ctx, **kw):
    """read_only(e); every result equals the same single call on a handle fresh() returns; a truncated request returns the
    first rows of the full list, the same summary and the same labels."""
    got = read_only(api, e, **kw)
    for key, value in got.items():
        f = fresh()
        assert call(api, f, key) == value, "%s: %r on the shared handle and on a fresh one" % (ctx, key)
        f.close()
    n = int(got["interface", 0][1][_abi.VOF_IFACE_SUM_SEGMENTS])
    full = got["interface", n]
    assert len(full[0]) == n * _abi.VOF_IFACE_N * 8 and got["interface", n + 50] == full, ctx
    for cap in (0, 1):
        assert got["interface", cap] == (full[0][:min(cap, n) * _abi.VOF_IFACE_N * 8], full[1]), ctx
    for phase in kw.get("phases", (0,)):
        nb = int(got["blobs", phase, 1, True][1][_abi.VOF_BLOB_SUM_BLOBS])
        whole = got["blobs", phase, nb, True]
        assert len(whole[0]) == nb * _abi.VOF_BLOB_N * 8, ctx
        for cap in (1, 3):
            for labels in (True, False):
                rows, summ, lab = got["blobs", phase, cap, labels]
                assert (rows, summ) == (whole[0][:min(cap, nb) * _abi.VOF_BLOB_N * 8], whole[1]) and (not labels or lab == whole[2]), ctx
        assert got["blobs", phase, nb, False][:2] == whole[:2], ctx
    print(ctx, "segments", n, "read-only calls", len(got))
    return got


def hold_restatements(e, ctx):
    diag_restated(e, ctx, bits=True)
    iface_restated(e, ctx)
    blobs_restated(e, ctx, "liquid")


@pytest.mark.parametrize("nx,ny,dtype", GRIDS)
def test_one_handle_runs_every_verb(hip_api, nx, ny, dtype):
    ctx = "%dx%d %s" % (nx, ny, dtype)
    e, twin, solo = (engine(hip_api, nx, ny, dtype, "f32", ic=3) for _ in range(3))
    for h in (e, twin, solo):
        h.step(4)
    fresh = lambda: given(hip_api, e, nx, ny, dtype)
    # 1-3: diagnostics, then rows recorded on the device: the row buffer grows 1 -> 7, then a smaller request
    first = call(hip_api, e, ("diagnostics",))
    assert first == vec(twin.diagnostics()).tobytes(), ctx
    for nsteps, every in ((7, 1), (2, 2)):
        rows = e.step_diag(nsteps, every)
        want = []
        for _ in range(nsteps // every):
            twin.step(every); solo.step(every)
            want.append(vec(twin.diagnostics()))
        assert rows.shape == (nsteps // every, _abi.VOF_DIAG_N) and rows.tobytes() == np.array(want).tobytes(), "%s step_diag(%d, %d)" % (ctx, nsteps, every)
    assert e.istep == twin.istep == 13
    # 4-6: the read-only verbs, capacities up and down
    before = hold_read_only(hip_api, e, fresh, ctx + " behind step_diag")
    hold_restatements(e, ctx + " behind step_diag")
    # 7: the solves share the scalars and the reduction buffer; `solo` runs nothing but them
    for name, args in (("solve_p_mg", (1e-9, 30)), ("solve_p_cg", (1e-9, 200, 10))):
        got, want = getattr(e, name)(*args), getattr(solo, name)(*args)
        print(ctx, name, got)
        assert np.array(got).tobytes() == np.array(want).tobytes(), "%s %s" % (ctx, name)
    assert_same_state(e, solo, ctx + " behind the solves")
    # 8: F, u, v did not change: the same bytes as before the solves
    assert read_only(hip_api, e) == before, ctx + " behind the solves"
    got, want = e.step_mg(2, 2), solo.step_mg(2, 2)
    assert np.array(got).tobytes() == np.array(want).tobytes(), ctx + " step_mg"
    assert_same_state(e, solo, ctx + " behind step_mg")
    after = hold_read_only(hip_api, e, fresh, ctx + " behind step_mg")
    assert after["diagnostics",] != before["diagnostics",]
    if (nx, ny) == (33, 17):
        # a checkerboard: 281 liquid blobs and a segment in every cell, more than any capacity so far
        set_pattern(e, bnp.checkerboard(nx, ny))
        board = hold_read_only(hip_api, e, fresh, ctx + " checkerboard", phases=(0, 1))
        most = max(r["interface", 0][1][_abi.VOF_IFACE_SUM_SEGMENTS] for r in (before, after)) + 50
        assert board["blobs", 0, 1, True][1][_abi.VOF_BLOB_SUM_BLOBS] == 281 and board["interface", 0][1][_abi.VOF_IFACE_SUM_SEGMENTS] > most
        hold_restatements(e, ctx + " checkerboard")
    # teardown: another handle on the same device, a short version of the above
    for h in (e, twin, solo):
        h.close()
    e, twin = (engine(hip_api, nx, ny, dtype, "f32", ic=3) for _ in range(2))
    e.step(4); twin.step(4)
    rows = e.step_diag(2, 1)
    for k in range(2):
        twin.step(1)
        assert rows[k].tobytes() == vec(twin.diagnostics()).tobytes(), ctx + " second handle"
    hold_read_only(hip_api, e, lambda: given(hip_api, e, nx, ny, dtype), ctx + " second handle")
    got, want = e.solve_p_mg(1e-9, 30), twin.solve_p_mg(1e-9, 30)
    assert np.array(got).tobytes() == np.array(want).tobytes(), ctx + " second handle"


def test_a_pair_of_strips_runs_the_verbs_that_take_one(hip_api):
    nx, ny, W = 130, 260, halo_rows(10)
    src = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    src.step(4)
    for own in ((1, 65), (66, 130)):
        kw = dict(rows=(max(0, own[0] - W), min(nx + 1, own[1] + W)), own=own)
        ctx = "130x260 f64 strip %d..%d" % own
        e = given(hip_api, src, nx, ny, "f64", **kw)
        fresh = lambda: given(hip_api, src, nx, ny, "f64", **kw)
        once = hold_read_only(hip_api, e, fresh, ctx, display=False, phases=(0, 1))
        assert read_only(hip_api, e, display=False, phases=(0, 1)) == once, ctx + " again"
        hold_restatements(e, ctx)
