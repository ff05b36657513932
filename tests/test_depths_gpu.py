"""vof_depths on the GPU (include/vof2d.h).

The device is held to the restatement of tests/_depths_np.py (judged on its own in tests/test_depths.py) applied to the F
vof_get_field returns: depth_i, depth_j and SUM bit for bit to the order kernels/depths.h states (a NaN equals a NaN in the
same place), top, the fronts, TOP_J, ROWS and ISTEP with ==.  Every figure is printed before it is asserted.
"""
import ctypes as C
import math

import numpy as np
import pytest

import _depths_np as dnp
from _tracers_np import same_bits
from test_diag_gpu import TM_GRID
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, gauges, halo_rows

pytestmark = pytest.mark.gpu
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int32)
UNTOUCHED = -777.25


def hold(e, ctx, F=None):
    """vof_depths of e against the restatement of its F on its owned cells; returns what the device gave."""
    di, dj, top, summ = e.depths()
    F = e.get("F") if F is None else F
    lo, hi = max(e.own_lo, 1), min(e.own_hi, e.nx)
    res = dnp.restate(F, lo, hi, row0=e.row_lo)
    R = dnp.depths_chunk_rows(e.nx, e.ny, e.row_lo, e.row_hi)
    wi, wj, wsum = dnp.ordered(res["terms"], R)
    want = dnp.summary(res, wsum, e.istep)
    got = [summ[k] for k in gauges.DEPTH_SUMMARY]
    print(ctx, "R", R, "summary", got, "restated", list(want[:6]), "depth_i", di[:3], "depth_j", dj[:3], "top", top[:3])
    assert di.shape == wi.shape and dj.shape == (e.ny,) and top.dtype == np.int32
    assert same_bits(di, wi), ctx + ": depth_i"
    assert same_bits(dj, wj), ctx + ": depth_j"
    assert np.array_equal(top, res["top"]), ctx + ": top"
    assert same_bits(np.array(got, dtype=np.float64), want[:6]), ctx + ": summary"
    return di, dj, top, summ


# ---------------------------------------------------------------------------- bit for bit with the restatement
@pytest.mark.parametrize("nx,ny,ic,kw", [(33, 17, 2, {}), (96, 130, 3, {"Lx": 0.1, "Ly": 0.13})])
def test_small_and_rectangular_f64(hip_api, nx, ny, ic, kw):
    """33 x 17: one ragged tile, odd rows.  96 x 130: two tiles, the second holding 2 of 128 columns, dx != dy."""
    e = engine(hip_api, nx, ny, "f64", "f32", ic=ic, **kw)
    if kw:
        assert e.get_param("dxi") != e.get_param("dyi")
    for upto in (0, 1, 20):
        e.step(upto - e.istep)
        hold(e, "%dx%d f64 ic %d step %d" % (nx, ny, ic, upto))


@pytest.mark.parametrize("ic", [1, 2, 3])
def test_200_f32_after_0_1_and_50_steps(hip_api, ic):
    e = engine(hip_api, 200, 200, "f32", "f32", ic=ic)
    for upto in (0, 1, 50):
        e.step(upto - e.istep)
        _, _, _, summ = hold(e, "200x200 f32 ic %d step %d" % (ic, upto))
        assert summ["ROWS"] == 200 and summ["SUM"] > 0 and summ["ISTEP"] == upto


def test_many_chunk_partials_per_column_f64(hip_api):
    """1100 x 130: the rule gives 2-row chunks, 550 partials per column for one lane of k_depths_fold to add in order, 2200
    row partials in nine blocks of rows; the second tile is ragged."""
    nx, ny = 1100, 130
    assert dnp.depths_chunk_rows(nx, ny) == 2 and dnp.partial_counts(nx, ny, 2) == (2200, 550 * 130)
    e = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    for upto in (0, 1):
        e.step(upto - e.istep)
        hold(e, "%dx%d f64 ic 3 step %d" % (nx, ny, upto))


def test_behind_k_tm_batches(hip_api):
    """The grid on which vof_step batches its steps in the k_tm form: the handle is ahead and its ghost cells virtual when the
    verb is called, so this is where settling shows.  8-row chunks, 16 tiles."""
    nx, ny, dtype, ic = TM_GRID
    a, b = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(2))
    assert dnp.depths_chunk_rows(nx, ny) == 8
    for upto in (2, 34):
        a.step(upto - a.istep); b.step(upto - b.istep)
        first = a.depths()                          # first: before any vof_get_field settles the handle
        again = hold(a, "%dx%d %s ic %d behind vof_step to %d" % (nx, ny, dtype, ic, upto))
        assert all(np.array_equal(x, y) for x, y in zip(first[:3], again[:3])) and first[3] == again[3]
    assert a.get_counter("tm_steps") >= 2
    a.step(6); b.step(6)
    assert_same_state(a, b, "vof_depths between the vof_step calls of the k_tm grid")


# ---------------------------------------------------------------------------- hand-made states
def put(e, F):
    e.set("F", F.astype(e.np_dtype))


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_a_staircase_through_set_field(hip_api, dtype):
    """tests/test_depths.py, test_a_staircase: every value known in closed form (dyadic: exact in any order and dtype)."""
    nx, ny = 40, 150
    e = engine(hip_api, nx, ny, dtype, "f32")
    h = [1 + (7 * i) % 37 for i in range(1, nx + 1)]
    F = np.zeros((nx + 2, ny + 2))
    for i, hi in enumerate(h, 1):
        F[i, 1:hi + 1] = 1.0
        F[i, hi + 1] = 0.25
    F[0, :], F[nx + 1, :], F[:, 0], F[:, ny + 1] = 1.0, 1.0, 1.0, 1.0        # the ghost cells are no members of anything
    put(e, F)
    di, dj, top, summ = hold(e, "staircase " + dtype)
    assert di.tolist() == [hi + 0.25 for hi in h] and top.tolist() == h
    assert dj.tolist() == [sum(hi >= j for hi in h) + 0.25 * sum(hi == j - 1 for hi in h) for j in range(1, ny + 1)]
    assert summ == {"ROWS": nx, "ISTEP": 0, "FRONT_LO": 1, "FRONT_HI": nx, "TOP_J": max(h), "SUM": sum(h) + 0.25 * nx}


def test_a_nan_a_half_and_an_empty_floor(hip_api):
    nx, ny = 33, 130
    e = engine(hip_api, nx, ny, "f64", "f32")
    F = np.zeros((nx + 2, ny + 2))
    put(e, F)
    di, dj, top, summ = hold(e, "all gas")
    assert not di.any() and not dj.any() and not top.any() and (summ["FRONT_LO"], summ["FRONT_HI"], summ["TOP_J"], summ["SUM"]) == (0, 0, 0, 0.0)
    # exactly 0.5 is a member, the double below it is not; the floor stays empty while the members sit above it
    F[5, 2], F[6, 1], F[20, 129], F[21, 130] = 0.5, np.nextafter(0.5, 0), 0.5, np.nextafter(0.5, 0)
    put(e, F)
    di, dj, top, summ = hold(e, "members above an empty floor")
    assert (summ["FRONT_LO"], summ["FRONT_HI"], summ["TOP_J"]) == (0, 0, 129) and top[4] == 2 and top[5] == 0 and top[19] == 129 and top[20] == 0
    F[5, 1] = 0.5
    put(e, F)
    _, _, top, summ = hold(e, "0.5 on the floor")
    assert (summ["FRONT_LO"], summ["FRONT_HI"]) == (5, 5) and top[4] == 2
    # one NaN cell reaches depth_i of its row, depth_j of its column and SUM; it is no member
    F[9, 70] = np.nan
    put(e, F)
    di, dj, top, summ = hold(e, "a NaN in F[9,70]")
    assert np.isnan(di).nonzero()[0].tolist() == [8] and np.isnan(dj).nonzero()[0].tolist() == [69] and math.isnan(summ["SUM"]) and top[8] == 0
    # all liquid
    put(e, np.ones((nx + 2, ny + 2)))
    di, dj, top, summ = hold(e, "all liquid")
    assert di.tolist() == [float(ny)] * nx and dj.tolist() == [float(nx)] * ny and top.tolist() == [ny] * nx
    assert summ == {"ROWS": nx, "ISTEP": 0, "FRONT_LO": 1, "FRONT_HI": nx, "TOP_J": ny, "SUM": float(nx * ny)}


# ---------------------------------------------------------------------------- against a verb that exists
@pytest.mark.parametrize("nx,ny,dtype,ic", [(200, 200, "f32", 1), (96, 130, "f64", 3)])
def test_sum_against_the_diagnostics(hip_api, nx, ny, dtype, ic):
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    e.step(30)
    summ = e.depths()[3]
    raw = e.diagnostics()
    t = e.get("F")[1:nx + 1, 1:ny + 1].astype(np.float64)
    bound = dnp.bound_of(t)                        # of either order of summing the same terms: the sum of the two bounds
    print("SUM", summ["SUM"], "SUM_F", raw["SUM_F"], "|d|", abs(summ["SUM"] - raw["SUM_F"]), "bound", 2 * bound)
    assert abs(summ["SUM"] - raw["SUM_F"]) <= 2 * bound and summ["ROWS"] * ny == raw["CELLS"]


# ---------------------------------------------------------------------------- strips
@pytest.mark.parametrize("nstrips", [2, 3])
def test_strips_combine_to_the_domain(hip_api, nstrips):
    nx, ny, W = 120, 70, halo_rows(10)
    full = engine(hip_api, nx, ny, "f64", "f32", ic=1)
    bounds = [round(k * nx / nstrips) for k in range(nstrips + 1)]
    strips = [engine(hip_api, nx, ny, "f64", "f32", ic=1, rows=(max(0, bounds[k] + 1 - W), min(nx + 1, bounds[k + 1] + W)),
                     own=(bounds[k] + 1, bounds[k + 1])) for k in range(nstrips)]
    for step in range(1, 13):
        full.step(1)
        for s in strips:
            s.step(1)
        for k in range(nstrips - 1):
            lo_s, hi_s = strips[k], strips[k + 1]
            edge = lo_s.own_hi
            for f in ("F", "u", "v", "p"):
                lo_s.copy_rows_from(hi_s, f, edge + 1, edge + W)
                hi_s.copy_rows_from(lo_s, f, edge + 1 - W, edge)
        if step in (1, 12):
            parts = [hold(s, "strip %d..%d step %d" % (s.own_lo, s.own_hi, step)) for s in strips]
            ci, cj, ctop, cs = gauges.combine(parts)
            di, dj, top, summ = hold(full, "the whole domain, step %d" % step)
            t = full.get("F")[1:nx + 1, 1:ny + 1].astype(np.float64)
            assert np.array_equal(ci, di) and np.array_equal(ctop, top)
            assert all(dnp.within_bound(cj[c], t[:, c]) for c in range(ny)) and dnp.within_bound(cs["SUM"], t)
            assert all(abs(cj[c] - dj[c]) <= 2 * dnp.bound_of(t[:, c]) for c in range(ny))
            assert {k: cs[k] for k in ("ROWS", "ISTEP", "FRONT_LO", "FRONT_HI", "TOP_J")} == {k: summ[k] for k in ("ROWS", "ISTEP", "FRONT_LO", "FRONT_HI", "TOP_J")}


def test_a_strip_that_owns_nothing(hip_api):
    s = engine(hip_api, 64, 64, "f64", "f32", ic=1, rows=(0, 40), own=(2, 1))
    di, dj, top, summ = hold(s, "a strip without owned rows")
    assert len(di) == 0 and len(top) == 0 and not dj.any() and summ == {"ROWS": 0, "ISTEP": 0, "FRONT_LO": 0, "FRONT_HI": 0, "TOP_J": 0, "SUM": 0.0}


# ---------------------------------------------------------------------------- buffers, errors, repeatability
def raw(api, e, ci, cj, ct, want_i=True, want_j=True, want_t=True):
    """One raw call with arrays two elements longer than the caps, filled with sentinels."""
    a, b, c = np.full(max(ci, 0) + 2, UNTOUCHED), np.full(max(cj, 0) + 2, UNTOUCHED), np.full(max(ct, 0) + 2, -7, dtype=np.int32)
    summ = (C.c_double * _abi.VOF_DEPTH_SUM_N)(*([UNTOUCHED] * _abi.VOF_DEPTH_SUM_N))
    rc = api.depths(e.handle, a.ctypes.data_as(DP) if want_i else None, ci, b.ctypes.data_as(DP) if want_j else None, cj,
                    c.ctypes.data_as(IP) if want_t else None, ct, summ)
    return rc, a, b, c, list(summ)


def test_buffers_errors_and_equal_bytes(hip_api):
    nx, ny = 96, 130
    api, EINVAL = hip_api, _abi.VOF_EINVAL
    e = engine(api, nx, ny, "f64", "f32", ic=3)
    e.step(5)
    before = {n: e.get(n) for n in FIELDS}
    di, dj, top, summ = hold(e, "96x130 f64 step 5")
    # larger caps: nothing behind rows / ny elements is touched; NULL outputs are skipped and the summary is whole
    rc, a, b, c, s = raw(api, e, nx + 1, ny + 1, nx + 1)
    assert rc == 0 and a[:nx].tobytes() == di.tobytes() and b[:ny].tobytes() == dj.tobytes() and c[:nx].tobytes() == top.tobytes()
    assert (a[nx:] == UNTOUCHED).all() and (b[ny:] == UNTOUCHED).all() and (c[nx:] == -7).all() and s[6:] == [0.0, 0.0]
    for wi, wj, wt in ((False, False, False), (True, False, False), (False, True, False), (False, False, True)):
        rc, a2, b2, c2, s2 = raw(api, e, nx if wi else 0, ny if wj else 0, nx if wt else 0, wi, wj, wt)
        assert rc == 0 and s2 == s, (wi, wj, wt)
        assert a2[:nx].tobytes() == di.tobytes() if wi else (a2 == UNTOUCHED).all()
        assert b2[:ny].tobytes() == dj.tobytes() if wj else (b2 == UNTOUCHED).all()
        assert c2[:nx].tobytes() == top.tobytes() if wt else (c2 == -7).all()
    # refusals: the outputs and the handle stay as they were
    for ci, cj, ct in ((nx - 1, ny, nx), (nx, ny - 1, nx), (nx, ny, nx - 1), (-1, ny, nx), (nx, -1, nx), (nx, ny, -1), (0, ny, nx)):
        rc, a2, b2, c2, s2 = raw(api, e, ci, cj, ct)
        assert rc == EINVAL and (a2 == UNTOUCHED).all() and (b2 == UNTOUCHED).all() and (c2 == -7).all() and s2 == [UNTOUCHED] * 8, (ci, cj, ct)
    assert api.depths(e.handle, None, -1, None, 0, None, 0, (C.c_double * 8)()) == EINVAL        # a negative cap, whatever it belongs to
    assert api.depths(e.handle, None, 0, None, 0, None, 0, None) == EINVAL and api.depths(None, None, 0, None, 0, None, 0, (C.c_double * 8)()) == EINVAL
    assert e.istep == 5 and all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    # two runs, and a second handle given the same steps: equal bytes
    twin = engine(api, nx, ny, "f64", "f32", ic=3)
    twin.step(5)
    for other in (e.depths(), twin.depths()):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(other[:3], (di, dj, top))) and other[3] == summ
    e.step(4); twin.step(4)
    assert_same_state(e, twin, "a vof_step behind vof_depths")


# ---------------------------------------------------------------------------- one physical check
def test_the_dam_break_front_advances_and_the_volume_holds(hip_api):
    """128 x 128 f64, -ic 1, 400 steps.  Asserted: FRONT_HI never decreases from record to record (the front of a collapsing
    column runs along the floor; F is held to [0, 1] and the wetted floor cells stay above the threshold); SUM dx dy is the
    volume vof_diagnostics reports to within the two derived bounds, so it stays within that verb's drift.  The front
    positions are printed, not judged."""
    n = 128
    e = engine(hip_api, n, n, "f64", "f32", ic=1)
    dx, dy = e.get_param("dx"), e.get_param("dy")
    di, _, _, summ = e.depths()
    v0 = summ["SUM"] * dx * dy
    last, drift = summ["FRONT_HI"], 0.0
    assert summ["FRONT_LO"] == 1 and v0 > 0
    for rec in range(1, 21):
        e.step(20)
        di, _, _, summ = e.depths()
        d = gauges.derive(di, summ, dx, dy)
        vol = e.diagnostics()["SUM_F"] * dx * dy
        bound = 2 * dnp.bound_of(e.get("F")[1:n + 1, 1:n + 1]) * dx * dy
        drift = max(drift, abs(vol - v0))
        print("istep %d front_lo %r front_hi %r (i = %d) top_j %d volume %r diagnostics %r drift so far %.3e" % (
            summ["ISTEP"], d["front_lo"], d["front_hi"], summ["FRONT_HI"], summ["TOP_J"], d["volume"], vol, drift))
        assert summ["FRONT_HI"] >= last, "record %d" % rec
        assert abs(d["volume"] - vol) <= bound and abs(d["volume"] - v0) <= drift + bound, "record %d" % rec
        last = summ["FRONT_HI"]
