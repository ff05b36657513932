"""vof_blobs on the GPU (include/vof2d.h): the list, its order, every integer and the labels are held exactly, the five sums
bit for bit, to the NumPy restatement of tests/_blobs_np.py applied to F, u, v read back (tests/test_blobs.py judges that
restatement on fields whose blobs are known by construction).  Every figure is printed before it is asserted.
"""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import _blobs_np as bnp
import _interface_np as inp
from test_blobs import sum_bound
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, blobs, halo_rows

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR, IPTR = C.POINTER(C.c_double), C.POINTER(C.c_int32)
PHASES = ("liquid", "gas")
INTS = list(bnp.INTS)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def own_rows(e):
    return max(e.own_lo, 1), min(e.own_hi, e.nx)


def restated(e, phase, thr=0.5):
    lo, hi = own_rows(e)
    return bnp.restate(e.get("F"), e.get("u"), e.get("v"), blobs.PHASES[phase], thr, lo=lo, hi=hi, row0=e.row_lo)


def hold_to_restatement(e, ctx, phase, thr=0.5, nan=False):
    rows, summ, lab = e.blobs(phase, thr, labels=True)
    want, wsum, wlab = restated(e, phase, thr)
    print(ctx, phase, "summary", summ, "restated", wsum)
    assert summ == dict(wsum, ISTEP=e.istep), ctx
    assert rows.shape == want.shape == (summ["BLOBS"], _abi.VOF_BLOB_N) and rows.dtype == np.float64, ctx
    assert lab.dtype == np.int32 and lab.shape == wlab.shape and np.array_equal(lab, wlab), ctx
    assert np.array_equal(rows[:, INTS], want[:, INTS]), ctx
    assert np.all(rows[:, bnp.SUM_WV + 1:] == 0), ctx
    if nan:                                         # a NaN has no bits to agree on: the same slots hold one, everything else is equal
        assert np.array_equal(np.isnan(rows), np.isnan(want)) and np.array_equal(bits(rows)[~np.isnan(rows)], bits(want)[~np.isnan(want)]), ctx
    else:
        bad = np.argwhere(bits(rows) != bits(want))
        assert len(bad) == 0, "%s: %d values differ, first at %s: %r vs %r" % (ctx, len(bad), bad[0], rows[tuple(bad[0])], want[tuple(bad[0])])
    first = rows[:, bnp.I0] * (e.ny + 2) + rows[:, bnp.J0]
    assert np.all(np.diff(first) > 0), ctx          # ascending first cells
    again = e.blobs(phase, thr)                      # without labels: the same rows
    assert again[0].tobytes() == rows.tobytes() and again[1] == summ, ctx
    return rows, summ, lab


def set_pattern(e, m, seed=5):
    """F = 0.9 / 0.2 (+ noise) from the interior pattern m, random u and v: the sums have something to add."""
    rng = np.random.default_rng(seed)
    e.set("F", bnp.with_ghosts(np.where(m > 0.5, 0.9, 0.2) + 0.05 * rng.random(m.shape)))
    e.set("u", rng.standard_normal((e.nx + 2, e.ny + 2)))
    e.set("v", rng.standard_normal((e.nx + 2, e.ny + 2)))


# ---------------------------------------------------------------------------- the shipped initial conditions
@pytest.mark.parametrize("ic", [1, 2, 3])
def test_200_f32_after_0_and_50_steps(hip_api, ic):
    e = engine(hip_api, 200, 200, "f32", "f32", ic=ic)
    dx, dy, Lx = e.get_param("dx"), e.get_param("dy"), 0.1
    for upto in (0, 50):
        e.step(upto - e.istep)
        for phase in PHASES:
            rows, summ, _ = hold_to_restatement(e, "200x200 f32 ic %d step %d" % (ic, upto), phase)
            if upto == 0 and ic == 3 and phase == "liquid":
                assert summ["BLOBS"] == 2                            # the drop and the pool (first cell (1, 1): the pool comes first)
                assert rows[0, bnp.CELLS] > rows[1, bnp.CELLS] > 100
            if upto == 0 and ic == 2 and phase == "gas":
                assert summ["BLOBS"] == 1                            # the bubble of 2dvof.py:150-151: centre (Lx / 2, Lx / 6)
                d = blobs.derived(rows, dx, dy)
                print("bubble centroid", d["xc"][0], d["yc"][0], "volume", d["volume"][0])
                assert abs(d["xc"][0] - Lx / 2) <= dx and abs(d["yc"][0] - Lx / 6) <= dy
                assert abs(d["volume"][0] - math.pi * (Lx / 12) ** 2) < 0.05 * math.pi * (Lx / 12) ** 2


# ---------------------------------------------------------------------------- constructed fields
def test_33x17_checkerboard_narrower_than_a_tile(hip_api):
    e = engine(hip_api, 33, 17, "f64", "f32", ic=1)
    set_pattern(e, bnp.checkerboard(33, 17))
    for phase in PHASES:
        _, summ, _ = hold_to_restatement(e, "33x17 checkerboard", phase)
        assert summ["MAX_CELLS"] == 1 and summ["BLOBS"] == summ["MEMBER_CELLS"] == (281 if phase == "liquid" else 280)


@pytest.mark.parametrize("nx,ny,dtype", [(130, 260, "f64"), (130, 516, "f32")])
def test_comb_across_tiles_and_chunks(hip_api, nx, ny, dtype):
    """Three and five column tiles (_interface_np.TILE = 128 columns), 130 rows = several row chunks of the marches and five
    chunks of the sum pass; the spine and some joins of the teeth cross the tile boundaries."""
    assert ny > 2 * inp.TILE and nx > 4 * bnp.CHUNK
    e = engine(hip_api, nx, ny, dtype, "f32", ic=1)
    set_pattern(e, bnp.comb(nx, ny))
    rows, summ, _ = hold_to_restatement(e, "%dx%d %s comb" % (nx, ny, dtype), "liquid")
    assert summ["BLOBS"] == 1 and tuple(rows[0, [bnp.IMIN, bnp.IMAX, bnp.JMIN, bnp.JMAX]]) == (1, nx - 2, 1, ny)
    _, gsum, _ = hold_to_restatement(e, "%dx%d %s comb" % (nx, ny, dtype), "gas")
    assert gsum["BLOBS"] == len(range(2, ny - 2, 4)) + 1           # the slot every join of two teeth closes, and the rest


def test_64x64_spiral_the_longest_chain(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    m = bnp.spiral(64)
    set_pattern(e, m)
    for phase in PHASES:
        _, summ, _ = hold_to_restatement(e, "64x64 spiral", phase)
        assert summ["BLOBS"] == 1 and summ["MAX_CELLS"] == int(m.sum() if phase == "liquid" else m.size - m.sum())


def test_66x66_checkerboard_more_blobs_than_scan_threads_and_the_capacity(hip_api):
    e = engine(hip_api, 66, 66, "f64", "f32", ic=1)
    set_pattern(e, bnp.checkerboard(66, 66))
    rows, summ, lab = hold_to_restatement(e, "66x66 checkerboard", "liquid")
    n = summ["BLOBS"]
    assert n == 2178 > inp.SCAN_THREADS
    s0 = (C.c_double * _abi.VOF_BLOB_SUM_N)()
    assert hip_api.blobs(e.handle, 0, 0.5, None, 0, None, 0, s0) == 0                     # sizing call: the same summary
    assert blobs.summary_of(list(s0)) == summ
    for cap in (n - 3, 1000, 1):
        buf = np.full((n, _abi.VOF_BLOB_N), -777.25)
        lbuf = np.full(lab.shape, -7, dtype=np.int32)
        s1 = (C.c_double * _abi.VOF_BLOB_SUM_N)()
        assert hip_api.blobs(e.handle, 0, 0.5, buf.ctypes.data_as(PTR), cap, lbuf.ctypes.data_as(IPTR), lbuf.nbytes, s1) == 0
        assert list(s1) == list(s0)                                                       # ... describes all blobs
        assert np.array_equal(bits(buf[:cap]), bits(rows[:cap])) and np.all(buf[cap:] == -777.25)
        assert np.array_equal(lbuf, lab)                                                  # the labels number all blobs
    big = np.full((n + 5, _abi.VOF_BLOB_N), -777.25)
    assert hip_api.blobs(e.handle, 0, 0.5, big.ctypes.data_as(PTR), n + 5, None, 0, s0) == 0
    assert np.array_equal(bits(big[:n]), bits(rows)) and np.all(big[n:] == -777.25)
    hold_to_restatement(e, "66x66 checkerboard", "gas")


def test_all_members_and_no_members(hip_api):
    e = engine(hip_api, 40, 130, "f32", "f32", ic=1)
    set_pattern(e, np.ones((40, 130)))
    rows, summ, lab = hold_to_restatement(e, "all liquid", "liquid")
    assert summ == {"BLOBS": 1, "MEMBER_CELLS": 40 * 130, "MAX_CELLS": 40 * 130, "ISTEP": 0} and np.all(lab == 0)
    assert tuple(rows[0, INTS]) == (1, 1, 40 * 130, 1, 40, 1, 130)
    rows, summ, lab = hold_to_restatement(e, "all liquid", "gas")
    assert summ == {"BLOBS": 0, "MEMBER_CELLS": 0, "MAX_CELLS": 0, "ISTEP": 0} and rows.shape == (0, _abi.VOF_BLOB_N) and np.all(lab == -1)


def test_nan_cells_in_F_split_and_a_nan_in_u_stays_in_its_blob(hip_api):
    e = engine(hip_api, 48, 140, "f64", "f32", ic=1)
    set_pattern(e, np.ones((48, 140)))
    F = e.get("F")
    F[1:-1, 130] = np.nan                            # a wall of NaN along i at j = 130, in the second tile
    F[20, 1:131] = np.nan                            # and one along j at i = 20 up to it
    e.set("F", F)
    rows, summ, lab = hold_to_restatement(e, "NaN walls", "liquid")
    assert summ["BLOBS"] == 3 and summ["MEMBER_CELLS"] == 48 * 140 - 48 - 129
    assert np.all(lab[:, 129] == -1) and np.all(lab[19, :130] == -1)
    _, gsum, glab = hold_to_restatement(e, "NaN walls", "gas")
    assert gsum["BLOBS"] == 0 and np.all(glab == -1)                  # a NaN is a member of neither
    u = e.get("u")
    u[30, 7] = np.nan                                # the west face of cell (30, 7), the east face of (29, 7): both in the third blob
    e.set("u", u)
    rows, _, lab = hold_to_restatement(e, "NaN in u", "liquid", nan=True)
    b = lab[29, 6]
    assert b == lab[28, 6] == 2 and np.isnan(rows[b, bnp.SUM_WU])
    assert not np.isnan(np.delete(rows, b, axis=0)).any() and not np.isnan(np.delete(rows[b], bnp.SUM_WU)).any()


def test_rectangular_cells(hip_api):
    e = engine(hip_api, 96, 130, "f64", "f32", ic=3, Lx=0.1, Ly=0.13)
    dx, dy = e.get_param("dx"), e.get_param("dy")
    assert dx != dy
    e.step(20)
    for phase in PHASES:
        rows, summ, _ = hold_to_restatement(e, "96x130 Lx != Ly ic 3 step 20", phase)
    liq = e.blobs("liquid")[0]
    d = blobs.derived(liq, dx, dy)
    vol = e.diagnostics()["SUM_F"] * dx * dy
    print("volumes", d["volume"], "of all liquid", vol)
    assert abs(d["volume"].sum() - vol) < 0.02 * vol                  # (what is left are the cells below the threshold)
    assert np.all((d["xc"] > 0) & (d["xc"] < 0.1) & (d["yc"] > 0) & (d["yc"] < 0.13))


# ---------------------------------------------------------------------------- the same bytes; reads only
def test_identical_bytes_and_a_twin(hip_api):
    a, b = (engine(hip_api, 130, 260, "f64", "f32", ic=3) for _ in range(2))
    a.step(30); b.step(30)
    for phase in PHASES:
        ra, rb, ra2 = a.blobs(phase, 0.5, True), b.blobs(phase, 0.5, True), a.blobs(phase, 0.5, True)
        assert ra[0].tobytes() == ra2[0].tobytes() == rb[0].tobytes()
        assert ra[2].tobytes() == ra2[2].tobytes() == rb[2].tobytes() and ra[1] == ra2[1] == rb[1]


@pytest.mark.parametrize("dtype,ic", [("f64", 1), ("f32", 3)])
def test_reads_only(hip_api, dtype, ic):
    a, b = (engine(hip_api, 128, 128, dtype, "f32", ic=ic) for _ in range(2))
    a.step(7); b.step(7)
    before = {n: a.get(n) for n in FIELDS}
    warn = a.get_counter("courant_violations")
    for phase in PHASES:
        a.blobs(phase, 0.5, True)
    assert a.istep == 7 and a.get_counter("courant_violations") == warn
    assert all(np.array_equal(a.get(n), before[n]) for n in FIELDS)
    a.step(20); b.step(20)
    assert_same_state(a, b, "128x128 %s: vof_step(20) behind vof_blobs" % dtype)
    a.blobs("gas")
    a.step_mg(3, 2, "rel"); b.step_mg(3, 2, "rel")
    assert_same_state(a, b, "128x128 %s: vof_step_mg behind vof_blobs" % dtype)


# ---------------------------------------------------------------------------- strips
@pytest.mark.parametrize("nstrips", [2, 3])
def test_strips_combine_to_the_domain(hip_api, nstrips):
    nx, ny, W = 96, 64, halo_rows(10)
    full = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    full.step(20)
    bounds = [round(k * nx / nstrips) for k in range(nstrips + 1)]
    strips = []
    for k in range(nstrips):
        r = (max(0, bounds[k] + 1 - W), min(nx + 1, bounds[k + 1] + W))
        s = engine(hip_api, nx, ny, "f64", "f32", ic=3, rows=r, own=(bounds[k] + 1, bounds[k + 1]))
        for f in ("F", "u", "v", "p"):
            s.set(f, full.get(f, r), rows=r)
        s.istep = full.istep
        strips.append(s)
    for phase in PHASES:
        parts = [hold_to_restatement(s, "strip %d..%d" % (s.own_lo, s.own_hi), phase) for s in strips]
        rows, summ, lab = blobs.combine(parts, ny)
        one, osum, olab = hold_to_restatement(full, "the domain", phase)
        assert summ == osum and np.array_equal(lab, olab)
        assert rows.shape == one.shape and np.array_equal(rows[:, INTS], one[:, INTS])
        terms = bnp.cell_terms(full.get("F"), full.get("u"), full.get("v"), blobs.PHASES[phase], 1, nx, 0)
        for b in range(len(one)):
            for k, slot in enumerate(bnp.SUMS):
                bound = sum_bound(terms[:, :, k][olab == b])
                print(phase, "blob", b, "slot", slot, "strips", rows[b, slot], "domain", one[b, slot], "bound", bound)
                assert abs(rows[b, slot] - one[b, slot]) <= bound
    if nstrips == 2:
        assert len(blobs.combine([s.blobs("liquid", 0.5, True) for s in strips], ny)[0]) < sum(s.blobs("liquid")[1]["BLOBS"] for s in strips)   # the pool was joined


# ---------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_alone(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.step(2)
    before = {n: e.get(n) for n in FIELDS}
    buf = np.full((16, _abi.VOF_BLOB_N), -1.5)
    lab = np.full((64, 64), -9, dtype=np.int32)
    s = (C.c_double * _abi.VOF_BLOB_SUM_N)(*([-1.5] * _abi.VOF_BLOB_SUM_N))
    rp, lp = buf.ctypes.data_as(PTR), lab.ctypes.data_as(IPTR)
    for phase in (-1, 2, 7):
        assert hip_api.blobs(e.handle, phase, 0.5, rp, 16, lp, lab.nbytes, s) == _abi.VOF_EINVAL, phase
    for thr in (math.nan, 0.0, 1.0, -0.5, 1.5, math.inf):
        assert hip_api.blobs(e.handle, 0, thr, rp, 16, lp, lab.nbytes, s) == _abi.VOF_EINVAL, thr
    assert hip_api.blobs(e.handle, 0, 0.5, rp, -1, lp, lab.nbytes, s) == _abi.VOF_EINVAL
    assert hip_api.blobs(e.handle, 0, 0.5, None, 16, lp, lab.nbytes, s) == _abi.VOF_EINVAL
    assert hip_api.blobs(e.handle, 0, 0.5, rp, 16, lp, lab.nbytes, None) == _abi.VOF_EINVAL
    for nbytes in (lab.nbytes - 4, lab.nbytes + 4, 0):
        assert hip_api.blobs(e.handle, 0, 0.5, rp, 16, lp, nbytes, s) == _abi.VOF_EINVAL, nbytes
    assert hip_api.blobs(None, 0, 0.5, None, 0, None, 0, s) == _abi.VOF_EINVAL
    assert np.all(buf == -1.5) and np.all(lab == -9) and list(s) == [-1.5] * _abi.VOF_BLOB_SUM_N
    assert e.istep == 2 and all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    twin = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    twin.step(4); e.step(2)
    assert_same_state(e, twin, "after the refusals")


# ---------------------------------------------------------------------------- the command line
def test_cli_writes_the_csv(hip_api, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "2dvof.py"), "-ic", "3", "--nx", "64", "--ny", "64", "--dtype", "f64", "--steps", "20",
                        "--blobs-every", "10"], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    text = open(os.path.join(str(tmp_path), "data", "blobs.csv")).read().strip().split("\n")
    assert text[0] == blobs.CSV_HEADER == "istep,blob,cells,volume,xc,yc,uc,vc,imin,imax,jmin,jmax"
    got = [line.split(",") for line in text[1:]]
    e = engine(hip_api, 64, 64, "f64", "f32", ic=3)
    dx, dy = e.get_param("dx"), e.get_param("dy")
    want = []
    for _ in range(2):
        e.step(10)
        rows, summ = e.blobs()
        d = blobs.derived(rows, dx, dy)
        assert summ["BLOBS"] >= 2
        for b, row in enumerate(rows):
            want.append([e.istep, b, int(row[bnp.CELLS])] + [float(d[k][b]) for k in ("volume", "xc", "yc", "uc", "vc")] +
                        [int(row[k]) for k in (bnp.IMIN, bnp.IMAX, bnp.JMIN, bnp.JMAX)])
    assert len(got) == len(want) and {int(g[0]) for g in got} == {10, 20}
    for g, w in zip(got, want):
        assert [int(x) for x in g[:3] + g[8:]] == w[:3] + w[8:], (g, w)
        assert [float(x) for x in g[3:8]] == w[3:8], (g, w)
