"""vof_curvature on the GPU (include/vof2d.h): rows and summary are held, bit for bit, to the NumPy restatement of
tests/_curvature_np.py applied to the field F read back (tests/test_curvature.py judges that restatement against analysis).
Every figure is printed before it is asserted.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _curvature_np as cnp
import _interface_np as inp
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, curvature
from vof2d.engine import VofError

pytestmark = pytest.mark.gpu
PTR = C.POINTER(C.c_double)
EPS = 1e-6
DOUBLES = [k for k in cnp.SUMMARY if k not in ("ROWS", "DEGENERATE", "VALID")]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def restated(e, eps=EPS):
    return cnp.restate(e.get("F"), eps, e.get_param("dx"), e.get_param("dy"), R=inp.chunk_rows(e.nx, e.ny))


def hold_to_restatement(e, ctx, eps=EPS, nan=False):
    rows, summ = e.curvature(eps)
    want, wsum = restated(e, eps)
    print(ctx, "summary", summ, "restated", wsum)
    assert rows.shape == want.shape == (summ["ROWS"], _abi.VOF_CURV_N) and rows.dtype == np.float64, ctx
    assert all(summ[k] == wsum[k] for k in ("ROWS", "DEGENERATE", "VALID")) and summ["ISTEP"] == e.istep, ctx
    if nan:                                     # a NaN has no bits to agree on: the same slots hold one, everything else is equal
        assert np.array_equal(np.isnan(rows), np.isnan(want)) and np.array_equal(rows, want, equal_nan=True), ctx
        for k in DOUBLES:
            assert summ[k] == wsum[k] or (math.isnan(summ[k]) and math.isnan(wsum[k])), "%s %s %r vs %r" % (ctx, k, summ[k], wsum[k])
    else:
        bad = np.argwhere(bits(rows) != bits(want))
        assert len(bad) == 0, "%s: %d values differ, first at %s: %r vs %r" % (ctx, len(bad), bad[0], rows[tuple(bad[0])], want[tuple(bad[0])])
        for k in DOUBLES:
            assert bits(summ[k]) == bits(wsum[k]), "%s %s %r vs %r" % (ctx, k, summ[k], wsum[k])
    keys = rows[:, 0] * (e.ny + 2) + rows[:, 1]
    assert np.all(np.diff(keys) > 0), ctx       # strictly ascending (i, j)
    return rows, summ


# ---------------------------------------------------------------------------- equal to the restatement
# ny at one column tile (64 * V = 128 for both dtypes) minus 1, exactly, plus 1; nx no multiple of the 4-row chunk, and smaller than
# one; the small golden shapes.  Rectangular grids of the default 0.1 x 0.1 domain have dx != dy.
SHAPES = [(33, 17, 3, 30), (24, 40, 2, 30), (48, 80, 1, 40), (30, 127, 3, 24), (29, 128, 2, 24), (31, 129, 1, 40), (3, 129, 3, 0)]


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny,ic,steps", SHAPES)
def test_initial_states_at_step_0_and_later(hip_api, nx, ny, ic, steps, dtype):
    assert inp.chunk_rows(nx, ny) == 4
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    for upto in sorted({0, steps}):
        e.step(upto - e.istep)
        rows, summ = hold_to_restatement(e, "%dx%d %s ic %d step %d" % (nx, ny, dtype, ic, upto))
        if ic != 1 and nx > 3:                   # (the dam of -ic 1 is a step function: no mixed cell until it moves; three rows of -ic 3 hold a pool that ends on a cell face)
            assert summ["ROWS"] > 0
        seg, _ = e.interface(EPS)                # the cells and the order of vof_interface
        assert np.array_equal(rows[:, :2], seg[:, :2])
        if dtype == "f64" and upto == steps:     # the solver's own kappa, bit for bit (the calls above have settled the ghost cells); no step follows the verb
            e.get_normal_young()
            kappa = e.get("kappa")
            own = kappa[rows[:, 0].astype(int), rows[:, 1].astype(int)]
            bad = np.flatnonzero(bits(own) != bits(rows[:, curvature.KAPPA_CSF]))
            assert len(bad) == 0, "KAPPA_CSF differs from kappa in %d rows, first %r: %r vs %r" % (len(bad), rows[bad[0], :2] if len(bad) else None,
                                                                                                 rows[bad[0], curvature.KAPPA_CSF] if len(bad) else None, own[bad[0]] if len(bad) else None)


def test_interfaces_across_tile_edges_and_on_walls_f64(hip_api):
    """130 x 260: three column tiles; the face of the dam crosses j = 128 | 129 within single rows, the drop over the pool has rows in
    two tiles and its pool meets both side walls."""
    for ic in (1, 3):
        e = engine(hip_api, 130, 260, "f64", "f32", ic=ic)
        e.step(20)
        rows, summ = hold_to_restatement(e, "130x260 f64 ic %d step 20" % ic)
        tiles = set(((rows[:, 1] - 1) // inp.TILE).astype(int))
        print("tiles holding rows", tiles)
        assert len(tiles) >= 2
        if ic == 3:
            assert rows[:, 0].min() == 1 and rows[:, 0].max() == 130 and summ["VALID"] > 0


def random_field(nx, ny, seed, nans):
    rng = np.random.default_rng(seed)
    F = rng.random((nx + 2, ny + 2))
    F[rng.random(F.shape) < 0.25] = 0.0                      # plateaus of exact 0 and 1: full and empty cells, valid stencils
    F[rng.random(F.shape) < 0.25] = 1.0
    F[: nx // 3, : ny // 2] = 1.0
    F[: nx // 3, ny // 2 + 1:] = 0.0
    if nx >= 4:
        F[-(nx // 4):, :] = 0.0
    for _ in range(nans):
        F[rng.integers(0, nx + 2), rng.integers(0, ny + 2)] = np.nan
    return F


@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny", [(37, 150), (3, 129)])
def test_random_values_plateaus_and_nans(hip_api, nx, ny, dtype):
    e = engine(hip_api, nx, ny, dtype, "f32", ic=1)
    e.set("F", random_field(nx, ny, 5, 0))
    rows, summ = hold_to_restatement(e, "%dx%d %s random" % (nx, ny, dtype))
    if nx > 3:
        assert 0 < summ["VALID"] < summ["ROWS"] and {0.0, 1.0} == set(rows[:, curvature.AXIS])
    e.set("F", random_field(nx, ny, 5, 6))
    rows, summ = hold_to_restatement(e, "%dx%d %s random with NaNs" % (nx, ny, dtype), nan=True)
    assert np.isnan(rows[:, 2:]).any()


def test_all_gas_has_no_rows(hip_api):
    e = engine(hip_api, 40, 30, "f64", "f32", ic=1)
    e.set("F", np.zeros((42, 32)))
    rows, summ = hold_to_restatement(e, "F = 0 everywhere")
    assert len(rows) == 0 and summ["ROWS"] == 0 and summ["SUM_K"] == 0.0 and summ["SUM_CSF"] == 0.0
    assert summ["MAX_K"] == summ["MAX_CSF"] == -math.inf and summ["MIN_K"] == summ["MIN_CSF"] == math.inf
    d = curvature.derive(summ)
    assert d["rows"] == 0 and math.isnan(d["k_mean"])


def test_behind_forced_k_tm_batches(hip_api):
    e = engine(hip_api, 256, 256, "f64", "f32", ic=3)
    e.set_param("fuse_tm", 1)
    e.step(40)
    print("tm_steps", e.get_counter("tm_steps"))
    hold_to_restatement(e, "256x256 f64 ic 3, fuse_tm = 1, behind vof_step(40)")   # first: the handle is ahead, its ghost cells virtual


# ---------------------------------------------------------------------------- order and capacity
def test_capacity_sizing_call_and_identical_bytes(hip_api):
    e = engine(hip_api, 96, 96, "f64", "f32", ic=3)
    e.step(10)
    rows, summ = hold_to_restatement(e, "96x96 f64 ic 3 step 10")
    n = summ["ROWS"]
    assert n > 8
    s0 = (C.c_double * _abi.VOF_CURV_SUM_N)()
    assert hip_api.curvature(e.handle, EPS, None, 0, s0) == 0                     # sizing call: the same summary
    assert curvature.summary_of(list(s0)) == summ and all(x == 0.0 for x in list(s0)[_abi.VOF_CURV_SUM_ISTEP + 1:])
    buf = np.full((n, _abi.VOF_CURV_N), -777.25)
    s1 = (C.c_double * _abi.VOF_CURV_SUM_N)()
    assert hip_api.curvature(e.handle, EPS, buf.ctypes.data_as(PTR), n - 3, s1) == 0
    assert list(s1) == list(s0)                                                   # ... describes all rows
    assert np.array_equal(bits(buf[:n - 3]), bits(rows[:n - 3])) and np.all(buf[n - 3:] == -777.25)
    big = np.full((n + 5, _abi.VOF_CURV_N), -777.25)
    assert hip_api.curvature(e.handle, EPS, big.ctypes.data_as(PTR), n + 5, s1) == 0
    assert np.array_equal(bits(big[:n]), bits(rows)) and np.all(big[n:] == -777.25)
    again, summ2 = e.curvature()
    assert again.tobytes() == rows.tobytes() and summ2 == summ
    wide, wsumm = hold_to_restatement(e, "eps = 0.05", eps=0.05)                  # the caller's eps decides what is mixed
    assert wsumm["ROWS"] < n


# ---------------------------------------------------------------------------- reads only
def test_reads_only(hip_api):
    a, b = (engine(hip_api, 128, 128, "f64", "f32", ic=1) for _ in range(2))
    a.step(7); b.step(7)
    before = {n: a.get(n) for n in FIELDS}
    warn = a.get_counter("courant_violations")
    a.curvature()
    assert a.istep == 7 and a.get_counter("courant_violations") == warn
    assert all(np.array_equal(a.get(n), before[n]) for n in FIELDS)
    a.step(10); b.step(10)
    a.curvature()
    a.step(10); b.step(10)
    assert_same_state(a, b, "128x128 f64: curvature between steps")


# ---------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_alone(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.step(2)
    before = {n: e.get(n) for n in FIELDS}
    buf = np.full((16, _abi.VOF_CURV_N), -1.5)
    s = (C.c_double * _abi.VOF_CURV_SUM_N)(*([-1.5] * _abi.VOF_CURV_SUM_N))
    for eps in (math.nan, -1e-9, 0.5, 0.75, math.inf):
        assert hip_api.curvature(e.handle, eps, buf.ctypes.data_as(PTR), 16, s) == _abi.VOF_EINVAL, eps
    assert hip_api.curvature(e.handle, EPS, buf.ctypes.data_as(PTR), 16, None) == _abi.VOF_EINVAL
    assert hip_api.curvature(e.handle, EPS, None, 16, s) == _abi.VOF_EINVAL
    assert hip_api.curvature(e.handle, EPS, buf.ctypes.data_as(PTR), -1, s) == _abi.VOF_EINVAL
    assert hip_api.curvature(None, EPS, None, 0, s) == _abi.VOF_EINVAL
    assert np.all(buf == -1.5) and list(s) == [-1.5] * _abi.VOF_CURV_SUM_N
    assert e.istep == 2 and all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    twin = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    twin.step(4); e.step(2)
    assert_same_state(e, twin, "after the refusals")


def test_a_strip_and_a_phased_step_are_refused(hip_api):
    s = engine(hip_api, 128, 128, "f64", "f32", ic=3, rows=(0, 80), own=(1, 60))
    before = {n: s.get(n) for n in FIELDS}
    with pytest.raises(VofError, match="VOF_ESTATE") as err:
        s.curvature()
    assert "whole domain" in str(err.value)
    assert s.istep == 0 and all(np.array_equal(s.get(n), before[n]) for n in FIELDS)
    assert s.interface()[1]["SEGMENTS"] > 0                              # vof_interface works on it
    e = engine(hip_api, 64, 64, "f64", "f32", ic=3)
    e.step(1)
    e.step_phase(0)
    with pytest.raises(VofError, match="VOF_ESTATE"):
        e.curvature()
    e.step_phase(1); e.step_phase(2)
    assert e.curvature()[1]["ISTEP"] == 2 == e.istep


# ---------------------------------------------------------------------------- the command line
def test_cli_writes_the_rows_and_the_csv(hip_api, tmp_path, monkeypatch):
    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    argv = ["-ic", "3", "--nx", "64", "--ny", "64", "--dtype", "f64", "--curvature-every", "5", "--steps", "12"]
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    data = os.path.join(str(tmp_path), "data")
    assert sorted(f for f in os.listdir(data) if f.startswith("curvature_")) == ["curvature_000005.npy", "curvature_000010.npy"]
    text = open(os.path.join(data, "curvature.csv")).read().strip().split("\n")
    assert text[0] == curvature.CSV_HEADER and [t.split(",")[0] for t in text[1:]] == ["5", "10"]
    e = engine(hip_api, 64, 64, "f64", "f32", ic=3)
    for line in text[1:]:
        e.step(5)
        rows, summ = e.curvature()
        assert line == curvature.csv_line(summ) and summ["ROWS"] > 0
        assert np.load(os.path.join(data, "curvature_%06d.npy" % e.istep)).tobytes() == rows.tobytes()
