"""vof_diagnostics and vof_step_diag on the GPU (include/vof2d.h).

vof_diagnostics is held to the NumPy restatement of tests/_diag_np.py applied to the fields read back: extrema, CELLS and
ISTEP with ==, every sum against math.fsum of the restated terms within n 2^-52 fsum(|t|) (derived in that module, not
measured).  vof_step_diag is held to its definition, bit for bit: the loop "step `every` steps; vof_diagnostics" on a twin.
Every figure is printed before it is asserted.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _diag_np as dnp
import _interface_np as inp
import _reduce_np as rnp
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, diag, halo_rows
from vof2d.engine import VofError

pytestmark = pytest.mark.gpu

TM_GRID = (2048, 2048, "f32", 2)          # vof_step batches its steady-state steps in the k_tm form here (tests/test_step_mg_gpu.py)


def restated(e):
    """(terms, extrema, cells) of the restatement on the fields of e as vof_get_field returns them, on its owned cells."""
    lo, hi = max(e.own_lo, 1), min(e.own_hi, e.nx)
    return dnp.restate(e.get("F"), e.get("u"), e.get("v"), e.get_param("dxi"), e.get_param("dyi"), e.get_param("rho_g"),
                       e.get_param("rho_l"), lo=lo, hi=hi, row0=e.row_lo)


def hold_to_restatement(e, ctx, bits=False):
    """bits: the sums also equal, bit for bit, the restated order of the reduction with the handle's chunk length"""
    raw = e.diagnostics()
    terms, ext, cells = restated(e)
    R = inp.diag_chunk_rows(e.nx, e.ny, e.row_lo, e.row_hi) if bits else None
    dnp.check(raw, terms, ext, cells, istep=e.istep, ctx=ctx, say=print, R=R)
    return raw


def vec(raw):
    return np.array([raw[k] for k in diag.NAMES] + [0.0] * (_abi.VOF_DIAG_N - len(diag.NAMES)))


# ---------------------------------------------------------------------------- equal to the restatement
@pytest.mark.parametrize("ic", [1, 2, 3])
def test_200_f32_after_0_1_and_50_steps(hip_api, ic):
    e = engine(hip_api, 200, 200, "f32", "f32", ic=ic)
    for upto in (0, 1, 50):
        e.step(upto - e.istep)
        raw = hold_to_restatement(e, "200x200 f32 ic %d step %d" % (ic, upto), bits=True)
        assert raw["CELLS"] == 200 * 200 and raw["SUM_F"] > 0
    assert raw["MAX_U"] > 0 and raw["MAX_DIV"] > 0 and raw["SUM_KE"] > 0


@pytest.mark.parametrize("nx,ny,ic,kw", [(96, 130, 3, {"Lx": 0.1, "Ly": 0.13}), (33, 17, 2, {})])
def test_small_and_rectangular_f64(hip_api, nx, ny, ic, kw):
    e = engine(hip_api, nx, ny, "f64", "f32", ic=ic, **kw)
    if kw:
        assert e.get_param("dxi") != e.get_param("dyi")
    for upto in (0, 1, 20):
        e.step(upto - e.istep)
        hold_to_restatement(e, "%dx%d f64 ic %d step %d" % (nx, ny, ic, upto), bits=True)


def test_more_partials_than_folding_threads_f64(hip_api):
    """1100 x 130: the rule gives 2-row chunks, 550 chunks x 2 tiles = 1100 waves = 275 blocks, so threads 0 .. 18 of
    k_row_finish fold two partials each; the second tile is ragged (2 of 128 columns).  Sums and extrema with ==."""
    nx, ny = 1100, 130
    R = inp.diag_chunk_rows(nx, ny)
    assert R == 2 and rnp.blocks(nx, ny, R) == 275 > 256
    e = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    for upto in (0, 1):
        e.step(upto - e.istep)
        hold_to_restatement(e, "%dx%d f64 ic 3 step %d" % (nx, ny, upto), bits=True)


def test_1024_f64_after_20_steps(hip_api):
    e = engine(hip_api, 1024, 1024, "f64", "f32", ic=1)
    e.step(20)
    raw = hold_to_restatement(e, "1024x1024 f64 ic 1 step 20")
    d = diag.derive(raw, e.get_param("dx"), e.get_param("dy"), e.get_param("dt"), 1024, 1024)
    print(d)
    # the dam of 2dvof.py:141-143 has hardly moved after 20 steps (8e-5 s): its volume and centroid are those of the block
    # Lx / 3 x Ly / 2 to within the one cell (dx = 9.8e-5) by which the cells' node test overshoots each edge
    assert abs(d["volume"] - 0.1 / 3 * 0.05) < 2e-5 and abs(d["xc"] - 0.1 / 6) < 1e-4 and abs(d["yc"] - 0.025) < 1e-4
    assert 0 < d["cfl"] < 0.25


def test_behind_a_k_tm_batch(hip_api):
    nx, ny, dtype, ic = TM_GRID
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    e.step(40)
    assert e.get_counter("tm_steps") >= 2
    raw = e.diagnostics()                      # first: the handle is ahead, its ghost cells virtual
    terms, ext, cells = restated(e)
    dnp.check(raw, terms, ext, cells, istep=40, ctx="2048x2048 f32 ic 2 behind vof_step(40)", say=print)


# ---------------------------------------------------------------------------- read-only and reproducible
@pytest.mark.parametrize("nx,ny,dtype,ic", [(256, 256, "f64", 1), TM_GRID])
def test_reads_only_and_interleaves_with_vof_step(hip_api, nx, ny, dtype, ic):
    a, b = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(2))
    a.step(7); b.step(7)
    before = {n: a.get(n) for n in FIELDS}
    warn = a.get_counter("courant_violations")
    r1 = a.diagnostics()
    r2 = a.diagnostics()
    assert r1 == r2                             # identical bits (no NaN in this state)
    assert a.istep == 7 and a.get_counter("courant_violations") == warn
    assert all(np.array_equal(a.get(n), before[n]) for n in FIELDS)
    for _ in range(2):
        a.step(7); b.step(7)
        a.diagnostics()
    if (nx, ny, dtype, ic) == TM_GRID:
        assert a.get_counter("tm_steps") >= 2
    assert_same_state(a, b, "%dx%d %s: diagnostics between vof_step(7) calls" % (nx, ny, dtype))


# ---------------------------------------------------------------------------- vof_step_diag held to its definition
def loop_on_a_twin(b, nsteps, every, K=0, crit="rel"):
    rows = []
    for _ in range(nsteps // every):
        b.step_mg(every, K, crit) if K else b.step(every)
        rows.append(vec(b.diagnostics()))
    if nsteps % every:
        b.step_mg(nsteps % every, K, crit) if K else b.step(nsteps % every)
    return np.array(rows).reshape(len(rows), _abi.VOF_DIAG_N)


def hold_to_definition(hip_api, nx, ny, dtype, ic, nsteps, every, K=0, flags=0, single=True):
    a = engine(hip_api, nx, ny, dtype, "f32", ic=ic, flags=flags)
    b = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    ctx = "%dx%d %s ic %d: step_diag(%d, %d, K = %d, flags %d)" % (nx, ny, dtype, ic, nsteps, every, K, flags)
    rows = a.step_diag(nsteps, every, K, "rel")
    want = loop_on_a_twin(b, nsteps, every, K)
    print(ctx, "rows", rows.shape, "last", rows[-1] if len(rows) else None)
    assert rows.shape == (nsteps // every, _abi.VOF_DIAG_N) and rows.dtype == np.float64
    assert np.array_equal(rows, want), ctx
    assert list(rows[:, diag.ISTEP]) == [float(every * (r + 1)) for r in range(nsteps // every)]
    assert_same_state(a, b, ctx)
    if single:
        c = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
        c.step_mg(nsteps, K, "rel") if K else c.step(nsteps)
        assert_same_state(a, c, ctx + " against one call of nsteps")
    # ... and once more from the state the call left
    rows = a.step_diag(2 * every, every, K, "rel")
    want = loop_on_a_twin(b, 2 * every, every, K)
    assert np.array_equal(rows, want), ctx + " (second call)"
    assert_same_state(a, b, ctx + " (second call)")
    return a


@pytest.mark.parametrize("every", [1, 5])
def test_step_diag_128_f64_with_a_remainder(hip_api, every):
    a = hold_to_definition(hip_api, 128, 128, "f64", 1, 23, every)
    hold_to_restatement(a, "128x128 f64 behind step_diag")


def test_step_diag_on_the_k_tm_grid(hip_api):
    nx, ny, dtype, ic = TM_GRID
    a = hold_to_definition(hip_api, nx, ny, dtype, ic, 32, 8)
    assert a.get_counter("tm_steps") >= 2


def test_step_diag_with_multigrid_steps(hip_api):
    hold_to_definition(hip_api, 256, 256, "f64", 1, 12, 4, K=3)


@pytest.mark.parametrize("K", [0, 3])
def test_step_diag_without_graphs(hip_api, K):
    hold_to_definition(hip_api, 128, 128, "f64", 2, 11, 3, K=K, flags=_abi.VOF_FLAG_NO_GRAPH, single=False)


def test_step_diag_of_no_steps_and_of_fewer_than_every(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    assert e.step_diag(0, 5).shape == (0, _abi.VOF_DIAG_N) and e.istep == 0
    assert e.step_diag(3, 5).shape == (0, _abi.VOF_DIAG_N) and e.istep == 3          # a remainder only: stepped, no row
    twin = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    twin.step(3)
    assert_same_state(e, twin, "step_diag(3, 5)")


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
            parts = [hold_to_restatement(s, "strip %d..%d step %d" % (s.own_lo, s.own_hi, step)) for s in strips]
            whole = diag.combine(parts)
            one = full.diagnostics()
            terms, ext, cells = restated(full)
            dnp.check(whole, terms, ext, cells, istep=step, ctx="%d strips combined, step %d" % (nstrips, step), say=print)
            assert all(whole[k] == one[k] for k in dnp.EXTREMA)
            assert sum(p["CELLS"] for p in parts) == nx * ny == one["CELLS"]


# ---------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_alone(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.step(2)
    before = {n: e.get(n) for n in FIELDS}
    out = (C.c_double * (4 * _abi.VOF_DIAG_N))()
    done = C.c_int64(-1)
    REL = _abi.VOF_RESID_REL
    assert hip_api.diagnostics(e.handle, None) == _abi.VOF_EINVAL
    for args in ((4, 0, 0, REL, out, 4), (4, -1, 0, REL, out, 4), (-1, 1, 0, REL, out, 4), (4, 1, 0, REL, None, 4), (4, 1, 0, REL, out, 3),
                 (4, 1, -1, REL, out, 4), (4, 1, 2, 7, out, 4)):
        assert hip_api.step_diag(e.handle, *args, C.byref(done)) == _abi.VOF_EINVAL, args
    assert e.istep == 2 and all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    # a bad criterion does not matter without multigrid steps; a NULL out does not matter with no row due
    assert hip_api.step_diag(e.handle, 1, 1, 0, 7, out, 4, C.byref(done)) == 0 and done.value == 1 and e.istep == 3
    assert hip_api.step_diag(e.handle, 1, 2, 0, REL, None, 0, None) == 0 and e.istep == 4


def test_step_diag_on_a_strip_is_refused(hip_api):
    s = engine(hip_api, 128, 128, "f64", "f32", ic=1, rows=(0, 80), own=(1, 60))
    before = {n: s.get(n) for n in FIELDS}
    with pytest.raises(VofError, match="VOF_ESTATE") as err:
        s.step_diag(4, 2)
    assert "whole domain" in str(err.value)
    assert s.istep == 0 and all(np.array_equal(s.get(n), before[n]) for n in FIELDS)
    raw = hold_to_restatement(s, "strip rows 0..80 owning 1..60")          # vof_diagnostics works on it
    assert raw["CELLS"] == 60 * 128


def test_a_strip_that_owns_nothing(hip_api):
    """No cell is reported: the pass is not launched and k_row_finish alone forms the row, from the `init` of kDiagRow."""
    s = engine(hip_api, 64, 64, "f64", "f32", ic=1, rows=(0, 40), own=(2, 1))
    raw = s.diagnostics()
    print(raw)
    want = {k: 0.0 for k in diag.NAMES}
    want.update(ISTEP=0, CELLS=0, MIN_F=math.inf, MAX_F=-math.inf)
    assert raw == want


# ---------------------------------------------------------------------------- a NaN is reported, not hidden
def test_a_nan_is_reported(hip_api):
    e = engine(hip_api, 96, 64, "f64", "f32", ic=1)
    e.step(5)
    u = e.get("u")
    u[40, 30] = np.nan                          # an interior face: ordinary data through vof_set_field
    e.set("u", u)
    raw = e.diagnostics()
    print(raw)
    assert raw["MAX_U"] == math.inf and raw["MAX_DIV"] == math.inf and math.isnan(raw["SUM_KE"]) and math.isnan(raw["SUM_DIV2"])
    assert raw["MAX_V"] < math.inf and not math.isnan(raw["SUM_F"]) and raw["CELLS"] == 96 * 64
    terms, ext, cells = restated(e)
    dnp.check(raw, terms, ext, cells, istep=5, ctx="a NaN in u")
    F = e.get("F")
    F[10, 10] = np.nan
    e.set("F", F)
    raw = e.diagnostics()
    assert raw["MIN_F"] == -math.inf and raw["MAX_F"] == math.inf and math.isnan(raw["SUM_F"])


# ---------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("more", [[], ["--pressure-solver", "mg", "--mg-cycles", "2"], ["--verbs"]])
def test_cli_writes_the_csv(hip_api, tmp_path, monkeypatch, more):
    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    base = ["-ic", "1", "--nx", "64", "--ny", "48", "--dtype", "f64", "--diag-every", "10"] + more
    argv = base + ["--steps", "30"]
    lines = []
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=lambda *a: lines.append(" ".join(str(x) for x in a))) == 0
    text = open(os.path.join(str(tmp_path), "data", "diagnostics.csv")).read().strip().split("\n")
    assert text[0].split(",") == ["istep", "time"] + list(diag.DERIVED)
    rows = [dict(zip(text[0].split(","), r.split(","))) for r in text[1:]]
    assert [int(r["istep"]) for r in rows] == [10, 20, 30]
    e = engine(hip_api, 64, 48, "f64", "f32", ic=1)
    K = 2 if "--mg-cycles" in more else 0
    if K:
        e.set_param("mg_coarse_block", 1)        # (--mg-coarse block, the default of the command line)
    for r in rows:
        e.step_mg(10, K, "abs") if K else e.step(10)
        d = diag.derive(e.diagnostics(), e.get_param("dx"), e.get_param("dy"), e.get_param("dt"), 64, 48)
        assert float(r["volume"]) == d["volume"] and float(r["div_max"]) == d["div_max"] and float(r["time"]) == int(r["istep"]) * e.get_param("dt")
    # a resumed run appends, without a second header
    monkeypatch.chdir(tmp_path)
    assert cli.run(cli.parse_args(argv + ["--save-every", "30"]), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    argv2 = base + ["--steps", "50", "--resume", "data/00000030.npz"]
    assert cli.run(cli.parse_args(argv2), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    text = open(os.path.join(str(tmp_path), "data", "diagnostics.csv")).read().strip().split("\n")
    assert [t.split(",")[0] for t in text] == ["istep", "10", "20", "30", "40", "50"]
