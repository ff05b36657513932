"""vof_interface on the GPU (include/vof2d.h): rows and summary are held, bit for bit, to the NumPy restatement of
tests/_interface_np.py applied to the field F read back (tests/test_interface.py judges that restatement by geometry).
Every figure is printed before it is asserted.
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

import _interface_np as inp
import _reduce_np as rnp
from test_diag_gpu import TM_GRID
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, halo_rows, interface

pytestmark = pytest.mark.gpu
PTR = C.POINTER(C.c_double)
EPS = 1e-6


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def restated(e, eps=EPS):
    """(rows, summary) of the restatement on F as vof_get_field returns it, on the handle's owned cells."""
    lo, hi = max(e.own_lo, 1), min(e.own_hi, e.nx)
    rows, summary, _ = inp.restate(e.get("F"), eps, e.get_param("dx"), e.get_param("dy"), lo=lo, hi=hi, row0=e.row_lo,
                                   R=inp.chunk_rows(e.nx, e.ny, e.row_lo, e.row_hi))
    return rows, summary


def hold_to_restatement(e, ctx, eps=EPS, nan=False):
    rows, summ = e.interface(eps)
    want, wsum = restated(e, eps)
    print(ctx, "summary", summ, "restated", wsum)
    assert rows.shape == want.shape == (summ["SEGMENTS"], _abi.VOF_IFACE_N) and rows.dtype == np.float64, ctx
    assert summ["SEGMENTS"] == wsum["SEGMENTS"] and summ["DEGENERATE"] == wsum["DEGENERATE"] and summ["ISTEP"] == e.istep, ctx
    if nan:                                     # a NaN has no bits to agree on: the same cells hold one, everything else is equal
        assert np.array_equal(np.isnan(rows), np.isnan(want)) and np.array_equal(rows, want, equal_nan=True), ctx
        assert math.isnan(summ["LENGTH"]) == math.isnan(wsum["LENGTH"]), ctx
    else:
        bad = np.argwhere(bits(rows) != bits(want))
        assert len(bad) == 0, "%s: %d values differ, first at %s: %r vs %r" % (ctx, len(bad), bad[0], rows[tuple(bad[0])], want[tuple(bad[0])])
        assert bits(summ["LENGTH"]) == bits(wsum["LENGTH"]), "%s LENGTH %r vs %r" % (ctx, summ["LENGTH"], wsum["LENGTH"])
    keys = rows[:, 0] * (e.ny + 2) + rows[:, 1]
    assert np.all(np.diff(keys) > 0), ctx       # strictly ascending (i, j)
    return rows, summ


# ---------------------------------------------------------------------------- equal to the restatement
@pytest.mark.parametrize("ic", [1, 2, 3])
def test_200_f32_after_0_1_and_50_steps(hip_api, ic):
    e = engine(hip_api, 200, 200, "f32", "f32", ic=ic)
    for upto in (0, 1, 50):
        e.step(upto - e.istep)
        rows, summ = hold_to_restatement(e, "200x200 f32 ic %d step %d" % (ic, upto))
        if ic == 1 and upto <= 1:
            # the dam of 2dvof.py:140-147 is a step function, F = 0 or 1, and one step (Courant number 1.6e-7) moves no cell
            # past eps: no mixed cell, no segment -- the empty list is the value
            assert summ["SEGMENTS"] == 0 and summ["LENGTH"] == 0.0 and len(rows) == 0
        else:
            assert summ["SEGMENTS"] > 0 and summ["LENGTH"] > 0


@pytest.mark.parametrize("nx,ny,ic,kw", [(33, 17, 2, {}), (96, 130, 3, {"Lx": 0.1, "Ly": 0.13}), (130, 260, 1, {}), (130, 260, 3, {})])
def test_small_rectangular_and_three_tiles_f64(hip_api, nx, ny, ic, kw):
    """33 x 17: narrower than a wave tile, odd, idle lanes.  96 x 130: rectangular cells, two tiles.  130 x 260: three column
    tiles; the upright face of the dam (-ic 1, j = 1 .. 130) crosses the boundary j = 128 | 129 within single rows i, the drop over the
    pool (-ic 3) has segments in two tiles."""
    e = engine(hip_api, nx, ny, "f64", "f32", ic=ic, **kw)
    if kw:
        assert e.get_param("dx") != e.get_param("dy")
    for upto in (0, 1, 20):
        e.step(upto - e.istep)
        rows, _ = hold_to_restatement(e, "%dx%d f64 ic %d step %d" % (nx, ny, ic, upto))
    if ny == 260:
        tiles = set(((rows[:, 1] - 1) // inp.TILE).astype(int))
        print("tiles holding segments", tiles)
        assert len(tiles) >= 2
        if ic == 1:
            assert any(len(set(((rows[rows[:, 0] == i, 1] - 1) // inp.TILE).astype(int))) >= 2 for i in set(rows[:, 0]))


def test_more_partials_than_scan_threads_f64(hip_api):
    """3277 x 513, the drop over the pool at step 0: five column tiles (the last one a single column) and 4-row chunks, the
    fewest rows for which the count pass has more blocks than k_cell_rows_scan has threads -- 820 chunks x 5 tiles = 4100 waves =
    1025 blocks, one row less gives 1024 -- so thread 0 folds two partials.  Everything with ==."""
    nx, ny = 3277, 513
    R = inp.chunk_rows(nx, ny)
    assert R == 4 and rnp.blocks(nx, ny, R) == 1025 > inp.SCAN_THREADS == 1024 == rnp.blocks(nx - 1, ny, inp.chunk_rows(nx - 1, ny))
    e = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    rows, summ = hold_to_restatement(e, "%dx%d f64 ic 3 step 0" % (nx, ny))
    assert summ["SEGMENTS"] > 0 and summ["LENGTH"] > 0


def test_behind_a_k_tm_batch(hip_api):
    nx, ny, dtype, ic = TM_GRID
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    e.step(40)
    assert e.get_counter("tm_steps") >= 2
    hold_to_restatement(e, "%dx%d %s ic %d behind vof_step(40)" % (nx, ny, dtype, ic))     # first: the handle is ahead, its ghost cells virtual


def test_256_dam_break_behind_forced_k_tm_batches(hip_api):
    e = engine(hip_api, 256, 256, "f64", "f32", ic=1)
    e.set_param("fuse_tm", 1)
    e.step(40)
    print("tm_steps", e.get_counter("tm_steps"))
    hold_to_restatement(e, "256x256 f64 ic 1, fuse_tm = 1, behind vof_step(40)")


# ---------------------------------------------------------------------------- order and capacity
def test_capacity_sizing_call_and_identical_bytes(hip_api):
    e = engine(hip_api, 200, 200, "f64", "f32", ic=3)
    e.step(10)
    rows, summ = hold_to_restatement(e, "200x200 f64 ic 3 step 10")
    n = summ["SEGMENTS"]
    assert n > 8
    s0 = (C.c_double * _abi.VOF_IFACE_SUM_N)()
    assert hip_api.interface(e.handle, EPS, None, 0, s0) == 0                     # sizing call: the same summary
    assert interface.summary_of(list(s0)) == summ
    buf = np.full((n, _abi.VOF_IFACE_N), -777.25)
    s1 = (C.c_double * _abi.VOF_IFACE_SUM_N)()
    assert hip_api.interface(e.handle, EPS, buf.ctypes.data_as(PTR), n - 3, s1) == 0
    assert list(s1) == list(s0)                                                   # ... describes all segments
    assert np.array_equal(bits(buf[:n - 3]), bits(rows[:n - 3])) and np.all(buf[n - 3:] == -777.25)
    big = np.full((n + 5, _abi.VOF_IFACE_N), -777.25)
    assert hip_api.interface(e.handle, EPS, big.ctypes.data_as(PTR), n + 5, s1) == 0
    assert np.array_equal(bits(big[:n]), bits(rows)) and np.all(big[n:] == -777.25)
    again, summ2 = e.interface()
    assert again.tobytes() == rows.tobytes() and summ2 == summ
    wide, wsumm = hold_to_restatement(e, "eps = 0.05", eps=0.05)                  # the caller's eps decides what is mixed
    assert wsumm["SEGMENTS"] < n


# ---------------------------------------------------------------------------- reads only
@pytest.mark.parametrize("mg", [0, 2])
def test_reads_only(hip_api, mg):
    a, b = (engine(hip_api, 128, 128, "f64", "f32", ic=1) for _ in range(2))
    step = (lambda e, n: e.step_mg(n, mg, "rel")) if mg else (lambda e, n: e.step(n))
    step(a, 7); step(b, 7)
    before = {n: a.get(n) for n in FIELDS}
    warn = a.get_counter("courant_violations")
    a.interface()
    assert a.istep == 7 and a.get_counter("courant_violations") == warn
    assert all(np.array_equal(a.get(n), before[n]) for n in FIELDS)
    step(a, 10); step(b, 10)
    a.interface()
    step(a, 10); step(b, 10)
    assert_same_state(a, b, "128x128 f64: interface between steps (mg cycles %d)" % mg)


def test_reads_only_on_the_k_tm_grid(hip_api):
    nx, ny, dtype, ic = TM_GRID
    a, b = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(2))
    for _ in range(2):
        a.step(20); b.step(20)
        a.interface()
    assert a.get_counter("tm_steps") >= 2
    assert_same_state(a, b, "k_tm grid: interface between vof_step(20) calls")


# ---------------------------------------------------------------------------- strips
@pytest.mark.parametrize("nstrips", [2, 3])
def test_strips_combine_to_the_domain(hip_api, nstrips):
    nx, ny, W = 120, 70, halo_rows(10)
    full = engine(hip_api, nx, ny, "f64", "f32", ic=3)
    bounds = [round(k * nx / nstrips) for k in range(nstrips + 1)]
    strips = [engine(hip_api, nx, ny, "f64", "f32", ic=3, rows=(max(0, bounds[k] + 1 - W), min(nx + 1, bounds[k + 1] + W)),
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
            parts = [hold_to_restatement(s, "strip %d..%d step %d" % (s.own_lo, s.own_hi, step)) for s in strips]   # LENGTH per strip
            if step == 12:                       # (-ic 3: the pool's surface has started to move in every strip)
                assert all(p[1]["SEGMENTS"] > 0 for p in parts)
            rows, summ = interface.combine(parts)
            one, osum = hold_to_restatement(full, "the domain, step %d" % step)
            assert np.array_equal(bits(rows), bits(one))
            assert summ["SEGMENTS"] == osum["SEGMENTS"] and summ["DEGENERATE"] == osum["DEGENERATE"] and summ["ISTEP"] == step
            print("LENGTH of the strips", summ["LENGTH"], "of the domain", osum["LENGTH"])
            assert abs(summ["LENGTH"] - osum["LENGTH"]) <= 1e-12 * osum["LENGTH"]


# ---------------------------------------------------------------------------- edge cases
def test_all_gas_all_liquid_and_a_cell_without_orientation(hip_api):
    e = engine(hip_api, 40, 30, "f64", "f32", ic=1)
    for fill in (0.0, 1.0):
        e.set("F", np.full((42, 32), fill))
        rows, summ = hold_to_restatement(e, "F = %g everywhere" % fill)
        assert len(rows) == 0 and summ["SEGMENTS"] == 0 and summ["DEGENERATE"] == 0 and summ["LENGTH"] == 0.0
    F = np.zeros((42, 32))
    F[20, 11] = 0.5                              # in all gas the four corner gradients of :287-294 cancel exactly (tests/test_interface.py)
    e.set("F", F)
    _, wsum = restated(e)
    assert wsum == {"SEGMENTS": 0, "DEGENERATE": 1, "LENGTH": 0.0}
    rows, summ = hold_to_restatement(e, "one mixed cell in all gas")
    assert len(rows) == 0 and summ["DEGENERATE"] == 1 and summ["LENGTH"] == 0.0


def test_a_nan_is_not_a_mixed_cell(hip_api):
    e = engine(hip_api, 96, 64, "f64", "f32", ic=1)
    e.step(5)
    clean, _ = e.interface()
    i, j = int(clean[len(clean) // 2, 0]), int(clean[len(clean) // 2, 1])
    F = e.get("F")
    F[i, j] = np.nan
    e.set("F", F)
    rows, summ = hold_to_restatement(e, "a NaN in F[%d, %d]" % (i, j), nan=True)
    assert summ["SEGMENTS"] == len(clean) - 1 and not ((rows[:, 0] == i) & (rows[:, 1] == j)).any()
    assert np.isnan(rows[:, 2:]).any() and math.isnan(summ["LENGTH"])


def test_refusals_leave_the_handle_alone(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.step(2)
    before = {n: e.get(n) for n in FIELDS}
    buf = np.full((16, _abi.VOF_IFACE_N), -1.5)
    s = (C.c_double * _abi.VOF_IFACE_SUM_N)(*([-1.5] * _abi.VOF_IFACE_SUM_N))
    for eps in (math.nan, -1e-9, 0.5, 0.75, math.inf):
        assert hip_api.interface(e.handle, eps, buf.ctypes.data_as(PTR), 16, s) == _abi.VOF_EINVAL, eps
    assert hip_api.interface(e.handle, EPS, buf.ctypes.data_as(PTR), 16, None) == _abi.VOF_EINVAL
    assert hip_api.interface(e.handle, EPS, None, 16, s) == _abi.VOF_EINVAL
    assert hip_api.interface(e.handle, EPS, buf.ctypes.data_as(PTR), -1, s) == _abi.VOF_EINVAL
    assert hip_api.interface(None, EPS, None, 0, s) == _abi.VOF_EINVAL
    assert np.all(buf == -1.5) and list(s) == [-1.5] * _abi.VOF_IFACE_SUM_N
    assert e.istep == 2 and all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    twin = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    twin.step(4); e.step(2)
    assert_same_state(e, twin, "after the refusals")


# ---------------------------------------------------------------------------- the command line
@pytest.mark.parametrize("more", [[], ["--pressure-solver", "mg", "--mg-cycles", "2"], ["--verbs"]])
def test_cli_writes_the_rows_and_the_csv(hip_api, tmp_path, monkeypatch, more):
    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    argv = ["-ic", "1", "--nx", "64", "--ny", "64", "--dtype", "f64", "--interface-every", "5", "--steps", "12"] + more
    assert cli.run(cli.parse_args(argv), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    data = os.path.join(str(tmp_path), "data")
    assert sorted(f for f in os.listdir(data) if f.startswith("interface_")) == ["interface_000005.npy", "interface_000010.npy"]
    text = open(os.path.join(data, "interface.csv")).read().strip().split("\n")
    assert text[0] == "istep,segments,degenerate,length" and [t.split(",")[0] for t in text[1:]] == ["5", "10"]
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    K = 2 if "--mg-cycles" in more else 0
    if K:
        e.set_param("mg_coarse_block", 1)        # (--mg-coarse block, the default of the command line)
    for line in text[1:]:
        e.step_mg(5, K, "abs") if K else e.step(5)
        rows, summ = e.interface()
        k, seg, deg, length = line.split(",")
        assert (int(k), int(seg), int(deg)) == (e.istep, summ["SEGMENTS"], summ["DEGENERATE"]) and float(length) == summ["LENGTH"]
        assert np.load(os.path.join(data, "interface_%06d.npy" % e.istep)).tobytes() == rows.tobytes()
