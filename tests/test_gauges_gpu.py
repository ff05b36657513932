"""vof_gauges_set / _get and vof_step_gauges on the GPU (include/vof2d.h).

A gauge's row is held bit for bit (a NaN equals a NaN in the same place) to the restatement of tests/_depths_np.py fed the
arrays vof_get_field returns: U, V, F, P by the tracers' sample, DEPTH and TOP from the ordered depth_i and the top of the
row above X.  vof_step_gauges is held to its definition -- the loop "vof_step(every); vof_gauges_get" on a twin handle --
byte for byte, and its final state to a plain vof_step(nsteps).
"""
import ctypes as C

import numpy as np
import pytest

import _depths_np as dnp
import _tracers_np as tnp
from test_diag_gpu import TM_GRID
from test_step_mg_gpu import FIELDS, assert_same_state
from util import engine
from vof2d import _abi, gauges
from vof2d.engine import VofError

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)
UNTOUCHED = -777.25


def positions(e, n=96, seed=0):
    """n gauges: the four corners, points on each wall, cell centres, faces (in x, in y, both), the two sides of the
    boundary between the column tiles (j = 128 | 129) where the grid has one, the rest anywhere in the closed domain."""
    rng = np.random.default_rng(seed)
    nx, ny = e.nx, e.ny
    Lx, Ly, dx, dy = (e.get_param(k) for k in ("Lx", "Ly", "dx", "dy"))
    p = [(0.0, 0.0), (Lx, 0.0), (0.0, Ly), (Lx, Ly)]
    for _ in range(3):
        p += [(0.0, rng.uniform(0, Ly)), (Lx, rng.uniform(0, Ly)), (rng.uniform(0, Lx), 0.0), (rng.uniform(0, Lx), Ly)]
    for _ in range(8):
        i, j = int(rng.integers(1, nx + 1)), int(rng.integers(1, ny + 1))
        p += [(min((i - 0.5) * dx, Lx), min((j - 0.5) * dy, Ly)), (min(i * dx, Lx), rng.uniform(0, Ly)), (rng.uniform(0, Lx), min(j * dy, Ly)),
              (min(i * dx, Lx), min(j * dy, Ly))]
    if ny > 128:
        x = rng.uniform(0, Lx)
        p += [(x, 127.5 * dy), (x, 128 * dy), (x, min(128.5 * dy, Ly)), (x, np.nextafter(128 * dy, 0))]
    rest = max(n - len(p), 0)
    p = np.array((p + list(zip(rng.uniform(0, Lx, rest), rng.uniform(0, Ly, rest))))[:n], dtype=np.float64)
    assert p.shape == (n, 2) and (p >= 0).all() and (p[:, 0] <= Lx).all() and (p[:, 1] <= Ly).all()
    return p


def restated_rows(e, xy):
    Fa = e.get("F")
    res = dnp.restate(Fa)
    di, _, _ = dnp.ordered(res["terms"], dnp.depths_chunk_rows(e.nx, e.ny))
    return dnp.gauge_rows(Fa, e.get("u"), e.get("v"), e.get("p"), xy, tnp.Grid.of(e), di, res["top"], e.get_param("dy"))


def hold(e, xy, records, ctx):
    rows, summ = e.gauges_get()
    want = restated_rows(e, xy)
    print(ctx, "rows", rows.shape, "summary", summ, "first", rows[:1], "restated", want[:1])
    assert rows.shape == (len(xy), _abi.VOF_GAUGE_N) and tnp.same_bits(rows, want), ctx
    assert summ == {"COUNT": len(xy), "ISTEP": e.istep, "RECORDS": records}, ctx
    di, _, top, _ = e.depths()                  # DEPTH and TOP are those of vof_depths on the same state
    ig = np.clip(np.floor(xy[:, 0] * e.get_param("dxi")).astype(int) + 1, 1, e.nx)
    assert np.array_equal(rows[:, gauges.DEPTH], di[ig - 1] * e.get_param("dy")) and np.array_equal(rows[:, gauges.TOP], top[ig - 1].astype(np.float64)), ctx
    return rows


# ---------------------------------------------------------------------------- bit for bit with the restatement
@pytest.mark.parametrize("nx,ny,dtype,ic,kw", [(33, 17, "f64", 2, {}), (96, 130, "f64", 3, {"Lx": 0.1, "Ly": 0.13}), (200, 200, "f32", 1, {})])
def test_rows_equal_the_restatement(hip_api, nx, ny, dtype, ic, kw):
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic, **kw)
    xy = positions(e)
    e.gauges_set(xy)
    for upto in (0, 1, 20):
        e.step(upto - e.istep)
        rows = hold(e, xy, 0, "%dx%d %s ic %d step %d" % (nx, ny, dtype, ic, upto))
    assert np.array_equal(rows[:, :2], xy) and np.abs(rows[:, gauges.P]).max() > 0 and rows[:, gauges.DEPTH].max() > 0


# ---------------------------------------------------------------------------- vof_step_gauges held to its definition
def twin_loop(b, nsteps, every, K=0):
    recs = []
    for _ in range(nsteps // every):
        b.step_mg(every, K, "rel") if K else b.step(every)
        recs.append(b.gauges_get()[0])
    if nsteps % every:
        b.step_mg(nsteps % every, K, "rel") if K else b.step(nsteps % every)
    return np.array(recs)


@pytest.mark.parametrize("nx,ny,dtype,ic,nsteps,every,K", [(33, 17, "f64", 2, 11, 1, 0), (33, 17, "f64", 2, 11, 3, 0), (200, 200, "f32", 1, 70, 32, 0),
                                                           (200, 200, "f32", 3, 10, 3, 0), TM_GRID + (68, 32, 0), (64, 64, "f64", 1, 11, 3, 2)])
def test_step_gauges_equals_the_loop_on_a_twin(hip_api, nx, ny, dtype, ic, nsteps, every, K):
    a, b, c = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(3))
    xy = positions(a, 40, seed=1)
    a.gauges_set(xy); b.gauges_set(xy)
    ctx = "%dx%d %s ic %d: step_gauges(%d, %d, K = %d)" % (nx, ny, dtype, ic, nsteps, every, K)
    recs = a.step_gauges(nsteps, every, K, "rel")
    want = twin_loop(b, nsteps, every, K)
    print(ctx, recs.shape, "last record, first gauge", recs[-1, 0])
    assert recs.shape == (nsteps // every, 40, _abi.VOF_GAUGE_N) and (every == 1 or nsteps % every) and recs.tobytes() == want.tobytes(), ctx
    c.step_mg(nsteps, K, "rel") if K else c.step(nsteps)
    assert_same_state(a, b, ctx)
    assert_same_state(a, c, ctx + " against one call of nsteps")
    if (nx, ny, dtype, ic) == TM_GRID:
        assert a.get_counter("tm_steps") >= 2
    assert a.gauges_get(rows=False)[1] == {"COUNT": 40, "ISTEP": nsteps, "RECORDS": nsteps // every}
    hold(a, xy, nsteps // every, ctx + ", the state it left")
    # ... and once more from the state the call left; a vof_step behind the calls gives the bits of the handle without gauges
    recs = a.step_gauges(2 * every, every, K, "rel")
    want = twin_loop(b, 2 * every, every, K)
    assert recs.tobytes() == want.tobytes() and a.gauges_get(rows=False)[1]["RECORDS"] == nsteps // every + 2, ctx + " (second call)"
    c.step_mg(2 * every, K, "rel") if K else c.step(2 * every)
    a.step(5); c.step(5)
    assert_same_state(a, c, ctx + " and a vof_step behind the calls")


def test_step_gauges_without_graphs_and_without_records(hip_api):
    a = engine(hip_api, 48, 80, "f64", "f32", ic=2, flags=_abi.VOF_FLAG_NO_GRAPH)
    b = engine(hip_api, 48, 80, "f64", "f32", ic=2)
    xy = positions(a, 17, seed=2)
    a.gauges_set(xy); b.gauges_set(xy)
    assert a.step_gauges(11, 3).tobytes() == twin_loop(b, 11, 3).tobytes()
    assert_same_state(a, b, "step_gauges(11, 3) without graphs")
    assert a.step_gauges(0, 5).shape == (0, 0, _abi.VOF_GAUGE_N) and a.istep == 11
    assert a.step_gauges(3, 5).shape == (0, 0, _abi.VOF_GAUGE_N) and a.istep == 14           # a remainder only: stepped, no record
    b.step(3)
    assert_same_state(a, b, "step_gauges(3, 5)")
    assert a.gauges_get(rows=False)[1]["RECORDS"] == 3


# ---------------------------------------------------------------------------- the set, the buffers, equal bytes
def test_the_set_grows_and_shrinks_and_short_buffers_keep_their_tail(hip_api):
    e = engine(hip_api, 96, 130, "f64", "f32", ic=3)
    e.step(6)
    xy = positions(e, 300, seed=3)
    want = restated_rows(e, xy)
    for n in (300, 0, 1, 63, 64, 65, 257, 300, 63, 257):            # (shrinks, grows, and a grow after a shrink)
        e.gauges_set(xy[:n])
        rows, summ = e.gauges_get()
        assert rows.shape == (n, _abi.VOF_GAUGE_N) and tnp.same_bits(rows, want[:n]) and summ == {"COUNT": n, "ISTEP": 6, "RECORDS": 0}, n
    e.gauges_set(xy[:100])
    full = e.gauges_get()[0]
    s = (C.c_double * _abi.VOF_GAUGE_SUM_N)()
    for cap in (30, 0, 100, 120):
        buf = np.full((cap + 2, _abi.VOF_GAUGE_N), UNTOUCHED)
        assert hip_api.gauges_get(e.handle, buf.ctypes.data_as(DP) if cap else None, cap, s) == 0
        k = min(cap, 100)
        assert buf[:k].tobytes() == full[:k].tobytes() and (buf[k:] == UNTOUCHED).all() and list(s) == [100.0, 6.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0], cap
    # two runs give equal bytes: the same call again, and a second handle given the same steps and set
    twin = engine(hip_api, 96, 130, "f64", "f32", ic=3)
    twin.step(6)
    twin.gauges_set(xy[:100])
    assert e.gauges_get()[0].tobytes() == full.tobytes() == twin.gauges_get()[0].tobytes()
    assert e.step_gauges(6, 2).tobytes() == twin.step_gauges(6, 2).tobytes()
    # set_field and set_init_F leave the set alone; vof_gauges_set zeroes RECORDS
    e.set("p", e.get("p"))
    e.set_init_F(3)
    rows, summ = e.gauges_get()
    assert rows[:, :2].tobytes() == xy[:100].tobytes() and summ["RECORDS"] == 3 and summ["COUNT"] == 100
    e.gauges_set(xy[:5])
    assert e.gauges_get(rows=False)[1] == {"COUNT": 5, "ISTEP": 12, "RECORDS": 0}


# ---------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_and_the_gauges_alone(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.step(2)
    xy = positions(e, 65, seed=7)
    e.gauges_set(xy)
    before = {n: e.get(n) for n in FIELDS}
    rows0, summ0 = e.gauges_get()
    Lx = e.get_param("Lx")
    api, h, EINVAL, REL = hip_api, e.handle, _abi.VOF_EINVAL, _abi.VOF_RESID_REL
    for bad in ([[0.01, np.nan]], [[np.inf, 0.01]], [[-1e-9, 0.01]], [[0.01, np.nextafter(Lx, 1)]], [[0.01, 0.01], [2 * Lx, 0.01]]):
        a = np.array(bad, dtype=np.float64)
        assert api.gauges_set(h, a.ctypes.data_as(DP), len(a)) == EINVAL, bad
    a = np.array([[0.01, 0.01]])
    assert api.gauges_set(h, a.ctypes.data_as(DP), -1) == EINVAL and api.gauges_set(h, a.ctypes.data_as(DP), 2 ** 31) == EINVAL
    assert api.gauges_set(h, None, 1) == EINVAL and api.gauges_set(None, a.ctypes.data_as(DP), 1) == EINVAL
    summ = (C.c_double * _abi.VOF_GAUGE_SUM_N)()
    buf = np.zeros((4, _abi.VOF_GAUGE_N))
    assert api.gauges_get(h, None, 4, summ) == EINVAL and api.gauges_get(h, buf.ctypes.data_as(DP), -1, summ) == EINVAL
    assert api.gauges_get(h, buf.ctypes.data_as(DP), 4, None) == EINVAL
    out = np.zeros((4, 65, _abi.VOF_GAUGE_N))
    op, done = out.ctypes.data_as(DP), C.c_int64(-1)
    #            nsteps every K crit out cap
    for args in ((4, 0, 0, REL, op, 4), (4, -1, 0, REL, op, 4), (-1, 1, 0, REL, op, 4), (4, 1, 0, REL, None, 4), (4, 1, 0, REL, op, 3),
                 (4, 1, -1, REL, op, 4), (4, 1, 2, 7, op, 4)):
        assert api.step_gauges(h, *args, C.byref(done)) == EINVAL, args
    assert done.value == -1 and not out.any()
    rows1, summ1 = e.gauges_get()
    assert rows1.tobytes() == rows0.tobytes() and summ1 == summ0 and e.istep == 2
    assert all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    # a bad criterion does not matter without multigrid steps; a NULL out does not matter with no record due
    assert api.step_gauges(h, 1, 1, 0, 7, op, 4, C.byref(done)) == 0 and done.value == 1 and e.istep == 3
    assert api.step_gauges(h, 1, 2, 0, REL, None, 0, None) == 0 and e.istep == 4
    # an empty set: a record due is refused, none due steps
    e.gauges_set(np.zeros((0, 2)))
    rows, summ = e.gauges_get()
    assert rows.shape == (0, _abi.VOF_GAUGE_N) and summ == {"COUNT": 0, "ISTEP": 4, "RECORDS": 0}
    assert api.step_gauges(h, 4, 2, 0, REL, op, 4, C.byref(done)) == EINVAL and e.istep == 4
    assert api.step_gauges(h, 1, 2, 0, REL, None, 0, C.byref(done)) == 0 and done.value == 0 and e.istep == 5


def test_a_strip_and_a_phased_step_are_refused(hip_api):
    s = engine(hip_api, 128, 128, "f64", "f32", ic=1, rows=(0, 80), own=(1, 60))
    before = {n: s.get(n) for n in FIELDS}
    for call in (lambda: s.gauges_set([[0.01, 0.01]]), lambda: s.gauges_get(), lambda: s.step_gauges(4, 2)):
        with pytest.raises(VofError, match="VOF_ESTATE") as err:
            call()
        assert "whole domain" in str(err.value)
    assert s.istep == 0 and all(np.array_equal(s.get(n), before[n]) for n in FIELDS)
    assert s.depths()[3]["ROWS"] == 60                                  # vof_depths works on it
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.gauges_set([[0.01, 0.01]])
    e.step(1)
    e.step_phase(0)
    for call in (lambda: e.gauges_get(), lambda: e.step_gauges(4, 2), lambda: e.gauges_set([[0.02, 0.02]])):
        with pytest.raises(VofError, match="VOF_ESTATE"):
            call()
    e.step_phase(1); e.step_phase(2)
    assert e.gauges_get()[0][0, :2].tolist() == [0.01, 0.01] and e.istep == 2


# ---------------------------------------------------------------------------- the command line
def test_cli_writes_the_csv_files_and_resumes(hip_api, tmp_path, monkeypatch):
    import os

    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    (tmp_path / "g.txt").write_text("# x y\n0.02 0.01\n0.09 0.03\n")
    base = ["-ic", "1", "--nx", "64", "--ny", "64", "--gauge", "0.01,0.02", "--gauges-file", "g.txt", "--gauges-every", "4", "--depths-every", "10"]
    lines = []
    assert cli.run(cli.parse_args(base + ["--steps", "20", "--save-every", "20"]), api=hip_api, world=1, rank=0,
                   out=lambda *a: lines.append(" ".join(str(x) for x in a))) == 0
    data = os.path.join(str(tmp_path), "data")
    assert any("3 gauges set" in ln for ln in lines)
    text = open(os.path.join(data, "gauges.csv")).read().strip().split("\n")
    assert text[0] == gauges.GAUGES_CSV_HEADER and len(text) == 1 + 5 * 3
    # the same run through the engine
    e = engine(hip_api, 64, 64, "f32", "f32", ic=1)
    xy = np.array([[0.01, 0.02], [0.02, 0.01], [0.09, 0.03]])
    e.gauges_set(xy)
    recs = e.step_gauges(20, 4)
    want = [ln for r, rows in enumerate(recs) for ln in gauges.gauges_csv_lines(4 * (r + 1), rows)]
    assert text[1:] == want
    dtext = open(os.path.join(data, "depths.csv")).read().strip().split("\n")
    assert dtext[0] == gauges.DEPTHS_CSV_HEADER and [t.split(",")[0] for t in dtext[1:]] == ["10", "20"]
    di, _, top, summ = e.depths()
    d = gauges.derive(di, summ, e.get_param("dx"), e.get_param("dy"))
    got = np.load(os.path.join(data, "depths_000020.npy"))
    assert got.shape == (64, 3) and np.array_equal(got[:, 0], d["x"]) and np.array_equal(got[:, 1], d["depth"]) and np.array_equal(got[:, 2], top)
    assert dtext[2] == gauges.depths_csv_line(summ, e.get_param("dx"), e.get_param("dy"))
    # resumed without naming the gauges: the set beside the checkpoint; the files are appended to
    assert os.path.exists(os.path.join(data, "gauges_state.npz"))
    resumed = ["-ic", "1", "--nx", "64", "--ny", "64", "--gauges-every", "4", "--depths-every", "10", "--steps", "28", "--resume", "data/00000020.npz"]
    assert cli.run(cli.parse_args(resumed), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    text = open(os.path.join(data, "gauges.csv")).read().strip().split("\n")
    recs = e.step_gauges(8, 4)
    assert len(text) == 1 + 7 * 3 and text[16:] == [ln for r, rows in enumerate(recs) for ln in gauges.gauges_csv_lines(20 + 4 * (r + 1), rows)]
    # with strips the gauge options are refused and say why
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--gpus", "2"])
    assert cli.parse_args(["-ic", "1", "--depths-every", "10", "--gpus", "2"]).depths_every == 10
