"""vof_tracers_set / _advance / _get and vof_step_tracers on the GPU (include/vof2d.h).

The device is held to the restatement of tests/_tracers_np.py (judged on its own in tests/test_tracers.py), fed the arrays
vof_get_field returns: X, Y, U, V, F, the counts and TIME bit for bit (a NaN equals a NaN in the same place).
vof_step_tracers is held to its definition -- the loop "vof_step(every); vof_tracers_advance(every * dt); vof_tracers_get at
the snapshot points" on a twin handle -- byte for byte, and a handle that carries tracers to a twin that does not.
"""
import ctypes as C
import os

import numpy as np
import pytest

import _tracers_np as tnp
from test_step_mg_gpu import FIELDS, assert_same_state
from test_tm_taper_gpu import pair_form
from util import engine
from vof2d import _abi, tracers
from vof2d.engine import VofError

pytestmark = pytest.mark.gpu

GRIDS = [(33, 17, 3), (48, 80, 2)]
DP = C.POINTER(C.c_double)


def points(e, n=1000, seed=0):
    """n start positions: the four corners, points exactly on each wall, exact cell faces and centres, the last cell in
    each direction, the rest anywhere in the closed domain."""
    rng = np.random.default_rng(seed)
    nx, ny = e.nx, e.ny
    Lx, Ly, dx, dy = (e.get_param(k) for k in ("Lx", "Ly", "dx", "dy"))
    p = [(0.0, 0.0), (Lx, 0.0), (0.0, Ly), (Lx, Ly)]
    for _ in range(8):
        p += [(0.0, rng.uniform(0, Ly)), (Lx, rng.uniform(0, Ly)), (rng.uniform(0, Lx), 0.0), (rng.uniform(0, Lx), Ly)]
    for _ in range(40):
        i, j = int(rng.integers(0, nx + 1)), int(rng.integers(0, ny + 1))
        p += [(min(i * dx, Lx), rng.uniform(0, Ly)), (rng.uniform(0, Lx), min(j * dy, Ly)), (min(i * dx, Lx), min(j * dy, Ly))]
        i, j = int(rng.integers(1, nx + 1)), int(rng.integers(1, ny + 1))
        p += [(min((i - 0.5) * dx, Lx), min((j - 0.5) * dy, Ly))]
    for _ in range(20):
        p += [(rng.uniform((nx - 1) * dx, Lx), rng.uniform(0, Ly)), (rng.uniform(0, Lx), rng.uniform((ny - 1) * dy, Ly)),
              (rng.uniform(0, dx), rng.uniform(0, dy))]
    rest = max(n - len(p), 0)
    p = np.array((p + list(zip(rng.uniform(0, Lx, rest), rng.uniform(0, Ly, rest))))[:n], dtype=np.float64)
    assert p.shape == (n, 2) and (p >= 0).all() and (p[:, 0] <= Lx).all() and (p[:, 1] <= Ly).all()
    return p


def restated_fields(e, record=False):
    return tnp.fields(e.get("F"), e.get("u"), e.get("v"), record)


def hold(e, xy, time, ctx):
    """The device's rows and summary against the restatement at the positions xy (which the device must hold)."""
    g = tnp.Grid.of(e)
    Ff, u, v = restated_fields(e)
    want = tnp.rows(Ff, u, v, xy, g)
    rows, summ = e.tracers()
    wsum = tnp.summary(want, e.istep, time)
    print(ctx, "rows", rows.shape, "summary", summ, "restated", list(wsum[:5]))
    assert tnp.same_bits(rows, want), ctx
    assert [summ[k] for k in tracers.SUMMARY] == list(wsum[:5]), ctx
    return rows


_cases = {}


def advanced_case(hip_api, nx, ny, ic, dtype):
    """A handle after 20 steps with 1000 tracers, moved by five advances of 7 dt and one long one, each held to the
    restatement; computed once per case and left alone: (engine, start positions, positions after the first advance)."""
    key = (nx, ny, ic, dtype)
    if key in _cases:
        return _cases[key]
    e = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    e.step(20)
    ctx = "%dx%d ic %d %s" % (nx, ny, ic, dtype)
    g = tnp.Grid.of(e)
    _, u, v = restated_fields(e)
    xy0 = points(e)
    e.tracers_set(xy0)
    xy = hold(e, xy0, 0.0, ctx + " as set")[:, :2]
    assert np.array_equal(xy, xy0)
    h, t, first = 7 * e.get_param("dt"), 0.0, None
    for k in range(5):
        e.tracers_advance(h)
        t += h
        xy = tnp.advance(u, v, xy, h, g)
        first = xy if first is None else first
        hold(e, xy, t, ctx + " advance %d" % (k + 1))
    # one advance long enough to throw tracers against the walls (the restatement itself must show at least two)
    umax, vmax = float(np.abs(e.get("u")).max()), float(np.abs(e.get("v")).max())   # (Python doubles: an f32 scalar would make t one too)
    assert umax > 0 and vmax > 0
    h = 100.0 * max(g.Lx, g.Ly) / min(umax, vmax)
    events = set()
    e.tracers_advance(h)
    t += h
    xy = tnp.advance(u, v, xy, h, g, events)
    print(ctx, "long advance h = %.3e: clamps at" % h, sorted(events))
    assert len(events) >= 2
    rows = hold(e, xy, t, ctx + " long advance")
    assert not np.isnan(rows[:, :2]).any()
    _cases[key] = (e, xy0, first)
    return _cases[key]


# ---------------------------------------------------------------------------- bit for bit with the restatement
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("nx,ny,ic", GRIDS)
def test_rows_counts_and_time_equal_the_restatement(hip_api, nx, ny, ic, dtype):
    advanced_case(hip_api, nx, ny, ic, dtype)


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_set_sizes_give_the_bits_of_the_first_1000(hip_api, dtype):
    nx, ny, ic = GRIDS[0]
    e, xy0, first = advanced_case(hip_api, nx, ny, ic, dtype)
    g = tnp.Grid.of(e)
    Ff, u, v = restated_fields(e)
    want = tnp.rows(Ff, u, v, first, g)
    h = 7 * e.get_param("dt")
    for n in (1000, 0, 1, 63, 64, 65, 257, 1000, 63, 257):          # (shrinks, grows, and a grow after a shrink)
        e.tracers_set(xy0[:n])
        rows, summ = e.tracers()
        assert np.array_equal(rows[:, :2], xy0[:n]) and summ["COUNT"] == n and summ["TIME"] == 0.0, n
        e.tracers_advance(h)
        rows, summ = e.tracers()
        assert rows.shape == (n, _abi.VOF_TRACER_N) and tnp.same_bits(rows, want[:n]), n
        assert summ["COUNT"] == n and summ["LOST"] == 0 and summ["TIME"] == h and summ["IN_LIQUID"] == int((want[:n, tnp.F] >= 0.5).sum()), n


# ---------------------------------------------------------------------------- rigid rotation on the device
@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_rigid_rotation_on_the_device(hip_api, dtype):
    nx, ny, w, xc, yc, h = 64, 48, 2.0, 0.5, 0.3, 0.05
    e = engine(hip_api, nx, ny, dtype, "f32", Lx=1.0, Ly=0.6)
    dx, dy = e.get_param("dx"), e.get_param("dy")
    for name, a in zip(("F", "u", "v"), tnp.rotation_fields(nx, ny, dx, dy, w, xc, yc)):
        e.set(name, a)
    rng = np.random.default_rng(3)
    r, th = rng.uniform(0.02, 0.2, 48), rng.uniform(0, 2 * np.pi, 48)
    xy = np.stack([xc + r * np.cos(th), yc + r * np.sin(th)], axis=1)
    e.tracers_set(xy)
    g = tnp.Grid.of(e)
    _, u, v = restated_fields(e)
    t = 0.0
    for k in range(1, 201):
        e.tracers_advance(h)
        t += h
        xy = tnp.advance(u, v, xy, h, g)
        if k % 50 == 0:
            rows = hold(e, xy, t, "rigid rotation %s, advance %d" % (dtype, k))
    assert min(xy[:, 0].min(), 1.0 - xy[:, 0].max(), xy[:, 1].min(), 0.6 - xy[:, 1].max()) > 2 * max(dx, dy)   # more than two cells from every wall
    rad = np.hypot(rows[:, 0] - xc, rows[:, 1] - yc)
    print("radius growth", (rad / r).min(), (rad / r).max(), "closed form", (1 + (w * h) ** 4 / 4) ** 100)
    if dtype == "f64":                          # (an f32 field is linear only to its rounding: the bits above are the check there)
        assert np.allclose(rad / r, (1 + (w * h) ** 4 / 4) ** 100, rtol=1e-11, atol=0)


# ---------------------------------------------------------------------------- vof_step_tracers held to its definition
def twin_loop(b, nsteps, every, snap_every, K=0):
    snaps, dt = [], b.get_param("dt")
    for r in range(nsteps // every):
        b.step_mg(every, K, "rel") if K else b.step(every)
        b.tracers_advance(float(every) * dt)
        if snap_every and (r + 1) % snap_every == 0:
            snaps.append(b.tracers()[0])
    if nsteps % every:
        b.step_mg(nsteps % every, K, "rel") if K else b.step(nsteps % every)
    return np.array(snaps)


@pytest.mark.parametrize("dtype,nsteps,K,flags", [("f64", 40, 0, 0), ("f32", 40, 0, 0), ("f64", 40, 2, 0), ("f64", 40, 0, _abi.VOF_FLAG_NO_GRAPH),
                                                   ("f64", 42, 0, 0), ("f32", 42, 2, _abi.VOF_FLAG_NO_GRAPH)])
def test_step_tracers_equals_the_loop_on_a_twin(hip_api, dtype, nsteps, K, flags):
    nx, ny, ic = GRIDS[1]
    a = engine(hip_api, nx, ny, dtype, "f32", ic=ic, flags=flags)
    b = engine(hip_api, nx, ny, dtype, "f32", ic=ic)
    xy = points(a, 257, seed=1)
    a.tracers_set(xy); b.tracers_set(xy)
    ctx = "%dx%d %s: step_tracers(%d, 4, K = %d, flags %d, snap_every 2)" % (nx, ny, dtype, nsteps, K, flags)
    snaps = a.step_tracers(nsteps, 4, K, "rel", snap_every=2)
    want = twin_loop(b, nsteps, 4, 2, K)
    print(ctx, snaps.shape)
    assert snaps.shape == (5, 257, _abi.VOF_TRACER_N) and snaps.tobytes() == want.tobytes(), ctx
    (ra, sa), (rb, sb) = a.tracers(), b.tracers()
    assert ra.tobytes() == rb.tobytes() and sa == sb, ctx
    dt, t = a.get_param("dt"), 0.0
    for _ in range(10):
        t += 4.0 * dt
    assert sa["TIME"] == t and sa["ISTEP"] == nsteps and sa["COUNT"] == 257, ctx      # (nsteps = 42: TIME lags by 2 dt)
    assert np.abs(ra[:, :2] - xy).max() > 0                                           # they have moved
    assert_same_state(a, b, ctx)
    # without snapshots nothing is copied and snaps may be NULL
    done = C.c_int64(-1)
    assert hip_api.step_tracers(a.handle, 8, 4, K, _abi.VOF_RESID_REL, 0, None, 0, C.byref(done)) == 0 and done.value == 0
    twin_loop(b, 8, 4, 0, K)
    assert a.tracers()[0].tobytes() == b.tracers()[0].tobytes()
    assert_same_state(a, b, ctx + " (second call)")


# ---------------------------------------------------------------------------- tracers change nothing else
@pytest.mark.parametrize("dtype", ["f64", "f32"])
@pytest.mark.parametrize("K", [0, 2])
def test_fields_are_those_of_a_handle_without_tracers(hip_api, dtype, K):
    nx, ny, ic = GRIDS[1]
    a, b = (engine(hip_api, nx, ny, dtype, "f32", ic=ic) for _ in range(2))
    a.tracers_set(points(a, 257, seed=2))
    a.step_tracers(30, 4, K, "rel", snap_every=3)
    b.step_mg(30, K, "rel") if K else b.step(30)
    assert_same_state(a, b, "%dx%d %s K = %d: step_tracers(30, 4) against the plain steps" % (nx, ny, dtype, K))
    a.tracers_advance(1e-5); a.tracers()
    a.step(5); b.step(5)
    assert_same_state(a, b, "... and a vof_step behind the verbs")


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_fields_are_those_of_a_handle_without_tracers_in_the_pair_form(hip_api, dtype):
    nx, ny = 160, 240
    a, b = (pair_form(hip_api, nx, ny, dtype, 1) for _ in range(2))
    a.tracers_set(points(a, 257, seed=2))
    snaps = a.step_tracers(40, 10, snap_every=2)
    b.step(40)
    print("tm_steps", a.get_counter("tm_steps"), b.get_counter("tm_steps"), "chained", a.get_counter("tm_chained_batches"), b.get_counter("tm_chained_batches"))
    assert a.get_counter("tm_steps") > 0 and snaps.shape == (2, 257, _abi.VOF_TRACER_N)
    assert_same_state(a, b, "%dx%d %s pair form: step_tracers(40, 10) against vof_step(40)" % (nx, ny, dtype))
    t = 0.0
    for _ in range(4):
        t += 10.0 * a.get_param("dt")
    hold(a, a.tracers()[0][:, :2], t, "behind a k_tm batch")


# ---------------------------------------------------------------------------- a NaN is reported, not hidden
def test_a_nan_in_u_loses_exactly_the_tracers_that_touch_it(hip_api):
    nx, ny, ic = GRIDS[1]
    e = engine(hip_api, nx, ny, "f64", "f32", ic=ic)
    e.step(20)
    ua = e.get("u")
    ua[20, 33] = np.nan                         # an interior face: ordinary data through vof_set_field
    e.set("u", ua)
    g = tnp.Grid.of(e)
    xy = points(e, 1000, seed=4)
    xy[:40] = np.stack([(19 + np.random.default_rng(5).uniform(-1.5, 1.5, 40)) / g.dxi, (32.5 + np.random.default_rng(6).uniform(-1.5, 1.5, 40)) / g.dyi], axis=1)
    e.tracers_set(xy)
    h = 7 * e.get_param("dt")
    e.tracers_advance(h)
    Ff, u, v = restated_fields(e)
    touched = []
    for x, y in xy.tolist():
        u.loads = []
        tnp.advance_one(u, v, x, y, h, g)
        touched.append((20, 33) in u.loads)
    u.loads = None
    want = tnp.advance(u, v, xy, h, g)
    rows = hold(e, want, h, "a NaN in u[20,33]")
    lost = np.isnan(rows[:, 0])
    print("lost", int(lost.sum()), "touching", int(np.sum(touched)))
    assert 0 < lost.sum() < 1000 and list(lost) == touched
    assert e.tracers(rows=False)[1]["LOST"] == int(lost.sum())
    # lost for good: a clean field does not bring them back, the others go on
    ua[20, 33] = 0.0
    e.set("u", ua)
    e.tracers_advance(h)
    _, u, v = restated_fields(e)
    hold(e, tnp.advance(u, v, want, h, g), h + h, "behind the NaN")


# ---------------------------------------------------------------------------- refusals
def test_refusals_leave_the_handle_and_the_tracers_alone(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.step(2)
    xy = points(e, 65, seed=7)
    e.tracers_set(xy)
    e.tracers_advance(1e-5)
    before = {n: e.get(n) for n in FIELDS}
    rows0, summ0 = e.tracers()
    Lx = e.get_param("Lx")
    api, h, EINVAL, REL = hip_api, e.handle, _abi.VOF_EINVAL, _abi.VOF_RESID_REL
    for bad in ([[0.01, np.nan]], [[np.inf, 0.01]], [[-1e-9, 0.01]], [[0.01, np.nextafter(Lx, 1)]], [[0.01, 0.01], [2 * Lx, 0.01]]):
        a = np.array(bad, dtype=np.float64)
        assert api.tracers_set(h, a.ctypes.data_as(DP), len(a)) == EINVAL, bad
    a = np.array([[0.01, 0.01]])
    assert api.tracers_set(h, a.ctypes.data_as(DP), -1) == EINVAL
    assert api.tracers_set(h, a.ctypes.data_as(DP), 2 ** 31) == EINVAL
    assert api.tracers_set(h, None, 1) == EINVAL
    for t in (np.nan, np.inf, -np.inf):
        assert api.tracers_advance(h, t) == EINVAL
    summ = (C.c_double * _abi.VOF_TRACER_SUM_N)()
    buf = np.zeros((4, _abi.VOF_TRACER_N))
    assert api.tracers_get(h, None, 4, summ) == EINVAL and api.tracers_get(h, buf.ctypes.data_as(DP), -1, summ) == EINVAL
    assert api.tracers_get(h, buf.ctypes.data_as(DP), 4, None) == EINVAL
    snaps = np.zeros((4, 65, _abi.VOF_TRACER_N))
    sp, done = snaps.ctypes.data_as(DP), C.c_int64(-1)
    #            nsteps every K crit snap_every snaps cap
    for args in ((8, 0, 0, REL, 1, sp, 4), (8, -1, 0, REL, 1, sp, 4), (-1, 2, 0, REL, 1, sp, 4), (8, 2, 0, REL, -1, sp, 4), (8, 2, 0, REL, 1, sp, 3),
                 (8, 2, 0, REL, 1, None, 4), (8, 2, -1, REL, 1, sp, 4), (8, 2, 2, 7, 1, sp, 4)):
        assert api.step_tracers(h, *args, C.byref(done)) == EINVAL, args
    assert done.value == -1 and not snaps.any()
    rows1, summ1 = e.tracers()
    assert rows1.tobytes() == rows0.tobytes() and summ1 == summ0 and e.istep == 2
    assert all(np.array_equal(e.get(n), before[n]) for n in FIELDS)
    # set_init_F and set_field leave the set alone; n = 0 clears it; an empty set advances nothing
    e.set("p", before["p"])
    assert e.tracers()[0][:, :2].tobytes() == rows0[:, :2].tobytes()
    e.set_init_F(1)
    assert e.tracers()[0][:, :2].tobytes() == rows0[:, :2].tobytes() and e.tracers(rows=False)[1]["TIME"] == 1e-5
    i0 = e.istep
    e.tracers_set(np.zeros((0, 2)))
    e.tracers_advance(1e-5)
    rows, summ = e.tracers()
    assert rows.shape == (0, _abi.VOF_TRACER_N) and summ["COUNT"] == 0 and summ["LOST"] == 0
    assert e.step_tracers(4, 2, snap_every=1).shape == (2, 0, _abi.VOF_TRACER_N) and e.istep == i0 + 4


def test_a_strip_and_a_phased_step_are_refused(hip_api):
    s = engine(hip_api, 128, 128, "f64", "f32", ic=1, rows=(0, 80), own=(1, 60))
    before = {n: s.get(n) for n in FIELDS}
    for call in (lambda: s.tracers_set([[0.01, 0.01]]), lambda: s.tracers_advance(1e-5), lambda: s.tracers(), lambda: s.step_tracers(4, 2)):
        with pytest.raises(VofError, match="VOF_ESTATE") as err:
            call()
        assert "whole domain" in str(err.value)
    assert s.istep == 0 and all(np.array_equal(s.get(n), before[n]) for n in FIELDS)
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    e.tracers_set([[0.01, 0.01]])
    e.step(1)
    e.step_phase(0)
    for call in (lambda: e.tracers_advance(1e-5), lambda: e.tracers(), lambda: e.step_tracers(4, 2), lambda: e.tracers_set([[0.02, 0.02]])):
        with pytest.raises(VofError, match="VOF_ESTATE"):
            call()
    e.step_phase(1); e.step_phase(2)
    assert e.tracers()[0][0, :2].tolist() == [0.01, 0.01]


# ---------------------------------------------------------------------------- the read-out
def test_a_short_buffer_is_filled_and_its_tail_left_alone(hip_api):
    nx, ny, ic = GRIDS[0]
    e, xy0, _ = advanced_case(hip_api, nx, ny, ic, "f64")
    e.tracers_set(xy0[:100])
    full, summ = e.tracers()
    buf = np.full((50, _abi.VOF_TRACER_N), -7.0)
    s = (C.c_double * _abi.VOF_TRACER_SUM_N)()
    assert hip_api.tracers_get(e.handle, buf.ctypes.data_as(DP), 30, s) == 0
    assert buf[:30].tobytes() == full[:30].tobytes() and (buf[30:] == -7.0).all()
    assert tracers.summary_of(list(s)) == summ and summ["COUNT"] == 100              # the summary describes all tracers
    s2 = (C.c_double * _abi.VOF_TRACER_SUM_N)()
    assert hip_api.tracers_get(e.handle, None, 0, s2) == 0 and list(s2) == list(s)
    big = np.full((120, _abi.VOF_TRACER_N), -7.0)
    assert hip_api.tracers_get(e.handle, big.ctypes.data_as(DP), 120, s2) == 0
    assert big[:100].tobytes() == full.tobytes() and (big[100:] == -7.0).all()


def test_seed_keeps_one_phase(hip_api):
    e = engine(hip_api, 64, 64, "f64", "f32", ic=1)
    n_all = len(tracers.seed(e, 400, "all"))
    liquid = tracers.seed(e, 400, "liquid")
    rows, summ = e.tracers()
    assert np.array_equal(rows[:, :2], liquid) and (rows[:, tnp.F] >= 0.5).all() and summ["IN_LIQUID"] == summ["COUNT"] == len(liquid) > 0
    gas = tracers.seed(e, 400, "gas")
    rows, summ = e.tracers()
    assert (rows[:, tnp.F] < 0.5).all() and summ["IN_LIQUID"] == 0 and len(gas) + len(liquid) == n_all == 400


# ---------------------------------------------------------------------------- the command line
def test_cli_writes_the_rows_and_the_csv_and_resumes(hip_api, tmp_path, monkeypatch):
    from vof2d import cli
    monkeypatch.chdir(tmp_path)
    base = ["-ic", "1", "--nx", "64", "--ny", "64", "--tracers", "200", "--tracers-every", "4", "--tracers-save-every", "20"]
    lines = []
    assert cli.run(cli.parse_args(base + ["--steps", "40", "--save-every", "40"]), api=hip_api, world=1, rank=0,
                   out=lambda *a: lines.append(" ".join(str(x) for x in a))) == 0
    data = os.path.join(str(tmp_path), "data")
    text = open(os.path.join(data, "tracers.csv")).read().strip().split("\n")
    assert text[0] == tracers.CSV_HEADER and len(text) == 3 and [t.split(",")[0] for t in text[1:]] == ["20", "40"]
    # the same run through the engine
    e = engine(hip_api, 64, 64, "f32", "f32", ic=1)
    kept = tracers.seed(e, 200, "liquid")
    assert any("%d tracers seeded" % len(kept) in ln for ln in lines)
    for k, istep in enumerate((20, 40)):
        e.step_tracers(20, 4)
        rows, summ = e.tracers()
        got = np.load(os.path.join(data, "tracers_%06d.npy" % istep))
        assert got.shape == (len(kept), _abi.VOF_TRACER_N) and got.tobytes() == rows.tobytes()
        assert text[k + 1] == tracers.csv_line(summ)
    t40 = float(text[2].split(",")[1])
    assert t40 == summ["TIME"] > 0
    # resumed: the positions and TIME continue
    assert os.path.exists(os.path.join(data, "tracers_state.npz"))
    assert cli.run(cli.parse_args(base + ["--steps", "60", "--resume", "data/00000040.npz"]), api=hip_api, world=1, rank=0, out=lambda *a: None) == 0
    text = open(os.path.join(data, "tracers.csv")).read().strip().split("\n")
    assert [t.split(",")[0] for t in text] == ["istep", "20", "40", "60"]
    e.tracers_set(rows[:, :2])
    e.step_tracers(20, 4)
    rows, summ = e.tracers()
    assert np.load(os.path.join(data, "tracers_000060.npy")).tobytes() == rows.tobytes()
    assert float(text[3].split(",")[1]) == t40 + summ["TIME"] and text[3].split(",")[2:] == [str(len(kept)), "0", str(summ["IN_LIQUID"])]
