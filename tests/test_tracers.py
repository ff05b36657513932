"""The tracer definitions of include/vof2d.h on the CPU: the NumPy restatement tests/_tracers_np.py is judged here on its own
-- against the closed form of the midpoint rule in a rigid rotation, on hand-made wall, NaN and inf cases, and for loads
that stay inside the stored arrays -- before tests/test_tracers_gpu.py holds the device to it bit for bit.  Also the
lattice of start positions (vof2d/tracers.py).  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import _tracers_np as tnp
from vof2d import tracers


# ---------------------------------------------------------------------------- the midpoint rule in a rigid rotation
def test_rigid_rotation_follows_the_closed_form():
    """u = -w (y - yc), v = w (x - xc) on 64 x 48, Lx, Ly = 1, 0.6, w = 2, centre (0.5, 0.3), start at radius 0.2, h = 0.05,
    200 advances.  Bilinear sampling is exact for a linear field, and one midpoint step multiplies z = (x - xc) + i (y - yc)
    by 1 + i w h - (w h)^2 / 2: the radius grows by sqrt(1 + (w h)^4 / 4), the angle by atan2(w h, 1 - (w h)^2 / 2).  Bound:
    1e-12 absolute in x and y at every advance (a few ulp of rounding per advance, 200 advances: three orders of margin)."""
    nx, ny, Lx, Ly, w, xc, yc, h = 64, 48, 1.0, 0.6, 2.0, 0.5, 0.3, 0.05
    dx, dy = Lx / nx, Ly / ny
    g = tnp.Grid(nx, ny, 1 / dx, 1 / dy, Lx, Ly)
    _, u, v = tnp.fields(*tnp.rotation_fields(nx, ny, dx, dy, w, xc, yc))
    grow = math.sqrt(1 + (w * h) ** 4 / 4)
    turn = math.atan2(w * h, 1 - (w * h) ** 2 / 2)
    x, y = xc + 0.2, yc
    worst, nearest = 0.0, math.inf
    for k in range(1, 201):
        x, y = tnp.advance_one(u, v, x, y, h, g)
        r, th = 0.2 * grow ** k, k * turn
        worst = max(worst, abs(x - (xc + r * math.cos(th))), abs(y - (yc + r * math.sin(th))))
        nearest = min(nearest, x, Lx - x, y, Ly - y)
        assert worst <= 1e-12, (k, worst)
    print("worst error against the closed form %.3e, nearest to a wall %.4f" % (worst, nearest))
    assert nearest > 2 * max(dx, dy)          # no clamp took part


# ---------------------------------------------------------------------------- walls, NaN, inf
def uniform(nx, ny, uval, vval):
    shape = (nx + 2, ny + 2)
    return tnp.fields(np.zeros(shape), np.full(shape, uval), np.full(shape, vval))


@pytest.mark.parametrize("uval,vval,want,wall", [(5.0, 0.0, (1.0, 0.25), "xL"), (-5.0, 0.0, (0.0, 0.25), "x0"),
                                                  (0.0, 5.0, (0.5, 0.5), "yL"), (0.0, -5.0, (0.5, 0.0), "y0")])
def test_an_overshoot_is_clamped_at_each_wall(uval, vval, want, wall):
    g = tnp.Grid(8, 4, 8.0, 8.0, 1.0, 0.5)
    _, u, v = uniform(8, 4, uval, vval)
    events = set()
    got = tnp.advance_one(u, v, 0.5, 0.25, 1.0, g, events)   # both the midpoint and the end point overshoot
    print(got, events)
    assert got == want and events == {wall}
    # a tracer on the wall stays on it and is not lost
    assert tnp.advance_one(u, v, want[0], want[1], 1.0, g) == want


def test_clamp_keeps_a_nan():
    assert math.isnan(tnp.clamp(math.nan, 1.0)) and tnp.clamp(-1e-300, 1.0) == 0.0 and tnp.clamp(2.0, 1.0) == 1.0 and tnp.clamp(0.3, 1.0) == 0.3


@pytest.mark.parametrize("bad", [math.nan, math.inf, -math.inf])
def test_a_nan_or_an_inf_in_a_stencil_loses_the_tracer(bad):
    nx, ny = 8, 4
    g = tnp.Grid(nx, ny, 8.0, 8.0, 1.0, 0.5)
    Fa, ua, va = (np.zeros((nx + 2, ny + 2)) for _ in range(3))
    ua[4, 2] = bad                              # u[4,2] sits at (0.375, 0.1875)
    Ff, u, v = tnp.fields(Fa, ua, va)
    near, far = (0.40, 0.20), (0.80, 0.40)
    assert all(math.isnan(c) for c in tnp.advance_one(u, v, *near, 0.01, g))
    assert tnp.advance_one(u, v, *far, 0.01, g) == far
    # an inf times a zero weight is a NaN too: exactly on the face line of the neighbour the stencil still holds the cell
    assert all(math.isnan(c) for c in tnp.advance_one(u, v, 0.25, 0.20, 0.01, g))
    # lost for good, and its row reads NaN
    assert all(math.isnan(c) for c in tnp.advance_one(u, v, math.nan, math.nan, 0.01, g))
    r = tnp.rows(Ff, u, v, np.array([[math.nan, math.nan], far]), g)
    assert np.isnan(r[0, :5]).all() and (r[0, 5:] == 0).all() and not np.isnan(r[1]).any()
    s = tnp.summary(r, 7, 0.5)
    assert list(s) == [2, 1, 0, 7, 0.5, 0, 0, 0]


# ---------------------------------------------------------------------------- every load inside the stored arrays
@pytest.mark.parametrize("nx,ny,Lx,Ly", [(3, 3, 0.1, 0.1), (5, 4, 1.0, 0.6), (33, 17, 0.1, 0.1), (7, 200, 0.3, 0.7)])
def test_samples_on_walls_corners_faces_and_centres_stay_inside(nx, ny, Lx, Ly):
    dx, dy = Lx / nx, Ly / ny
    rng = np.random.default_rng(nx * 1000 + ny)
    Fa, ua, va = (rng.standard_normal((nx + 2, ny + 2)) for _ in range(3))
    # dxi, dyi rounded either way: x * dxi may come out just above nx at the wall
    for dxi, dyi in ((1 / dx, 1 / dy), (np.nextafter(1 / dx, math.inf), np.nextafter(1 / dy, math.inf)), (np.nextafter(1 / dx, 0), np.nextafter(1 / dy, 0))):
        g = tnp.Grid(nx, ny, dxi, dyi, Lx, Ly)
        Ff, u, v = tnp.fields(Fa, ua, va, record=True)   # (Field.at raises on an index outside the array)
        xs = sorted({0.0, Lx} | {i * dx for i in range(nx + 1)} | {(i + 0.5) * dx for i in range(nx)} | {np.nextafter(Lx, 0), np.nextafter(0.0, 1)})
        ys = sorted({0.0, Ly} | {j * dy for j in range(ny + 1)} | {(j + 0.5) * dy for j in range(ny)} | {np.nextafter(Ly, 0), np.nextafter(0.0, 1)})
        xy = np.array([(min(x, Lx), min(y, Ly)) for x in xs for y in ys])
        r = tnp.rows(Ff, u, v, xy, g)
        assert np.isfinite(r).all()
        for f in (Ff, u, v):
            ii, jj = np.array(f.loads).T
            assert ii.min() >= 0 and ii.max() <= nx + 1 and jj.min() >= 0 and jj.max() <= ny + 1
        # u never reads row 0, v never column 0: nothing is stored for a face there that the flow uses
        assert min(i for i, _ in u.loads) >= 1 and min(j for _, j in v.loads) >= 1


def test_a_sample_at_a_field_point_is_the_field_value():
    nx, ny, Lx, Ly = 8, 4, 1.0, 0.5            # dx = dy = 1 / 8: every product below is exact
    g = tnp.Grid(nx, ny, 8.0, 8.0, Lx, Ly)
    rng = np.random.default_rng(5)
    Fa, ua, va = (rng.standard_normal((nx + 2, ny + 2)) for _ in range(3))
    Ff, u, v = tnp.fields(Fa, ua, va)
    for i in range(1, nx + 1):
        for j in range(1, ny + 1):
            assert tnp.sample(u, (i - 1) / 8, (j - 0.5) / 8, g) == ua[i, j]
            assert tnp.sample(v, (i - 0.5) / 8, (j - 1) / 8, g) == va[i, j]
            assert tnp.sample(Ff, (i - 0.5) / 8, (j - 0.5) / 8, g) == Fa[i, j]
    assert tnp.sample(u, Lx, 0.0, g) == 0.5 * (ua[nx + 1, 0] + ua[nx + 1, 1])     # the wall face, half way into the ghost column
    assert tnp.sample(Ff, 0.0, 0.0, g) == 0.25 * (Fa[0, 0] + Fa[1, 0] + Fa[0, 1] + Fa[1, 1])


# ---------------------------------------------------------------------------- the lattice
@pytest.mark.parametrize("nx,ny,Lx,Ly", [(64, 64, 0.1, 0.1), (64, 48, 1.0, 0.6), (200, 50, 0.4, 0.1), (30, 300, 0.05, 0.5)])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 50, 200, 1000])
def test_lattice_is_inside_and_of_about_the_size_asked_for(nx, ny, Lx, Ly, n):
    p = tracers.lattice(nx, ny, Lx, Ly, n)
    print(nx, ny, n, len(p))
    assert p.shape == (len(p), 2) and p.dtype == np.float64
    assert (p[:, 0] > 0).all() and (p[:, 0] < Lx).all() and (p[:, 1] > 0).all() and (p[:, 1] < Ly).all()
    assert n / 2 <= len(p) <= 3 * n / 2        # the factor its docstring states (no cap applies on these grids)
    assert len({tuple(q) for q in p.tolist()}) == len(p)


def test_lattice_of_nothing_and_the_cap_of_one_point_per_cell():
    assert tracers.lattice(8, 8, 1.0, 1.0, 0).shape == (0, 2)
    assert len(tracers.lattice(4, 4, 1.0, 1.0, 1000)) == 16


def test_summary_of_names_the_slots():
    s = tracers.summary_of([5.0, 1.0, 3.0, 40.0, 1.6e-4, 0.0, 0.0, 0.0])
    assert s == {"COUNT": 5, "LOST": 1, "IN_LIQUID": 3, "ISTEP": 40, "TIME": 1.6e-4}
    assert tracers.csv_line(s) == "40,0.00016,5,1,3"
    with pytest.raises(ValueError):
        tracers.summary_of([0.0] * 4)


# ---------------------------------------------------------------------------- the command line's combinations
@pytest.mark.parametrize("argv", [["--tracers", "100", "--gpus", "2"], ["--tracers-save-every", "10"], ["--tracers", "-1"],
                                  ["--tracers", "100", "--tracers-every", "0"], ["--tracers", "100", "--tracers-save-every", "0"],
                                  ["--tracers", "100", "--tracers-phase", "foam"]])
def test_cli_refuses_what_tracers_cannot_do(argv, capsys):
    from vof2d import cli
    with pytest.raises(SystemExit):
        cli.parse_args(argv)
    assert "--tracers" in capsys.readouterr().err


def test_cli_defaults():
    from vof2d import cli
    a = cli.parse_args(["--tracers", "100"])
    assert (a.tracers, a.tracers_phase, a.tracers_every, a.tracers_save_every) == (100, "liquid", 1, None)
    assert cli.parse_args([]).tracers == 0


def test_cli_advances_every_k_steps_wherever_the_loop_stops(oracle_api):
    """The chunking of the command line's driver on the CPU oracle, with the two tracer calls of the engine recorded
    instead of made (the oracle has no tracers): an advance by K dt behind every K-th step counted from the seeding."""
    from vof2d import cli
    args = cli.parse_args(["--nx", "16", "--ny", "16", "--dtype", "f64", "--tracers", "10", "--tracers-every", "4"])
    drv = cli._Single(args, oracle_api)
    drv.init(1)
    eng, calls = drv.eng, []
    dt = eng.get_param("dt")

    def step_tracers(n, every):
        assert n % every == 0 and eng.istep % every == 0
        calls.append(("step_tracers", eng.istep, n))
        eng.step(n)
    eng.step_tracers = step_tracers
    eng.tracers_advance = lambda h: calls.append(("advance", eng.istep, h))
    for n in (3, 7, 10, 1, 3, 8):
        drv.advance(n)
    print(calls)
    assert eng.istep == 32 and drv.tr_pending == 0
    # 3 | 1 + advance, 4 in one call, 2 | 2 + advance, 8 in one call | 1 | 3 + advance | 8 in one call
    assert calls == [("advance", 4, 4.0 * dt), ("step_tracers", 4, 4), ("advance", 12, 4.0 * dt), ("step_tracers", 12, 8),
                     ("advance", 24, 4.0 * dt), ("step_tracers", 24, 8)]
    drv.close()
