"""The restatement of vof_depths and of a gauge's row (tests/_depths_np.py) judged on its own, without a GPU: on states whose
marginals, tops and fronts are known in closed form, on the bound of the ordered sums against math.fsum (derived in that
module, not measured), on a bilinear field (where the bilinear sample is exact), and vof2d/gauges.py (derive, combine) on
split arrays.  tests/test_depths_gpu.py and tests/test_gauges_gpu.py hold the device to this restatement.
"""
import math

import numpy as np
import pytest

import _depths_np as dnp
import _tracers_np as tnp
import vof_oracle_np as onp
from vof2d import _abi, gauges


def block(nx, ny, a, b, dtype=np.float64):
    """F = 1 on the cells i <= a, j <= b (ghost cells included on that side, as set_init_F leaves them), 0 elsewhere."""
    F = np.zeros((nx + 2, ny + 2), dtype=dtype)
    F[:a + 1, :b + 1] = 1.0
    return F


def hold_block(res, di, dj, total, nx, ny, a, b):
    assert res["rows"] == nx and res["top"].dtype == np.int32
    assert di.tolist() == [float(b)] * a + [0.0] * (nx - a) and dj.tolist() == [float(a)] * b + [0.0] * (ny - b)
    assert res["top"].tolist() == [b] * a + [0] * (nx - a)
    assert (res["front_lo"], res["front_hi"], res["top_j"]) == ((1, a, b) if a and b else (0, 0, 0)) and total == float(a * b)


# ---------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("nx,ny,a,b", [(32, 32, 11, 16), (24, 40, 8, 20)])
def test_the_dam_at_step_0(nx, ny, a, b):
    """-ic 1 (2dvof.py:141-143): F = 1 where the node (i - 1) dx <= Lx / 3 and (j - 1) dy <= Ly / 2 in the coordinates' float32:
    i <= 11, j <= 16 on 32 x 32 (10.67 and 16 cells); on 24 x 40 the two comparisons are ties the float32 grid decides
    against, i <= 8, j <= 20.  Every sum is a count of ones: exact in any order."""
    s = onp.new_state(nx, ny, 1, np.float64, "f32")
    assert np.array_equal(s.F, block(nx, ny, a, b))
    res = dnp.restate(s.F)
    for R in (2, 4, 32):
        di, dj, total = dnp.ordered(res["terms"], R)
        hold_block(res, di, dj, total, nx, ny, a, b)
    d = gauges.derive(di, dnp.summary(res, total, 0), s.prm.dx, s.prm.dy)
    assert d["front_lo"] == 0.0 and d["front_hi"] == a * s.prm.dx and d["volume"] == a * b * s.prm.dx * s.prm.dy
    assert d["depth"].tolist() == [b * s.prm.dy] * a + [0.0] * (nx - a) and d["x"][0] == 0.5 * s.prm.dx and d["x"][-1] == (nx - 0.5) * s.prm.dx


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_a_staircase(dtype):
    """Row i holds liquid up to j = h(i) = 1 + (7 i) % 37, the cell above it 0.25 (below the threshold), on 40 x 150 (two
    tiles): depth_i = h + 0.25, top = h, depth_j[j] = #{i: h(i) >= j} + 0.25 #{i: h(i) == j - 1}; dyadic values, exact."""
    nx, ny = 40, 150
    h = [1 + (7 * i) % 37 for i in range(1, nx + 1)]
    F = np.zeros((nx + 2, ny + 2), dtype=dtype)
    for i, hi in enumerate(h, 1):
        F[i, 1:hi + 1] = 1.0
        F[i, hi + 1] = 0.25
    res = dnp.restate(F)
    di, dj, total = dnp.ordered(res["terms"], 2)
    assert di.tolist() == [hi + 0.25 for hi in h] and res["top"].tolist() == h
    assert dj.tolist() == [sum(hi >= j for hi in h) + 0.25 * sum(hi == j - 1 for hi in h) for j in range(1, ny + 1)]
    assert (res["front_lo"], res["front_hi"], res["top_j"]) == (1, nx, max(h)) and total == sum(h) + 0.25 * nx
    # the floor dry left of row 7 and right of row 30
    F[1:7, 1] = 0.0
    F[31:, 1] = 0.49
    res = dnp.restate(F)
    assert (res["front_lo"], res["front_hi"]) == (7, 30) and res["top"].tolist()[:6] == [hi if hi > 1 else 0 for hi in h[:6]]


def test_all_gas_and_all_liquid():
    nx, ny = 33, 130
    for value, a, b in ((0.0, 0, 0), (1.0, nx, ny)):
        F = np.full((nx + 2, ny + 2), value)
        res = dnp.restate(F)
        di, dj, total = dnp.ordered(res["terms"], 2)
        hold_block(res, di, dj, total, nx, ny, a, b)
    # exactly 0.5 is a member, the float below it is not; a NaN is not, and reaches its own row and column alone
    F = np.zeros((nx + 2, ny + 2))
    F[5, 1], F[6, 1], F[9, 70], F[20, 129] = 0.5, np.nextafter(0.5, 0), np.nan, 0.5
    res = dnp.restate(F)
    di, dj, total = dnp.ordered(res["terms"], 2)
    assert (res["front_lo"], res["front_hi"], res["top_j"]) == (5, 5, 129) and res["top"][4] == 1 and res["top"][5] == 0 and res["top"][8] == 0
    assert np.isnan(di).nonzero()[0].tolist() == [8] and np.isnan(dj).nonzero()[0].tolist() == [69] and math.isnan(total)
    assert dnp.within_bound(total, res["terms"]) and not dnp.within_bound(1.0, res["terms"])


def test_strips_and_a_strip_that_owns_nothing():
    rng = np.random.default_rng(0)
    F = rng.uniform(0, 1, (40 + 2, 17 + 2))
    whole = dnp.restate(F)
    part = dnp.restate(F[10:35], lo=12, hi=30, row0=10)
    assert np.array_equal(part["terms"], whole["terms"][11:30]) and np.array_equal(part["top"], whole["top"][11:30]) and part["first"] == 12
    none = dnp.restate(F[0:3], lo=2, hi=1, row0=0)
    di, dj, total = dnp.ordered(none["terms"], 2)
    assert none["rows"] == 0 and len(di) == 0 and dj.tolist() == [0.0] * 17 and total == 0.0
    assert (none["front_lo"], none["front_hi"], none["top_j"]) == (0, 0, 0)


# ---------------------------------------------------------------------------- the ordered sums against fsum
@pytest.mark.parametrize("nx,ny,R", [(33, 17, 2), (96, 130, 2), (200, 200, 2), (130, 300, 8)])
def test_ordered_sums_lie_within_the_derived_bound(nx, ny, R):
    rng = np.random.default_rng(nx * 1000 + ny)
    # F of a real run is in [0, 1] with tiny excursions; signs and eleven decades of magnitude make cancellation count
    t = rng.uniform(-1, 1, (nx, ny)) * 10.0 ** rng.integers(-8, 3, (nx, ny))
    F = np.zeros((nx + 2, ny + 2))
    F[1:-1, 1:-1] = t
    res = dnp.restate(F)
    di, dj, total = dnp.ordered(res["terms"], R)
    worst = 0.0
    for r in range(nx):
        assert dnp.within_bound(di[r], t[r]), r
        worst = max(worst, abs(di[r] - math.fsum(t[r])) / dnp.bound_of(t[r]))
    for c in range(ny):
        assert dnp.within_bound(dj[c], t[:, c]), c
    assert dnp.within_bound(total, t)
    print("%dx%d R %d: worst |depth_i - fsum| / bound %.3f; SUM off by %.3e of a bound %.3e" % (nx, ny, R, worst, abs(total - math.fsum(t.ravel())), dnp.bound_of(t)))
    # the order is part of the value: another chunk length changes bits of depth_j at most, never depth_i
    di2, dj2, _ = dnp.ordered(res["terms"], 2 * R)
    assert np.array_equal(di, di2) and all(dnp.within_bound(dj2[c], t[:, c]) for c in range(ny))


def test_the_chunk_rule_and_the_partial_counts():
    assert [dnp.depths_chunk_rows(*g) for g in ((33, 17), (96, 130), (200, 200), (1100, 130), (2048, 2048), (4096, 4096), (8192, 8192))] == [2, 2, 2, 2, 8, 32, 32]
    assert dnp.depths_chunk_rows(120, 70, 22, 98) == 2                    # a strip: by the rows it can compute
    assert dnp.partial_counts(1100, 130, 2) == (2200, 550 * 130) and dnp.partial_counts(0, 130, 2) == (0, 0) and dnp.partial_counts(33, 17, 2) == (33, 17 * 17)


# ---------------------------------------------------------------------------- the gauges' rows
def test_gauge_rows_on_a_bilinear_field():
    """p = 3 + 2 x - 5 y + 40 x y laid on the cell centres ((i - 0.5) dx, (j - 0.5) dy), ghost cells included: the bilinear
    sample of a bilinear function is the function, to rounding (a few ulp of the largest term); positions inside the band of
    cell centres.  DEPTH and TOP come from the row above X: ig = floor(X dxi) + 1 held to [1, nx]."""
    nx, ny, Lx, Ly = 12, 20, 0.75, 0.5          # (dx = 1 / 16: the faces are exact)
    dx, dy = Lx / nx, Ly / ny
    g = tnp.Grid(nx, ny, 1 / dx, 1 / dy, Lx, Ly)
    i = np.arange(nx + 2, dtype=np.float64)[:, None]
    j = np.arange(ny + 2, dtype=np.float64)[None, :]
    xc, yc = (i - 0.5) * dx, (j - 0.5) * dy
    p = 3 + 2 * xc - 5 * yc + 40 * xc * yc
    F = block(nx, ny, 5, 8)
    z = np.zeros_like(p)
    res = dnp.restate(F)
    di, _, _ = dnp.ordered(res["terms"], 2)
    rng = np.random.default_rng(1)
    xy = np.stack([rng.uniform(0, Lx, 200), rng.uniform(0, Ly, 200)], axis=1)
    xy[:6] = [(0.0, 0.0), (Lx, Ly), (Lx, 0.0), (0.0, Ly), (5 * dx, 0.1), (np.nextafter(5 * dx, 0), 0.1)]
    rows = dnp.gauge_rows(F, z, z, p, xy, g, di, res["top"], dy)
    assert rows.shape == (200, dnp.GAUGE_N) and np.array_equal(rows[:, :2], xy) and not rows[:, [dnp.U, dnp.V]].any()
    exact = 3 + 2 * xy[:, 0] - 5 * xy[:, 1] + 40 * xy[:, 0] * xy[:, 1]
    assert np.abs(rows[:, dnp.P] - exact).max() <= 16 * 2.0 ** -52 * 32.0       # (|p| < 32 on the domain; a dozen roundings)
    ig = np.clip(np.floor(xy[:, 0] * g.dxi).astype(int) + 1, 1, nx)
    assert ig[:6].tolist() == [1, nx, nx, 1, 6, 5]
    assert rows[:, dnp.DEPTH].tolist() == [(8.0 if k <= 5 else 0.0) * dy for k in ig] and rows[:, dnp.TOP].tolist() == [8.0 if k <= 5 else 0.0 for k in ig]
    # F sampled across the dam's edge: 1 deep inside, 0 far outside, between on the edge cells
    assert rows[4, dnp.F] == 0.5 and (rows[:, dnp.F] >= 0).all() and (rows[:, dnp.F] <= 1).all()


def test_slot_names_agree():
    assert gauges.NAMES == ("X", "Y", "U", "V", "F", "P", "DEPTH", "TOP") and (dnp.X, dnp.Y, dnp.U, dnp.V, dnp.F, dnp.P, dnp.DEPTH, dnp.TOP) == tuple(range(8))
    assert (gauges.X, gauges.P, gauges.DEPTH, gauges.TOP) == (_abi.VOF_GAUGE_X, _abi.VOF_GAUGE_P, _abi.VOF_GAUGE_DEPTH, _abi.VOF_GAUGE_TOP)
    assert gauges.DEPTH_SUMMARY == ("ROWS", "ISTEP", "FRONT_LO", "FRONT_HI", "TOP_J", "SUM") and dnp.SUM == _abi.VOF_DEPTH_SUM_SUM == 5
    assert dnp.SUM_N == _abi.VOF_DEPTH_SUM_N and dnp.GAUGE_N == _abi.VOF_GAUGE_N == 8 and _abi.VOF_GAUGE_SUM_N == 8
    assert gauges.summary_of([3.0, 7.0, 2.0, 0, 0, 0, 0, 0]) == {"COUNT": 3, "ISTEP": 7, "RECORDS": 2}
    with pytest.raises(ValueError):
        gauges.summary_of([1.0, 2.0])


# ---------------------------------------------------------------------------- vof2d/gauges.py
def test_combine_joins_split_arrays():
    rng = np.random.default_rng(2)
    nx, ny = 60, 33
    F = np.zeros((nx + 2, ny + 2))
    F[1:-1, 1:-1] = rng.uniform(0, 1, (nx, ny))
    F[1:13, 1] = 0.0                               # the floor is dry left of row 13 and right of row 44
    F[45:, 1] = 0.0
    F[13, 1] = F[44, 1] = 0.75
    whole = dnp.restate(F)
    di, dj, total = dnp.ordered(whole["terms"], 2)
    parts = []
    for lo, hi in ((1, 10), (11, 40), (41, 60)):   # the first strip has a dry floor
        res = dnp.restate(F, lo=lo, hi=hi)
        a, b, t = dnp.ordered(res["terms"], 2)
        parts.append((a, b, res["top"], list(dnp.summary(res, t, 5))))
    ci, cj, ctop, cs = gauges.combine(parts)
    assert np.array_equal(ci, di) and np.array_equal(ctop, whole["top"]) and ctop.dtype == np.int32
    assert cs["ROWS"] == nx and cs["ISTEP"] == 5 and (cs["FRONT_LO"], cs["FRONT_HI"], cs["TOP_J"]) == (13, 44, whole["top_j"]) == (whole["front_lo"], whole["front_hi"], whole["top_j"])
    assert all(dnp.within_bound(cj[c], whole["terms"][:, c]) for c in range(ny)) and dnp.within_bound(cs["SUM"], whole["terms"])
    assert np.array_equal(cj, (parts[0][1] + parts[1][1]) + parts[2][1]) and cs["SUM"] == (parts[0][3][dnp.SUM] + parts[1][3][dnp.SUM]) + parts[2][3][dnp.SUM]
    one = gauges.combine(parts[1:2])
    assert np.array_equal(one[0], parts[1][0]) and one[3]["FRONT_LO"] == 13
    dry = gauges.combine([parts[0], parts[0]])
    assert (dry[3]["FRONT_LO"], dry[3]["FRONT_HI"]) == (0, 0) and math.isnan(gauges.derive(dry[0], dry[3], 0.1, 0.1)["front_hi"])
    bad = list(parts[2][3]); bad[dnp.ISTEP] = 6
    with pytest.raises(ValueError):
        gauges.combine([parts[0], (parts[2][0], parts[2][1], parts[2][2], bad)])
    d = gauges.derive(ci[10:40], parts[1][3], 0.5, 0.25, first=11)
    assert d["x"][0] == 10.5 * 0.5 and d["front_lo"] == 12 * 0.5 and d["front_hi"] == 40 * 0.5 and np.array_equal(d["depth"], ci[10:40] * 0.25)


def test_positions_and_csv_lines(tmp_path):
    f = tmp_path / "g.txt"
    f.write_text("# x y\n0.01 0.02\n\n0.03,0.04\n")
    xy = gauges.parse_positions(["0.05,0.06"], str(f))
    assert xy.tolist() == [[0.05, 0.06], [0.01, 0.02], [0.03, 0.04]] and gauges.parse_positions().shape == (0, 2)
    with pytest.raises(ValueError):
        gauges.parse_positions(["0.05"])
    lines = gauges.gauges_csv_lines(12, np.arange(16, dtype=np.float64).reshape(2, 8))
    assert lines[1].split(",")[:3] == ["12", "1", "8.0"] and len(lines[0].split(",")) == len(gauges.GAUGES_CSV_HEADER.split(",")) == 10
    line = gauges.depths_csv_line([60, 12, 13, 44, 30, 100.0, 0, 0], 0.5, 0.25)
    assert line == "12,13,44,30,12.5" and len(gauges.DEPTHS_CSV_HEADER.split(",")) == 5
