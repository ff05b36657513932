"""vof_regrid, the method: properties of the operators of kernels/regrid.h, checked on their NumPy restatement (tests/_regrid_np.py)
with the golden states of tests/golden, in float64.  No GPU, no library: what the kernels are held to bit for bit
(tests/test_regrid_gpu.py) is held to what the method promises here.

The two measured bounds (printed; recorded in profiles/regrid.md): CONSERVATION = 4 x the largest |mean of a parent's children -
parent's F| the restatement shows over the golden states and the factors below; DIVERGENCE = 4 x the largest |child divergence -
parent divergence| over the same, in units of (max|u| rx / dx + max|v| ry / dy) of the state.  They are measured against the
restatement, never the library; the flat-pool and round-trip tests use them on other inputs.  Beside the measured bound the
divergence defect is held to one from the formats: a child face is one rounded product and one rounded sum away from exact
(2 x 2^-53 relative to max|u| each), a divergence takes two differences of two faces each and two divisions: 16 x 2^-52 units
covers it with room.
"""
import functools
import os
from fractions import Fraction

import numpy as np
import pytest

import _interface_np as inp
import _regrid_np as rnp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATES = [("dam32_f64", 10), ("dam32_f64", 100), ("bubble33x17_f64", 10), ("bubble33x17_f64", 100), ("dam128_f64", 100), ("dam128_f64", 1000)]
FACTORS = [(2, 2), (2, 3), (4, 4), (3, 1), (16, 16)]
L = 0.1
EPS = 1e-6


@functools.lru_cache(maxsize=None)
def state(name, step):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return {n: z["%s_%d" % (n, step)] for n in rnp.FIELDS}


def cell_sizes(s):
    return L / (s["F"].shape[0] - 2), L / (s["F"].shape[1] - 2)


def block_mean(x, rx, ry):
    nx, ny = x.shape[0] // rx, x.shape[1] // ry
    return x.reshape(nx, rx, ny, ry).mean(axis=(1, 3))


def divergence(u, v, dx, dy):
    """Of dense u, v (ghost cells included) on the interior cells."""
    nx, ny = u.shape[0] - 2, u.shape[1] - 2
    return (u[2:nx + 2, 1:ny + 1] - u[1:nx + 1, 1:ny + 1]) / dx + (v[1:nx + 1, 2:ny + 2] - v[1:nx + 1, 1:ny + 1]) / dy


@functools.lru_cache(maxsize=None)
def measured():
    """(conservation defect, divergence defect in units, children outside [0, 1]) over STATES x FACTORS."""
    cons = div = 0.0
    outside = 0
    for name, step in STATES:
        s = state(name, step)
        dx, dy = cell_sizes(s)
        nx, ny = s["F"].shape[0] - 2, s["F"].shape[1] - 2
        F0 = s["F"][1:nx + 1, 1:ny + 1]
        inside = (F0 >= 0.0) & (F0 <= 1.0)
        d0 = divergence(s["u"], s["v"], dx, dy)
        for rx, ry in FACTORS:
            inner, nplic, _ = rnp.refine_interior(s, rx, ry, True, EPS, dx, dy)
            assert nplic > 0
            Fc = inner["F"]
            up = np.repeat(np.repeat(inside, rx, axis=0), ry, axis=1)
            outside += int((up & ((Fc < 0.0) | (Fc > 1.0))).sum())
            cons = max(cons, float(np.max(np.abs(block_mean(Fc, rx, ry) - F0))))
            # the children's divergence from their own faces: the face behind the last child is the parent's next face (k = 0 of I + 1)
            uf = np.concatenate([inner["u"], np.repeat(s["u"][nx + 1:nx + 2, 1:ny + 1], ry, axis=1)], axis=0)
            vf = np.concatenate([inner["v"], np.repeat(s["v"][1:nx + 1, ny + 1:ny + 2], rx, axis=0)], axis=1)
            dc = (uf[1:] - uf[:-1]) / (dx / rx) + (vf[:, 1:] - vf[:, :-1]) / (dy / ry)
            unit = np.max(np.abs(s["u"])) * rx / dx + np.max(np.abs(s["v"])) * ry / dy
            div = max(div, float(np.max(np.abs(dc - np.repeat(np.repeat(d0, rx, axis=0), ry, axis=1)))) / unit)
    return cons, div, outside


def conservation_bound():
    return 4.0 * measured()[0]


def test_children_lie_in_the_unit_interval_and_keep_the_parents_volume():
    cons, div, outside = measured()
    print("regrid: largest |mean(children) - parent| = %.3e -> CONSERVATION bound %.3e; largest divergence defect %.3e units -> DIVERGENCE bound %.3e"
          % (cons, 4 * cons, div, 4 * div))
    assert outside == 0
    assert 0.0 < cons < 32 * 2.0 ** -52          # a few ulp of 1: each child is a handful of roundings of values in [0, 1], and the mean of at most 256 of them
    assert div <= 16 * 2.0 ** -52                # the bound from the formats (module docstring)


def test_the_line_is_the_one_vof_interface_cuts():
    """line() restates iface_line; _interface_np.restate the same expressions up to the segment: the same cells, and the end
    points that a, b, alpha give are the rows'."""
    for name, step in STATES[:4]:
        s = state(name, step)
        dx, dy = cell_sizes(s)
        kind, a, b, alpha, fx, fy = rnp.line(s["F"], EPS, dx, dy)
        rows, summ, unit = inp.restate(s["F"], EPS, dx, dy)
        ii, jj = np.nonzero(kind == 2)
        assert summ["SEGMENTS"] == len(ii) and summ["DEGENERATE"] == int((kind == 1).sum())
        assert np.array_equal(rows[:, 0], ii + 1.0) and np.array_equal(rows[:, 1], jj + 1.0)
        a, b, alpha, fx, fy = (x[ii, jj] for x in (a, b, alpha, fx, fy))
        with np.errstate(all="ignore"):
            p_left, q_bottom = (b > 0.0) & (alpha <= b), (a > 0.0) & (alpha <= a)
            pxi, peta = np.where(p_left, 0.0, (alpha - b) / a), np.where(p_left, alpha / b, 1.0)
            qxi, qeta = np.where(q_bottom, alpha / a, 1.0), np.where(q_bottom, 0.0, (alpha - a) / b)
        pxi, qxi = np.where(fx, 1.0 - pxi, pxi), np.where(fx, 1.0 - qxi, qxi)
        peta, qeta = np.where(fy, 1.0 - peta, peta), np.where(fy, 1.0 - qeta, qeta)
        first = fx != fy
        mine = np.stack([np.where(first, pxi, qxi), np.where(first, peta, qeta), np.where(first, qxi, pxi), np.where(first, qeta, peta)], axis=1)
        assert np.array_equal(mine, unit)


def pool(nx, ny, rx, ry, normal, c):
    """F of the half-plane normal . (x, y) < c, lengths in cells of the nx x ny grid, on that grid refined by (rx, ry), ghost
    cells sampled like any other.  The clip runs in rational arithmetic (a reference in doubles, alpha = c - (j - 1) dy, would
    carry an error of ulp(c) / dy, ten times the bound it is to check): every value is the exact area, rounded once."""
    F = np.zeros((nx * rx + 2, ny * ry + 2))
    a, b = Fraction(normal[0], rx), Fraction(normal[1], ry)
    for i in range(nx * rx + 2):
        for j in range(ny * ry + 2):
            F[i, j] = inp.clipped_area(a, b, c - a * (i - 1) - b * (j - 1))
    return F


@pytest.mark.parametrize("normal,c", [((0, 1), Fraction(5243, 1000)), ((1, 0), Fraction(7331, 1000)), ((1, 1), Fraction(10477, 1000)), ((-1, 1), Fraction(-1523, 1000))],
                         ids=["horizontal", "vertical", "diagonal", "antidiagonal"])
@pytest.mark.parametrize("rx,ry", FACTORS[:4])
def test_a_flat_pool_is_refined_exactly(normal, c, rx, ry):
    nx = ny = 12
    F = pool(nx, ny, 1, 1, normal, c)
    assert ((F > EPS) & (F < 1 - EPS)).sum() >= nx
    z = np.zeros_like(F)
    inner, nplic, ndeg = rnp.refine_interior({"F": F, "u": z, "v": z, "p": z}, rx, ry, True, EPS, L / nx, L / ny)
    exact = pool(nx, ny, rx, ry, normal, c)[1:-1, 1:-1]
    err = float(np.max(np.abs(inner["F"] - exact)))
    print("flat pool %s x (%d, %d): %d cells from a line, max error %.3e (bound %.3e)" % (normal, rx, ry, nplic, err, conservation_bound()))
    assert nplic > 0 and ndeg == 0
    assert err <= conservation_bound()


def test_coarsening_gives_the_mean_of_the_childrens_divergences():
    div_bound = 4.0 * measured()[1]
    for name, step in STATES:
        s = state(name, step)
        dx, dy = cell_sizes(s)
        nx, ny = s["F"].shape[0] - 2, s["F"].shape[1] - 2
        for rx, ry in ((2, 2), (4, 8), (3, 1)):
            if nx % rx or ny % ry:
                continue
            c = rnp.coarsen_interior(s, rx, ry)
            # the coarse faces behind the last cells: the walls, where u and v are 0 in a state that holds its boundary conditions
            uc = np.concatenate([c["u"], np.zeros((1, ny // ry))], axis=0)
            vc = np.concatenate([c["v"], np.zeros((nx // rx, 1))], axis=1)
            assert not s["u"][nx + 1, 1:ny + 1].any() and not s["v"][1:nx + 1, ny + 1].any()
            dc = (uc[1:] - uc[:-1]) / (dx * rx) + (vc[:, 1:] - vc[:, :-1]) / (dy * ry)
            mean = block_mean(divergence(s["u"], s["v"], dx, dy), rx, ry)
            unit = np.max(np.abs(s["u"])) / dx + np.max(np.abs(s["v"])) / dy
            # sums of rx (ry) faces and of rx ry divergences: their roundings, in the units of the fine divergence
            assert float(np.max(np.abs(dc - mean))) / unit <= max(div_bound, (rx * ry + 8) * 2.0 ** -52), (name, step, rx, ry)


@pytest.mark.parametrize("rx,ry", [(2, 2), (4, 8), (16, 1), (1, 4)])
def test_round_trip_through_a_power_of_two(rx, ry):
    for name, step in STATES[:5]:
        s = state(name, step)
        nx, ny = s["F"].shape[0] - 2, s["F"].shape[1] - 2
        for plic in (False, True):
            fine, _ = rnp.restate(s, nx * rx, ny * ry, np.float64, plic=plic, eps=EPS)
            back, summ = rnp.restate(fine, nx, ny, np.float64)
            assert summ["DIR"] == -1.0 and (summ["RX"], summ["RY"]) == (rx, ry)
            inner = (slice(1, nx + 1), slice(1, ny + 1))
            assert np.array_equal(back["u"][inner], s["u"][inner]) and np.array_equal(back["v"][inner], s["v"][inner])
            if plic:
                assert float(np.max(np.abs(back["F"][inner] - s["F"][inner]))) <= conservation_bound()
            else:
                assert np.array_equal(back["F"][inner], s["F"][inner])


def test_the_same_grid_is_the_identity_and_a_conversion():
    for name, step in STATES[:5]:
        s = state(name, step)
        nx, ny = s["F"].shape[0] - 2, s["F"].shape[1] - 2
        same, summ = rnp.restate(s, nx, ny, np.float64, istep=step)
        assert (summ["RX"], summ["RY"], summ["DIR"], summ["PLIC_CELLS"], summ["ISTEP"]) == (1.0, 1.0, 0.0, 0.0, float(step))
        assert summ["F_SRC"] == summ["F_DST"]
        single, _ = rnp.restate(s, nx, ny, np.float32)
        for n in rnp.FIELDS:
            assert same[n].tobytes() == s[n].tobytes(), n        # (the golden states hold their boundary conditions: the ring too)
            assert single[n].dtype == np.float32 and single[n].tobytes() == s[n].astype(np.float32).tobytes(), n


def test_factors_mirror_the_c_check():
    from vof2d.regrid import factors
    assert factors(33, 17, 66, 51) == (2, 3, 1) and factors(128, 128, 32, 16) == (4, 8, -1) and factors(33, 17, 33, 17) == (1, 1, 0)
    assert factors(128, 128, 384, 128) == (3, 1, 1) and factors(33, 17, 11, 17) == (3, 1, -1) and factors(64, 64, 1024, 1024) == (16, 16, 1)
    for bad in ((64, 64, 128, 32), (64, 64, 96, 64), (64, 64, 1088, 64), (1088, 64, 64, 64), (0, 64, 64, 64), (33, 17, 66, 50)):
        with pytest.raises(ValueError):
            factors(*bad)
