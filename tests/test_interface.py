"""vof_interface on the CPU, without the library: the NumPy restatement of tests/_interface_np.py (the yardstick the GPU
tests hold the kernels to, bit for bit) is judged here by geometry, not by itself.

Fixtures: F from 16 x 16 sample points per cell of a circle and of a tilted half-plane.  The circle is centred at
(0.47 Lx, 0.52 Ly) with radius 0.31 min(Lx, Ly): off the grid lines, so that no symmetry of the grid cancels errors.
"""
import math
import os
import re

import numpy as np
import pytest

import _interface_np as inp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = [(32, 32, 0.1, 0.1), (48, 80, 0.1, 0.13), (33, 17, 0.1, 0.1)]
EPS = 1e-6


def circle(Lx, Ly):
    r = 0.31 * min(Lx, Ly)
    return (lambda x, y: (x - 0.47 * Lx) ** 2 + (y - 0.52 * Ly) ** 2 < r * r), r


def half_plane(Lx, Ly):
    c, s = math.cos(math.radians(27.0)), math.sin(math.radians(27.0))
    return lambda x, y: c * x / Lx + s * y / Ly < 0.61


def fixture(shape, nx, ny, Lx, Ly):
    inside = circle(Lx, Ly)[0] if shape == "circle" else half_plane(Lx, Ly)
    return inp.supersampled(nx, ny, Lx, Ly, inside)


@pytest.mark.parametrize("shape", ["circle", "half_plane"])
@pytest.mark.parametrize("nx,ny,Lx,Ly", GRIDS)
def test_every_segment_is_the_plic_line_of_its_cell(shape, nx, ny, Lx, Ly):
    """Per mixed cell: the unit square clipped with the half-plane to the LEFT of (X0, Y0) -> (X1, Y1) has the area F to
    1e-13 (measured: 2.3e-16; the bound leaves room for another order of operations, a few hundred ulps, not a fit); both
    end points lie on the cell boundary; the liquid is on the left (cross product against the normal); the normal has unit
    length to 1e-15."""
    F, dx, dy = fixture(shape, nx, ny, Lx, Ly)
    rows, summary, unit = inp.restate(F, EPS, dx, dy)
    mixed = (EPS < F[1:-1, 1:-1]) & (F[1:-1, 1:-1] < 1 - EPS)
    assert summary["SEGMENTS"] == len(rows) == int(mixed.sum()) - summary["DEGENERATE"] > 0
    worst = {"area": 0.0, "unit": 0.0}
    for r, u in zip(rows, unit):
        i, j = int(r[0]), int(r[1])
        assert mixed[i - 1, j - 1]
        ddx, ddy = u[2] - u[0], u[3] - u[1]
        a, b = ddy, -ddx                                   # left of the direction d: d x (X - P0) > 0
        area = inp.clipped_area(a, b, a * u[0] + b * u[1])
        worst["area"] = max(worst["area"], abs(area - F[i, j]))
        for xi, eta in ((u[0], u[1]), (u[2], u[3])):
            on_edge = (xi in (0.0, 1.0) and -1e-15 <= eta <= 1 + 1e-15) or (eta in (0.0, 1.0) and -1e-15 <= xi <= 1 + 1e-15)
            assert on_edge, (i, j, xi, eta)
        # the physical end points are the unit-cell ones in the cell (i, j)
        assert r[2] == (i - 1 + u[0]) * dx and r[3] == (j - 1 + u[1]) * dy and r[4] == (i - 1 + u[2]) * dx and r[5] == (j - 1 + u[3]) * dy
        assert (r[4] - r[2]) * r[7] - (r[5] - r[3]) * r[6] < 0.0, (i, j)      # the normal (liquid -> gas) points to the right
        worst["unit"] = max(worst["unit"], abs(math.hypot(r[6], r[7]) - 1.0))
    print(shape, nx, ny, summary, worst)
    assert worst["area"] <= 1e-13 and worst["unit"] <= 1e-15
    keys = rows[:, 0] * (ny + 2) + rows[:, 1]
    assert np.all(np.diff(keys) > 0)                       # ascending (i, j)


@pytest.mark.parametrize("axis", ["x", "y"])
def test_a_flat_interface_joins_end_to_end(axis):
    nx, ny, Lx, Ly = 40, 24, 0.1, 0.06
    dx, dy = Lx / nx, Ly / ny
    F = np.zeros((nx + 2, ny + 2))
    if axis == "x":                                        # liquid below y = 9.5 dy
        F[:, :10] = 1.0
        F[:, 10] = 0.5
    else:                                                  # liquid left of x = 17.25 dx
        F[:18, :] = 1.0
        F[18, :] = 0.25
    rows, summary, _ = inp.restate(F, EPS, dx, dy)
    n, width = (nx, Lx) if axis == "x" else (ny, Ly)
    assert summary["SEGMENTS"] == n and summary["DEGENERATE"] == 0
    if axis == "x":
        assert np.all(rows[:, 3] == 9.5 * dy) and np.all(rows[:, 5] == 9.5 * dy) and np.all(rows[:, 7] == 1.0)
        assert np.array_equal(rows[1:, 4], rows[:-1, 2])   # liquid below: the segments run towards -x and meet exactly
    else:
        assert np.all(rows[:, 2] == 17.25 * dx) and np.all(rows[:, 4] == 17.25 * dx) and np.all(rows[:, 6] == 1.0)
        assert np.array_equal(rows[1:, 3], rows[:-1, 5])   # liquid on the left: towards +y
    assert abs(summary["LENGTH"] - width) <= 4 * n * 2.0 ** -53 * width


def circle_length_errors(cx=0.47, cy=0.52, rf=0.31):
    out = {}
    for n in (32, 64, 128):
        r = rf * 0.1
        F, dx, dy = inp.supersampled(n, n, 0.1, 0.1, lambda x, y: (x - cx * 0.1) ** 2 + (y - cy * 0.1) ** 2 < r * r)
        _, summary, _ = inp.restate(F, EPS, dx, dy)
        out[n] = summary["LENGTH"] / (2 * math.pi * r) - 1.0
    return out


def test_circle_length_against_2_pi_r():
    """Sum of the segment lengths against 2 pi r, measured with the restatement on this file's circle (16 x 16 samples per
    cell): +0.524 % at 32^2, +0.221 % at 64^2, +0.268 % at 128^2.  PLIC segments do not join and Youngs' normal is first-order,
    so the sum does not converge to the circumference; the figures depend on the circle (one centred on the grid's centre
    with r = 0.3 Lx reads +0.087 %, -1.184 %, +0.916 %, its small value at 32^2 being a cancellation by symmetry).  Asserted:
    each measured figure plus half of itself, and that the error at 128^2 is smaller than at 32^2."""
    measured = {32: 0.00524, 64: 0.00221, 128: 0.00268}
    err = circle_length_errors()
    print({n: "%+.4f %%" % (100 * e) for n, e in err.items()})
    for n, m in measured.items():
        assert abs(err[n]) <= 1.5 * m, (n, err[n])
    assert abs(err[128]) < abs(err[32])


def test_degenerate_nan_and_empty():
    nx, ny, dx, dy = 12, 9, 0.01, 0.02
    F = np.zeros((nx + 2, ny + 2))
    F[6, 4] = 0.5                                          # one mixed cell in all gas: the four corner gradients cancel exactly
    rows, summary, _ = inp.restate(F, EPS, dx, dy)
    assert len(rows) == 0 and summary == {"SEGMENTS": 0, "DEGENERATE": 1, "LENGTH": 0.0}
    for fill in (0.0, 1.0):
        rows, summary, _ = inp.restate(np.full((nx + 2, ny + 2), fill), EPS, dx, dy)
        assert len(rows) == 0 and summary == {"SEGMENTS": 0, "DEGENERATE": 0, "LENGTH": 0.0}
    F, dx, dy = fixture("circle", 32, 32, 0.1, 0.1)
    clean, _, _ = inp.restate(F, EPS, dx, dy)
    i, j = int(clean[5, 0]), int(clean[5, 1])
    F[i, j] = np.nan                                       # a NaN is not a mixed cell; its mixed neighbours keep their rows, with NaNs in them
    rows, summary, _ = inp.restate(F, EPS, dx, dy)
    assert summary["SEGMENTS"] == len(clean) - 1 and not ((rows[:, 0] == i) & (rows[:, 1] == j)).any()
    assert np.isnan(rows[:, 2:]).any() and math.isnan(summary["LENGTH"])


def test_length_sum_is_a_sum():
    rng = np.random.default_rng(7)
    for shape, R in (((33, 17), 4), ((70, 300), 8), ((5000, 40), 32)):
        L = rng.random(shape) * (rng.random(shape) < 0.1)
        assert abs(inp.length_sum(L, R) - math.fsum(L.ravel())) <= L.size * 2.0 ** -52 * math.fsum(L.ravel())
    assert inp.chunk_rows(4096, 4096) == 32 and inp.chunk_rows(200, 200) == 4 and inp.chunk_rows(2048, 2048) == 8


def length_sum_as_first_stated(L, R):
    """The body of _interface_np.length_sum before tests/_reduce_np.py took it over: kept as the yardstick of fixed_order."""
    TILE, SCAN_THREADS = 128, 1024
    nrows, ny = L.shape
    ntj = (ny + TILE - 1) // TILE
    Lp = np.zeros((nrows, ntj * TILE))
    Lp[:, :ny] = L
    Lp = Lp.reshape(nrows, ntj, 64, 2)
    nch = (nrows + R - 1) // R
    acc = np.zeros((nch, ntj, 64))
    for ch in range(nch):                      # a lane adds its cells row by row, column by column
        for r in range(ch * R, min(ch * R + R, nrows)):
            acc[ch] = acc[ch] + Lp[r, :, :, 0]
            acc[ch] = acc[ch] + Lp[r, :, :, 1]
    w = acc.reshape(nch * ntj, 64)             # wave = chunk * ntj + tile
    s = 32
    while s > 0:                               # lanes -> wave by __shfl_down
        new = w.copy()
        new[:, :64 - s] = w[:, :64 - s] + w[:, s:]
        w = new
        s >>= 1
    waves = w[:, 0]
    nb = (len(waves) + 3) // 4
    wv = np.zeros(nb * 4)
    wv[:len(waves)] = waves
    wv = wv.reshape(nb, 4)
    part = ((wv[:, 0] + wv[:, 1]) + wv[:, 2]) + wv[:, 3]   # waves -> block in wave order
    red = np.zeros(SCAN_THREADS)
    for start in range(0, nb, SCAN_THREADS):   # thread t takes t, t + 1024, ...
        blk = part[start:start + SCAN_THREADS]
        red[:len(blk)] = red[:len(blk)] + blk
    s = SCAN_THREADS // 2
    while s > 0:                               # ... and a tree over the threads
        red[:s] = red[:s] + red[s:2 * s]
        s >>= 1
    return float(red[0])


def test_fixed_order_has_the_bits_of_the_first_length_sum():
    """tests/_reduce_np.fixed_order on random per-cell terms: narrower than a tile, one full tile, two and three tiles with a
    ragged last one; one-row chunks, the rule's 4 and a length that divides nothing.  nrows: fewer rows than a chunk, a ragged
    last chunk, and with 1500 rows of three tiles in one-row chunks 1125 blocks -- more than the 1024 folding threads."""
    import struct
    from _reduce_np import blocks, fixed_order
    rng = np.random.default_rng(11)
    assert blocks(1500, 300, 1) == 1125
    for ny in (17, 128, 130, 300):
        for R in (1, 4, 7):
            for nrows in (3, 33, 1500 if ny == 300 else 210):
                L = rng.random((nrows, ny)) * (rng.random((nrows, ny)) < 0.3)
                got, want = fixed_order(L, R, 1024, "add"), length_sum_as_first_stated(L, R)
                assert struct.pack("d", got) == struct.pack("d", want) and got == inp.length_sum(L, R), (nrows, ny, R, got, want)
    # the other fold: a maximum does not depend on the order, so fixed_order must return np.max for any geometry and width
    M = rng.standard_normal((70, 300))
    assert fixed_order(M, 4, 256, "fmax") == M.max() and fixed_order(-np.abs(M), 2, 256, "fmax", init=0.0) == 0.0
    assert fixed_order(np.zeros((0, 40)), 4, 256, "add") == 0.0 and fixed_order(np.zeros((0, 40)), 4, 256, "fmax") == -math.inf


def test_polylines_chain_the_flat_interface_and_the_circle():
    from vof2d import interface
    nx, ny = 40, 24
    F = np.zeros((nx + 2, ny + 2))
    F[:, :10] = 1.0
    F[:, 10] = 0.5
    rows, _, _ = inp.restate(F, EPS, 0.0025, 0.0025)
    lines = interface.polylines(rows)
    assert len(lines) == 1 and lines[0].shape == (nx + 1, 2) and lines[0][0, 0] == nx * 0.0025 and lines[0][-1, 0] == 0.0
    F, dx, dy = fixture("circle", 64, 64, 0.1, 0.1)
    rows, _, _ = inp.restate(F, EPS, dx, dy)
    lines = interface.polylines(rows, tol=0.5 * dx)
    assert sum(len(p) - 1 for p in lines) == len(rows) and len(lines) <= 8
    assert interface.polylines(np.zeros((0, 8))) == []
    a, b = (rows[:40], {"SEGMENTS": 40, "DEGENERATE": 1, "LENGTH": 1.0, "ISTEP": 3}), (rows[40:], {"SEGMENTS": len(rows) - 40, "DEGENERATE": 0, "LENGTH": 2.0, "ISTEP": 3})
    both, summ = interface.combine([a, b])
    assert np.array_equal(both, rows) and summ == {"SEGMENTS": len(rows), "DEGENERATE": 1, "LENGTH": 3.0, "ISTEP": 3}


def test_the_names_are_in_the_header_and_bound():
    from vof2d import _abi, interface
    txt = open(os.path.join(ROOT, "include", "vof2d.h")).read()
    defines = dict(re.findall(r"#define (VOF_IFACE_[A-Z0-9_]+) (\d+)", txt))
    assert len(defines) == 14
    for name, value in defines.items():
        assert getattr(_abi, name) == int(value), name
    assert re.search(r"int vof_interface\(vof2d_handle h, double eps, double\* rows, int64_t cap_rows, double\* summary", txt)
    assert "interface" in _abi.SIGNATURES and "interface" in _abi.GPU_ONLY
    assert [getattr(interface, n) for n in interface.NAMES] == list(range(_abi.VOF_IFACE_N)) and len(interface.SUMMARY) == _abi.VOF_IFACE_SUM_N
    args = __import__("vof2d.cli", fromlist=["cli"]).parse_args(["--interface-every", "5"])
    assert args.interface_every == 5
