"""vof_curvature on the CPU, without the library: the NumPy restatement of tests/_curvature_np.py (the yardstick the GPU tests hold the
kernels to, bit for bit) is judged here against analysis, not by itself; then the derived quantities, the CSV line and the options.

The method test: discs whose area fractions are integrated analytically (the 8 x 8 samples of the scene painter are too coarse for
second differences), centred at ((nx / 2 + 0.37) dx, (ny / 2 + 0.21) dy) -- off the cell centres, so that no symmetry of the grid
cancels errors.  Errors are relative errors against -1/R (a drop) or +1/R (a bubble).  Measured with the restatement:

    case                 rows  valid (share)   HF median   HF max    CSF median  CSF max
    drop   48x48  R 12    96    93 (0.969)     0.00315     0.00523   0.333       1.77
    bubble 48x48  R 12    96    93 (0.969)     0.00315     0.00523   0.333       1.77
    drop   96x96  R 24   192   191 (0.995)     0.00079     0.00135   0.470       3.72
    drop   40x64  R 10    69    66 (0.957)     0.00635     0.01220   0.214       1.56      (dy = 1.3 dx)

The height-function median falls at second order (0.00079 / 0.00315 = 0.25); the solver's own curvature does not converge.  The absolute
bounds below are these figures with a margin of 2x.
"""
import math

import numpy as np
import pytest

import _curvature_np as cnp

EPS = 1e-6
#        name          nx  ny  dy/dx  R     bubble  HF median, HF max as measured
DISCS = [("drop48", 48, 48, 1.0, 12.0, False, 0.00315, 0.00523),
         ("bubble48", 48, 48, 1.0, 12.0, True, 0.00315, 0.00523),
         ("drop96", 96, 96, 1.0, 24.0, False, 0.00079, 0.00135),
         ("drop40x64", 40, 64, 1.3, 10.0, False, 0.00635, 0.01220)]
MARGIN = 2.0
_measured = {}


def measured(name):
    """rows, summary, the relative errors of KAPPA (valid rows) and of KAPPA_CSF (all rows), the exact curvature: computed once a case."""
    if name not in _measured:
        _, nx, ny, ratio, R, bubble, _, _ = next(c for c in DISCS if c[0] == name)
        dx, dy = 1.0, ratio
        F = cnp.disc(nx, ny, dx, dy, (nx / 2 + 0.37) * dx, (ny / 2 + 0.21) * dy, R)
        rows, summ = cnp.restate(1.0 - F if bubble else F, EPS, dx, dy)
        want = (1.0 if bubble else -1.0) / R
        valid = rows[:, cnp.VALID] == 1.0
        _measured[name] = (rows, summ, np.abs(rows[valid, cnp.KAPPA] - want) / abs(want), np.abs(rows[:, cnp.KAPPA_CSF] - want) / abs(want), want)
    return _measured[name]


def test_the_analytic_disc_has_the_area_of_a_disc():
    F = cnp.disc(48, 48, 1.0, 1.3, 24.37, 31.2, 12.0)
    assert abs(F.sum() * 1.3 - math.pi * 144.0) < 1e-9 and F.min() == 0.0 and F.max() == 1.0


@pytest.mark.parametrize("name", [c[0] for c in DISCS])
def test_height_functions_measure_a_disc(name):
    _, nx, ny, ratio, R, bubble, med, worst = next(c for c in DISCS if c[0] == name)
    rows, summ, ek, ec, want = measured(name)
    valid = rows[:, cnp.VALID] == 1.0
    print(name, "rows", len(rows), "valid", int(valid.sum()), "share %.4f" % valid.mean(), "HF median %.5f max %.5f" % (np.median(ek), ek.max()),
          "CSF median %.4f max %.4f" % (np.median(ec), ec.max()))
    assert summ["ROWS"] == len(rows) and summ["VALID"] == valid.sum() and summ["DEGENERATE"] == 0
    assert valid.mean() >= 0.95
    assert np.all(np.sign(rows[valid, cnp.KAPPA]) == np.sign(want))            # -1/R for a drop, +1/R for a bubble: the solver's sign
    assert np.median(ek) < np.median(ec)                                        # nearer the truth than the solver's own
    assert np.median(ek) <= MARGIN * med and ek.max() <= MARGIN * worst
    assert np.all(rows[~valid, cnp.KAPPA] == 0.0) and np.all(rows[~valid, cnp.HP] == 0.0)
    assert summ["MIN_K"] == rows[valid, cnp.KAPPA].min() and summ["MAX_K"] == rows[valid, cnp.KAPPA].max()
    assert summ["MIN_CSF"] == rows[:, cnp.KAPPA_CSF].min() and summ["MAX_CSF"] == rows[:, cnp.KAPPA_CSF].max()
    assert math.isclose(summ["SUM_K"], rows[valid, cnp.KAPPA].sum(), rel_tol=1e-12) and math.isclose(summ["SUM_CSF2"], (rows[:, cnp.KAPPA_CSF] ** 2).sum(), rel_tol=1e-12)


def test_the_median_error_falls_at_second_order():
    e12, e24 = np.median(measured("drop48")[2]), np.median(measured("drop96")[2])
    print("median error, radius 12: %.5f, radius 24: %.5f, ratio %.3f" % (e12, e24, e24 / e12))
    assert e24 < 0.5 * e12                                                      # (second order predicts a quarter)


def test_a_drop_and_its_bubble_mirror_each_other():
    d, b = measured("drop48")[0], measured("bubble48")[0]
    assert np.array_equal(d[:, :2], b[:, :2]) and np.array_equal(d[:, cnp.VALID], b[:, cnp.VALID]) and np.array_equal(d[:, cnp.AXIS], b[:, cnp.AXIS])
    assert np.allclose(d[:, cnp.KAPPA], -b[:, cnp.KAPPA], rtol=1e-9, atol=1e-12)


def pool(nx=24, ny=20, level=9):
    F = np.zeros((nx + 2, ny + 2))
    F[:, :level] = 1.0
    F[:, level] = 0.3
    return F


def test_a_flat_pool_is_flat_along_j():
    rows, summ = cnp.restate(pool(), EPS, 0.01, 0.013)
    assert len(rows) == 24 == summ["ROWS"] == summ["VALID"] and summ["DEGENERATE"] == 0
    assert np.all(rows[:, cnp.J] == 9) and np.array_equal(rows[:, cnp.I], np.arange(1, 25))
    assert np.all(rows[:, cnp.VALID] == 1.0) and np.all(rows[:, cnp.AXIS] == 0.0) and np.all(rows[:, cnp.FVAL] == 0.3)
    assert np.all(rows[:, cnp.KAPPA] == 0.0) and np.all(rows[:, cnp.HP] == 0.0)
    assert summ["SUM_K"] == 0.0 == summ["MIN_K"] == summ["MAX_K"]
    assert np.all(rows[1:-1, cnp.KAPPA_CSF] == 0.0)                              # (the solver's own: flat away from the side walls)


def test_the_transposed_pool_is_flat_along_i():
    rows, summ = cnp.restate(pool().T.copy(), EPS, 0.013, 0.01)
    assert len(rows) == 24 == summ["VALID"] and np.all(rows[:, cnp.I] == 9)
    assert np.all(rows[:, cnp.VALID] == 1.0) and np.all(rows[:, cnp.AXIS] == 1.0) and np.all(rows[:, cnp.KAPPA] == 0.0)
    F = 1.0 - pool().T                                                           # the liquid on the high-i side: the same heights from the other end
    rows, summ = cnp.restate(F, EPS, 0.013, 0.01)
    assert len(rows) == 24 == summ["VALID"] and np.all(rows[:, cnp.AXIS] == 1.0) and np.all(rows[:, cnp.KAPPA] == 0.0)


def test_a_stencil_without_both_phases_is_not_valid_and_nothing_is_the_empty_summary():
    F = np.zeros((26, 22))
    F[:, :3] = 0.5                                                               # a film: no full cell under the surface
    rows, summ = cnp.restate(F, EPS, 0.01, 0.01)
    assert summ["VALID"] == 0 and np.all(rows[:, cnp.KAPPA] == 0.0)
    assert summ["MAX_K"] == -math.inf and summ["MIN_K"] == math.inf and summ["SUM_K"] == 0.0
    rows, summ = cnp.restate(np.zeros((26, 22)), EPS, 0.01, 0.01)
    assert rows.shape == (0, 8) and summ["ROWS"] == 0 and summ["MAX_CSF"] == -math.inf and summ["MIN_CSF"] == math.inf


# ---------------------------------------------------------------------------- vof2d/curvature.py, the options
def test_derive_and_the_csv_line():
    from vof2d import _abi, curvature
    assert curvature.NAMES[_abi.VOF_CURV_KAPPA_CSF] == "KAPPA_CSF" and len(curvature.NAMES) == _abi.VOF_CURV_N == 8
    assert curvature.SUMMARY.index("ISTEP") == _abi.VOF_CURV_SUM_ISTEP and _abi.VOF_CURV_SUM_N == 16
    raw = [0.0] * 16
    for name, x in dict(ROWS=10, DEGENERATE=1, VALID=8, SUM_K=-16.0, SUM_K2=40.0, MIN_K=-3.0, MAX_K=-1.0, SUM_CSF=-30.0, SUM_CSF2=160.0, MIN_CSF=-9.0,
                        MAX_CSF=2.0, ISTEP=25).items():
        raw[curvature.SUMMARY.index(name)] = float(x)
    s = curvature.summary_of(raw)
    assert s["ROWS"] == 10 and isinstance(s["ROWS"], int) and s["ISTEP"] == 25 and curvature.summary_of(s) is s
    d = curvature.derive(raw)
    assert d["valid_share"] == 0.8 and d["k_mean"] == -2.0 and d["k_rms"] == math.sqrt(5.0) and (d["k_min"], d["k_max"]) == (-3.0, -1.0)
    assert d["csf_mean"] == -3.0 and d["csf_rms"] == 4.0 and (d["csf_min"], d["csf_max"]) == (-9.0, 2.0)
    line = curvature.csv_line(raw).split(",")
    assert len(line) == len(curvature.CSV_HEADER.split(",")) == 13 and line[:5] == ["25", "10", "1", "8", "0.8"] and float(line[5]) == -2.0
    empty = curvature.derive([0.0] * 5 + [math.inf, -math.inf, 0.0, 0.0, math.inf, -math.inf] + [0.0] * 5)
    assert empty["rows"] == 0 and all(math.isnan(empty[k]) for k in ("valid_share", "k_mean", "k_min", "csf_rms", "csf_max"))
    with pytest.raises(ValueError):
        curvature.summary_of([0.0] * 4)


def test_the_option():
    from vof2d import cli, recorders
    assert cli.parse_args([]).curvature_every is None                            # off by default
    args = cli.parse_args(["--curvature-every", "5"])
    assert args.curvature_every == 5
    for bad in (["--curvature-every", "0"], ["--curvature-every", "5", "--gpus", "2"]):
        with pytest.raises(SystemExit):
            cli.parse_args(bad)

    class Drv:
        diag_every, diag_in_advance = 0, False
    kinds = lambda a, world: [type(r).__name__ for r in recorders.recorders_of(a, Drv(), world)]
    assert "Curvature" in kinds(args, 1) and "Curvature" not in kinds(args, 2) and "Curvature" not in kinds(cli.parse_args([]), 1)


def test_the_kernel_header_stands_alone(tmp_path):
    import test_kernel_headers as tkh
    if tkh.HIPCC is None:
        pytest.skip("hipcc is not installed")
    tkh.test_header_compiles_alone(tmp_path, "curvature.h")
    assert {"cells.h", "cell_rows.h"} <= set(tkh.includes("curvature.h"))      # mul_rounded and the reduction; the count, scan and emit passes


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")], ids=["plain", "asan-ubsan"])
def test_the_arena_layout(tmp_path, flags):
    """carve_cell_rows of runtime/carve.h is plain C++: tests/host/curv_carve_check.cpp, compiled with the host compiler and run stand-alone."""
    import os
    import subprocess
    from test_rows_geometry import CSRC, ROOT, host_compiler
    exe = str(tmp_path / "curv_carve_check")
    subprocess.run([host_compiler(), "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "host", "curv_carve_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
