"""The conjugate-gradient pressure solve (vof_solve_p_cg), CPU part: the NumPy restatement of the method
(tests/_cg_np.py) judged by the ORACLE's Jacobi sweep, the argument checks of the HIP library that need no GPU, and
the command line.

What "converged" means here is pinned to the existing iteration, not to the restatement itself: from the p the
restatement returns, one oracle sweep must change every interior cell by the same constant, the drift
c = sum(b) / sum(ap).  With |z| <= tol * max|p| in every cell (z = what the sweep changes beyond c) the changes lie in
[c - tol max|p|, c + tol max|p|]: their spread is at most 2 tol max|p| and their plain mean lies within tol max|p| of c
(measured: within 3e-4 of that).  The mean weighted with ap is sharper: sum(ap (p_new - p)) = sum(b - L p) = sum(b) for
ANY p, because the columns of the symmetric L sum to zero, so it equals c up to rounding alone.
"""
import ctypes as C

import numpy as np
import pytest

import _cg_np as cg
from test_residual_solve import predictor_state
from util import engine
from vof2d import _abi


def oracle_problem(api, nx, ny, dtype, ic, steps, **kw):
    """(engine, p, rhs) where the pressure solve of a step is about to run: rhs as the oracle builds it."""
    e = predictor_state(engine(api, nx, ny, dtype, "f32", ic=ic, **kw), steps)
    p0 = e.get("p")
    e.jacobi_sweeps_norms(1, build_rhs=True)      # (builds rhs, then sweeps once: p is put back)
    rhs = e.get("rhs")
    e.set("p", p0)
    return e, p0, rhs


def sweep_judgement(e, p, rhs, tol_abs, drift, ctx=""):
    """One Jacobi sweep of engine e (rhs as it stands) from p changes p by the constant `drift`."""
    e.set("p", p)
    e.jacobi_sweeps_norms(1, build_rhs=False)
    p_new = e.get("p")
    e.set("p", p)
    spread, mean = cg.sweep_change(p_new, p)
    allow = cg.allowance(p)
    co = cg.coefficients(p.shape[0] - 2, p.shape[1] - 2, e.get_param("dxi2"), e.get_param("dyi2"), p.dtype)
    ap = co[4].astype(np.float64)
    d = p_new[1:-1, 1:-1].astype(np.float64) - p[1:-1, 1:-1].astype(np.float64)
    wmean = float(np.sum(ap * d) / np.sum(ap))
    print("%s spread %.3e (bound %.3e) |mean - c| %.3e (bound %.3e) |weighted mean - c| %.3e (bound %.3e)" %
          (ctx, spread, 2 * tol_abs + allow, abs(mean - drift), tol_abs + allow, abs(wmean - drift), allow))
    assert spread <= 2 * tol_abs + allow, ctx
    assert abs(mean - drift) <= tol_abs + allow, ctx
    assert abs(wmean - drift) <= allow, ctx


@pytest.mark.parametrize("nx,ny,ic,steps", [(48, 40, 1, 0), (48, 40, 3, 0), (64, 64, 1, 3), (64, 64, 3, 3)])
def test_restatement_converges_to_what_the_sweeps_tend_to(oracle_api, nx, ny, ic, steps):
    e, p0, rhs = oracle_problem(oracle_api, nx, ny, "f64", ic, steps)
    cx, cy = e.get_param("dxi2"), e.get_param("dyi2")
    tol = 1e-8
    p, it, res, c = cg.cg_solve(p0, rhs, cx, cy, tol, 10 * max(nx, ny), 10, "rel")
    assert res <= tol and it < 10 * max(nx, ny) and it % 10 == 0
    e.set("p", p)
    e.jacobi_sweeps_norms(1, build_rhs=False)
    assert np.array_equal(cg.jacobi_update(p, rhs, cx, cy)[1:-1, 1:-1], e.get("p")[1:-1, 1:-1])   # jacobi_update IS the oracle's sweep
    maxp = float(np.abs(p[1:-1, 1:-1]).max())
    sweep_judgement(e, p, rhs, tol * maxp, c, "%dx%d ic %d" % (nx, ny, ic))
    mz, mp, c2 = cg.z_of(p, rhs, cx, cy)          # the literal form of L agrees with what the solve reported
    assert c2 == c and abs(mz - res * mp) <= cg.allowance(p)


def test_restatement_first_check_and_cap(oracle_api):
    e, p0, rhs = oracle_problem(oracle_api, 48, 40, "f64", 1, 0)
    cx, cy = e.get_param("dxi2"), e.get_param("dyi2")
    p, it, res, c = cg.cg_solve(p0, rhs, cx, cy, 1e-30, 95, 30, "abs")
    assert it == 95 and res > 1e-30
    p, it, res, c = cg.cg_solve(p0, rhs, cx, cy, 1e-8, 1000, 10, "rel")
    p2, it2, res2, c2 = cg.cg_solve(p, rhs, cx, cy, 1e-8, 1000, 10, "rel")
    assert it2 == 0 and res2 == res and c2 == c and np.array_equal(p2, p)
    bad = p0.copy()
    bad[10, 10] = np.nan
    assert cg.cg_solve(bad, rhs, cx, cy, 1e-8, 1000, 10, "rel")[1:3] == (0, float("inf"))


def test_bad_arguments_are_rejected_without_a_gpu(hip_api):
    it, res, drift = C.c_int32(), C.c_double(), C.c_double()
    ok = (C.byref(it), C.byref(res), C.byref(drift))
    assert hip_api.solve_p_cg(None, 1e-8, 100, 10, _abi.VOF_RESID_ABS, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_cg(None, 1e-8, 0, 10, _abi.VOF_RESID_ABS, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_cg(None, 1e-8, 100, 0, _abi.VOF_RESID_REL, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_cg(None, 1e-8, 100, 10, 7, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_cg(None, 1e-8, 100, 10, _abi.VOF_RESID_ABS, 1, None, None, None) == _abi.VOF_EINVAL
    assert "solve_p_cg" in _abi.GPU_ONLY and "solve_p_cg" in _abi.SIGNATURES


def test_oracle_binds_without_the_verb(oracle_api):
    assert not hasattr(oracle_api, "solve_p_cg") and hasattr(oracle_api, "solve_p")


def test_command_line_flag_and_refusals(capsys):
    from vof2d import cli
    a = cli.parse_args([])
    assert a.pressure_solver == "jacobi"
    assert cli.numerics_of(a, 4e-6) == {"dt": 4e-6, "jacobi_iters": 10, "coord_cast": "f32", "jacobi_tol": 0.0,
                                         "jacobi_max": 0, "jacobi_crit": ""}
    a = cli.parse_args(["--pressure-solver", "cg", "--jacobi-tol", "1e-8", "--jacobi-crit", "rel", "--jacobi-max", "5000"])
    num = cli.numerics_of(a, 4e-6)
    assert num["pressure_solver"] == "cg" and num["jacobi_tol"] == 1e-8 and num["jacobi_max"] == 5000 and num["jacobi_crit"] == "rel"
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--pressure-solver", "cg"])
    assert e.value.code == 2 and "--jacobi-tol" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--pressure-solver", "cg", "--jacobi-tol", "1e-8", "--gpus", "2"])
    assert e.value.code == 2 and "one GPU" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.parse_args(["--pressure-solver", "multigrid", "--jacobi-tol", "1e-8"])
    with pytest.raises(SystemExit):       # and before any engine is made when a launcher calls run() itself
        cli.run(cli.build_parser().parse_args(["--gpus", "2", "--pressure-solver", "cg", "--jacobi-tol", "1e-8"]),
                api=object(), rank=0, world=2)


def test_a_checkpoint_of_a_cg_run_is_not_continued_with_sweeps(tmp_path):
    from vof2d import cli
    f = {k: np.zeros((6, 6)) for k in ("F", "u", "v", "p")}
    cgargs = cli.parse_args(["--pressure-solver", "cg", "--jacobi-tol", "1e-8"])
    swargs = cli.parse_args(["--jacobi-tol", "1e-8"])
    ck = str(tmp_path / "a.npz")
    cli.save_state(ck, f, 5, 4, 4, "f64", 1, 0, cli.numerics_of(cgargs, 4e-6))
    assert cli.load_state(ck, 4, 4, "f64", cli.numerics_of(cgargs, 4e-6))[1] == 5
    ck2 = str(tmp_path / "b.npz")
    cli.save_state(ck2, f, 5, 4, 4, "f64", 1, 0, cli.numerics_of(swargs, 4e-6))
    assert cli.load_state(ck2, 4, 4, "f64", cli.numerics_of(swargs, 4e-6))[1] == 5      # as before
    with pytest.raises(SystemExit) as e:
        cli.load_state(ck2, 4, 4, "f64", cli.numerics_of(cgargs, 4e-6))
    assert "pressure-solver" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.load_state(ck, 4, 4, "f64", cli.numerics_of(swargs, 4e-6))
    assert "pressure-solver" in str(e.value)
