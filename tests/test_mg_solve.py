"""The geometric-multigrid pressure solve (vof_solve_p_mg), CPU part: the NumPy restatement of the method
(tests/_mg_np.py) on ORACLE right-hand sides, judged as tests/test_cg_solve.py judges conjugate gradients (one oracle
sweep from the result changes every cell by the drift c), the cycle cap, the argument checks of the HIP library that need
no GPU, and the command line.

The cap of 40 cycles is the GPU tests' (tests/test_mg_solve_gpu.py): a condition.  The grids are the GPU tests' too.
"""
import ctypes as C

import numpy as np
import pytest

import _cg_np as cg
import _mg_np as mg
from test_cg_solve import oracle_problem, sweep_judgement
from vof2d import _abi

CAP = 40
GRIDS = [(64, 64, "f64", 1, {}), (64, 64, "f64", 2, {}), (64, 64, "f64", 3, {}),
         (96, 130, "f64", 1, {}), (96, 130, "f64", 2, {}), (96, 130, "f64", 3, {}),
         (256, 256, "f64", 1, {}), (256, 256, "f64", 2, {}), (256, 256, "f64", 3, {}),
         (80, 50, "f64", 3, {"Lx": 0.1, "Ly": 0.13}), (128, 128, "f32", 1, {}),
         (200, 200, "f64", 1, {}), (48, 80, "f64", 2, {})]


def test_hierarchy_rule():
    assert mg.hierarchy(1024, 1024)[-1] == (4, 4) and len(mg.hierarchy(1024, 1024)) == 9
    assert mg.hierarchy(200, 200) == [(200, 200), (100, 100), (50, 50), (25, 25)]
    assert mg.hierarchy(96, 130) == [(96, 130), (48, 65)]          # an odd factor: shallow, a large coarsest level
    assert mg.hierarchy(48, 80)[-1] == (6, 10) and mg.hierarchy(6, 64) == [(6, 64)]
    assert mg.hierarchy(256, 256, 2) == [(256, 256), (128, 128)] and mg.hierarchy(256, 256, 1) == [(256, 256)]


@pytest.mark.parametrize("steps", [3, 0])
@pytest.mark.parametrize("nx,ny,dtype,ic,kw", GRIDS)
def test_restatement_converges_within_the_cap(oracle_api, nx, ny, dtype, ic, kw, steps):
    e, p0, rhs = oracle_problem(oracle_api, nx, ny, dtype, ic, steps, **kw)
    cx, cy = e.get_param("dxi2"), e.get_param("dyi2")
    tol = 1e-8 if dtype == "f64" else 1e-5
    hist = []
    p, it, res, c = mg.mg_solve(p0, rhs, cx, cy, tol, CAP, 1, "rel", history=hist)
    sizes = mg.hierarchy(nx, ny)
    print("%dx%d %s ic %d steps %d: levels %d coarsest %dx%d cycles %d worst factor %.2f" %
          (nx, ny, dtype, ic, steps, len(sizes), sizes[-1][0], sizes[-1][1], it, mg.worst_factor(hist)))
    assert res <= tol and 0 < it <= 20 < CAP          # (20: beyond it a grid would leave the list, tests/test_mg_solve_gpu.py)
    maxp = float(np.abs(p[1:-1, 1:-1]).max())
    sweep_judgement(e, p, rhs, tol * maxp, c, "%dx%d ic %d" % (nx, ny, ic))
    mz, mp, c2 = cg.z_of(p, rhs, cx, cy)              # the literal form of L agrees with what the solve reported
    assert c2 == c and abs(mz - res * mp) <= cg.allowance(p)


@pytest.mark.parametrize("nu,levels", [(1, -1), (3, -1), (2, 1), (2, 2)])
def test_restatement_sweep_counts_and_depths(oracle_api, nu, levels):
    for (nx, ny, ic) in ((96, 96, 1), (48, 80, 2)):
        e, p0, rhs = oracle_problem(oracle_api, nx, ny, "f64", ic, 3)
        cap = 10 * max(nx, ny) if levels == 1 else CAP
        p, it, res, c = mg.mg_solve(p0, rhs, e.get_param("dxi2"), e.get_param("dyi2"), 1e-8, cap, 1, "rel", nu, levels)
        assert res <= 1e-8 and 0 < it <= CAP, (nx, ny, it)
        sweep_judgement(e, p, rhs, 1e-8 * float(np.abs(p[1:-1, 1:-1]).max()), c, "%dx%d nu %d levels %d" % (nx, ny, nu, levels))


def test_restatement_first_check_and_cap(oracle_api):
    e, p0, rhs = oracle_problem(oracle_api, 48, 40, "f64", 1, 0)
    cx, cy = e.get_param("dxi2"), e.get_param("dyi2")
    p, it, res, c = mg.mg_solve(p0, rhs, cx, cy, 1e-30, 5, 2, "abs")
    assert it == 5 and res > 1e-30
    p, it, res, c = mg.mg_solve(p0, rhs, cx, cy, 1e-8, CAP, 1, "rel")
    p2, it2, res2, c2 = mg.mg_solve(p, rhs, cx, cy, 1e-8, CAP, 1, "rel")
    assert it2 == 0 and res2 == res and c2 == c and np.array_equal(p2, p)
    bad = p0.copy()
    bad[10, 10] = np.nan
    assert mg.mg_solve(bad, rhs, cx, cy, 1e-8, CAP, 1, "rel")[1:3] == (0, float("inf"))


def test_bad_arguments_are_rejected_without_a_gpu(hip_api):
    it, res, drift = C.c_int32(), C.c_double(), C.c_double()
    ok = (C.byref(it), C.byref(res), C.byref(drift))
    assert hip_api.solve_p_mg(None, 1e-8, 40, 1, _abi.VOF_RESID_ABS, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_mg(None, 1e-8, 0, 1, _abi.VOF_RESID_ABS, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_mg(None, 1e-8, 40, 0, _abi.VOF_RESID_REL, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_mg(None, 1e-8, 40, 1, 7, 1, *ok) == _abi.VOF_EINVAL
    assert hip_api.solve_p_mg(None, 1e-8, 40, 1, _abi.VOF_RESID_ABS, 1, None, None, None) == _abi.VOF_EINVAL


def test_abi_lists_the_symbol_and_the_library_exports_it(hip_api, oracle_api):
    assert "solve_p_mg" in _abi.GPU_ONLY and "solve_p_mg" in _abi.SIGNATURES
    assert _abi.SIGNATURES["solve_p_mg"] == _abi.SIGNATURES["solve_p_cg"]
    assert hasattr(hip_api.lib, "vof_solve_p_mg")
    assert not hasattr(oracle_api, "solve_p_mg") and hasattr(oracle_api, "solve_p")


def test_command_line_flag_and_refusals(capsys):
    from vof2d import cli
    a = cli.parse_args(["--pressure-solver", "mg", "--jacobi-tol", "1e-8", "--jacobi-crit", "rel", "--jacobi-max", "40"])
    num = cli.numerics_of(a, 4e-6)
    assert num["pressure_solver"] == "mg" and num["jacobi_tol"] == 1e-8 and num["jacobi_max"] == 40 and num["jacobi_crit"] == "rel"
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--pressure-solver", "mg"])
    assert e.value.code == 2 and "--jacobi-tol" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        cli.parse_args(["--pressure-solver", "mg", "--jacobi-tol", "1e-8", "--gpus", "2"])
    assert e.value.code == 2 and "one GPU" in capsys.readouterr().err
    with pytest.raises(SystemExit):       # and before any engine is made when a launcher calls run() itself
        cli.run(cli.build_parser().parse_args(["--gpus", "2", "--pressure-solver", "mg", "--jacobi-tol", "1e-8"]),
                api=object(), rank=0, world=2)


def test_checkpoints_do_not_cross_between_the_solvers(tmp_path):
    from vof2d import cli
    f = {k: np.zeros((6, 6)) for k in ("F", "u", "v", "p")}
    args = {s: cli.parse_args((["--pressure-solver", s] if s != "jacobi" else []) + ["--jacobi-tol", "1e-8"]) for s in ("jacobi", "cg", "mg")}
    for s in args:
        ck = str(tmp_path / (s + ".npz"))
        cli.save_state(ck, f, 5, 4, 4, "f64", 1, 0, cli.numerics_of(args[s], 4e-6))
        for t in args:
            if t == s:
                assert cli.load_state(ck, 4, 4, "f64", cli.numerics_of(args[t], 4e-6))[1] == 5
            else:
                with pytest.raises(SystemExit) as e:
                    cli.load_state(ck, 4, 4, "f64", cli.numerics_of(args[t], 4e-6))
                assert "pressure-solver" in str(e.value)
