#!/usr/bin/env python3
"""Time the three converged pressure solves on one GPU, in one process, on the same state and to the same relative
tolerance: first pressure solve of a dam-break run (p = 0), fp64 unless --dtype f32, warm repetitions.

  (a) vof_solve_p_mg  -- geometric multigrid, a check after every V-cycle
  (b) vof_solve_p_cg  -- conjugate gradients, a check every 50 iterations
  (c) vof_solve_p     -- Jacobi sweeps as `bench.py --full` -> residual_solve_1024 calls it (a check every 5000)

    python tools/time_mg.py --n 1024 --tol 1e-6 1e-8
    python tools/time_mg.py --n 4096 --tol 1e-6 1e-8 --jacobi-seconds 8    # the sweeps are given up after that long
    python tools/time_mg.py --n 1024 --no-graph                           # mg launches every kernel itself (knob mg_graph = 0)

Kernel times per level: the --trace form (mg only, 20 cycles on a warm handle) under the profiler, in a run of its own,
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/time_mg.py --trace --n 1024
The levels of one kernel differ in their grid size (the trace's Grid_Size column), so the trace splits by level.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fresh(api, n, dtype, device):
    from vof2d.engine import Engine, make_desc
    e = Engine(api, make_desc(api, n, n, dtype, "f32", device=device))
    e.set_init_F(1)
    e.cal_nu_rho(); e.get_normal_young(); e.advect_upwind(); e.set_BC()    # :513-518 of step 1
    return e


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--tol", type=float, nargs="+", default=[1e-6])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--jacobi-seconds", type=float, default=0.0, help="> 0: cap the Jacobi solve at the sweeps that fit this many seconds")
    ap.add_argument("--no-jacobi", action="store_true")
    ap.add_argument("--no-cg", action="store_true")
    ap.add_argument("--no-graph", action="store_true", help="mg: knob mg_graph = 0")
    ap.add_argument("--trace", action="store_true", help="mg only: 20 cycles on a warm handle, nothing else")
    a = ap.parse_args()
    import numpy as np
    from vof2d._lib import hip_api
    api = hip_api()
    n = a.n
    zero = lambda e: e.set("p", np.zeros((n + 2, n + 2), dtype=e.np_dtype))
    if a.trace:
        e = fresh(api, n, a.dtype, a.device)
        e.solve_p_mg(1e-30, 2, 2, "rel")
        e.sync()
        e.solve_p_mg(1e-30, 20, 20, "rel")
        e.sync()
        e.close()
        print("traced: 2 + 20 cycles of vof_solve_p_mg at %d^2 %s" % (n, a.dtype))
        return 0
    for tol in a.tol:
        print("# %d x %d %s dam-break, pressure solve of step 1 from p = 0, relative tolerance %g" % (n, n, a.dtype, tol), flush=True)
        for rep in range(a.reps):
            e = fresh(api, n, a.dtype, a.device)
            if a.no_graph:
                e.set_param("mg_graph", 0)
            e.solve_p_mg(1e-30, 1, 1, "rel")          # (warm the kernels, allocate the levels, capture the cycle)
            zero(e)
            e.sync()
            t0 = time.perf_counter()
            it, res, drift = e.solve_p_mg(tol, 40, 1, "rel")
            dt = time.perf_counter() - t0
            print("mg     rep %d: %7d cycles      %9.4f s  %8.2f us/cycle      residual %.3e  drift %.6e  converged %s" %
                  (rep, it, dt, 1e6 * dt / max(it, 1), res, drift, res <= tol), flush=True)
            e.close()
        for rep in range(0 if a.no_cg else a.reps):
            e = fresh(api, n, a.dtype, a.device)
            e.solve_p_cg(1e-30, 10, 10, "rel")
            zero(e)
            e.sync()
            t0 = time.perf_counter()
            it, res, drift = e.solve_p_cg(tol, 10 * n, 50, "rel")
            dt = time.perf_counter() - t0
            print("cg     rep %d: %7d iterations  %9.4f s  %8.2f us/iteration  residual %.3e  drift %.6e  converged %s" %
                  (rep, it, dt, 1e6 * dt / max(it, 1), res, drift, res <= tol), flush=True)
            e.close()
        if a.no_jacobi:
            continue
        cap = 3000000
        if a.jacobi_seconds > 0:
            e = fresh(api, n, a.dtype, a.device)
            e.solve_p_jacobi(10)
            e.sync()
            t0 = time.perf_counter()
            e.solve_p(1e-30, 2000, 1000, "rel")
            per = (time.perf_counter() - t0) / 2000
            cap = max(5000, int(a.jacobi_seconds / per / 5000) * 5000)
            print("jacobi: %.2f us/sweep in a short run; capped at %d sweeps (about %.0f s)" % (1e6 * per, cap, cap * per), flush=True)
            e.close()
        for rep in range(a.reps):
            e = fresh(api, n, a.dtype, a.device)
            e.solve_p_jacobi(10)
            e.sync()
            t0 = time.perf_counter()
            it, res = e.solve_p(tol, cap, 5000, "rel")
            dt = time.perf_counter() - t0
            print("jacobi rep %d: %7d sweeps      %9.4f s  %8.2f us/sweep      residual %.3e  converged %s" %
                  (rep, it + 10, dt, 1e6 * dt / max(it, 1), res, res <= tol), flush=True)
            e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
