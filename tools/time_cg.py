#!/usr/bin/env python3
"""Time the two converged pressure solves on one GPU, on the same state and to the same relative tolerance:

  (a) vof_solve_p     -- Jacobi sweeps, exactly as `bench.py --full` -> residual_solve_1024 calls it
  (b) vof_solve_p_cg  -- conjugate gradients on the same equation

first pressure solve of a dam-break run (p = 0), fp64 unless --dtype f32, three warm repetitions each.  Prints
iterations, seconds, microseconds per iteration, and what the two end states look like to the other solver's measure.

    python tools/time_cg.py                         # 1024^2, tol 1e-6
    python tools/time_cg.py --n 4096 --jacobi-seconds 60   # Jacobi is given up after that long (its sweeps are capped)
    python tools/time_cg.py --trace                 # CG only, few iterations: for a kernel-trace run (see below)

Array passes per iteration: run the --trace form under the profiler in a run of its own,
    rocprofv3 --kernel-trace --stats -d OUT -- python tools/time_cg.py --trace --n 1024
and divide each kernel's average time by the time one pass over an array takes (n * n * 8 bytes at the bandwidth the
copy-like k_cg_update reaches); by construction an iteration moves r, s (read) + s', q (write) in k_cg_apply and
p, s, r, q (read) + p, r (write) in k_cg_update: ten passes, against 0.3 per sweep of the fused Jacobi kernels.
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
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--every", type=int, default=5000, help="sweeps between checks of the Jacobi solve (bench.py: 5000)")
    ap.add_argument("--cg-every", type=int, default=50, help="iterations between checks of the CG solve")
    ap.add_argument("--jacobi-seconds", type=float, default=0.0,
                    help="> 0: cap the Jacobi solve at the sweeps that fit this many seconds (from a short timing), and say so")
    ap.add_argument("--no-jacobi", action="store_true")
    ap.add_argument("--trace", action="store_true", help="CG only: 200 iterations on a warm handle, nothing else (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    import numpy as np
    from vof2d._lib import hip_api
    import _cg_np as cgnp
    api = hip_api()
    n = a.n
    if a.trace:
        e = fresh(api, n, a.dtype, a.device)
        e.solve_p_cg(1e-30, 200, 100, "rel")
        e.sync()
        e.close()
        print("traced: 200 iterations of vof_solve_p_cg at %d^2 %s" % (n, a.dtype))
        return 0
    print("# %d x %d %s dam-break, pressure solve of step 1 from p = 0, relative tolerance %g" % (n, n, a.dtype, a.tol))
    cg_state = None
    for rep in range(a.reps):
        e = fresh(api, n, a.dtype, a.device)
        e.solve_p_cg(1e-30, 10, 10, "rel")          # (warm the kernels and allocate the work arrays)
        e.set("p", np.zeros((n + 2, n + 2), dtype=e.np_dtype))
        e.sync()
        t0 = time.perf_counter()
        it, res, drift = e.solve_p_cg(a.tol, 10 * n, a.cg_every, "rel")
        dt = time.perf_counter() - t0
        print("cg     rep %d: %7d iterations  %9.4f s  %8.2f us/iteration  residual %.3e  drift %.6e  converged %s" %
              (rep, it, dt, 1e6 * dt / max(it, 1), res, drift, res <= a.tol), flush=True)
        if rep == a.reps - 1:
            upd, pmax = e.jacobi_sweeps_norms(1, build_rhs=False)
            print("cg     end state by the sweeps' measure: max|p_new - p| / max|p_new| = %.3e  (the drift alone is %.3e)" %
                  (upd / pmax, abs(drift) / pmax), flush=True)
        e.close()
    if a.no_jacobi:
        return 0
    cap = 3000000
    if a.jacobi_seconds > 0:
        e = fresh(api, n, a.dtype, a.device)
        e.solve_p_jacobi(10)
        e.sync()
        t0 = time.perf_counter()
        e.solve_p(1e-30, 2000, 1000, "rel")
        per = (time.perf_counter() - t0) / 2000
        cap = max(a.every, int(a.jacobi_seconds / per / a.every) * a.every)
        print("jacobi: %.2f us/sweep in a short run; capped at %d sweeps (about %.0f s)" % (1e6 * per, cap, cap * per), flush=True)
        e.close()
    for rep in range(a.reps):
        e = fresh(api, n, a.dtype, a.device)
        e.solve_p_jacobi(10)                        # (warm the kernels; 10 sweeps of the solve -- as bench.py does)
        e.sync()
        t0 = time.perf_counter()
        it, res = e.solve_p(a.tol, cap, a.every, "rel")
        dt = time.perf_counter() - t0
        print("jacobi rep %d: %7d sweeps      %9.4f s  %8.2f us/sweep      residual %.3e  converged %s" %
              (rep, it + 10, dt, 1e6 * dt / max(it, 1), res, res <= a.tol), flush=True)
        if rep == a.reps - 1:
            p, rhs = e.get("p"), e.get("rhs")
            mz, mp, c = cgnp.z_of(p, rhs, e.get_param("dxi2"), e.get_param("dyi2"))
            print("jacobi end state by the CG measure: max|z| / max|p| = %.3e" % (mz / mp), flush=True)
        e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
