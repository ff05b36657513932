#!/usr/bin/env python3
"""Time vof_stats_sample and vof_step_stats: -ic 1 (one process, one handle per grid).

    python tools/time_stats.py
    python tools/time_stats.py --grids 1024 --dtypes f64 --steps 512 --only kernel

  kernel      us per vof_stats_sample (one launch of k_stats; a hipEvent pair around `--calls` back-to-back samples, `--reps`
              times) for each mask at each grid and dtype, and the bytes per second it reaches on its algorithmic traffic of
              3 esz + 16 planes bytes a cell (F, u, v once; every plane read and written).  Beside it, from the same process: the
              single-sweep k_jacobi (knobs jacobi_tb = 1, solve_pairs = 0; vof_time_jacobi) on its 3 esz bytes a cell, and a vof_diagnostics
              call (k_diag, its finish kernel and the read-back of one row)
  step        ms per step of vof_step(steps) against vof_step_stats(steps, every) at every = 1, 8, 32 with both groups on
              the largest grid in fp64, alternating on the same handle, `--reps` times each; the median and the spread,
              the counters tm_steps and tm_chained_batches of every leg

No threshold: the numbers go to profiles/stats.md.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))


def wall(fn, e):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--dtypes", nargs="+", default=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--only", choices=["kernel", "step"], default=None)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d import stats
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    S = a.steps

    def events(e, fn, calls):
        """us per call between a hipEvent pair around `calls` back-to-back calls."""
        e.sync()
        e.timer_start()
        for _ in range(calls):
            fn()
        return 1e3 * e.timer_stop() / calls

    for n in a.grids:
        for dtype in a.dtypes:
            esz = 8 if dtype == "f64" else 4
            e = Engine(api, make_desc(api, n, n, dtype, "f32", device=a.device))
            e.set_init_F(1)
            e.step(a.warm)
            cells = float(n) * n
            print("# %d x %d %s dam-break, %d warm steps" % (n, n, dtype, a.warm), flush=True)
            if a.only != "step":
                e.set_param("solve_pairs", 0); e.set_param("jacobi_tb", 1)      # (one sweep per launch, as bench.py times it)
                e.time_jacobi(4)
                jac = statistics.median(1e3 * e.time_jacobi(20) for _ in range(a.reps))
                e.set_param("jacobi_tb", 5); e.set_param("solve_pairs", -1)
                jrate = 3 * esz * cells / (jac * 1e-6) / 1e12
                print("  k_jacobi, one sweep        %9.1f us  %6.2f TB/s on 3 x %d bytes a cell" % (jac, jrate, esz), flush=True)
                e.diagnostics()
                dg = [1e6 * wall(lambda: [e.diagnostics() for _ in range(a.calls)], e) / a.calls for _ in range(a.reps)]
                print("  vof_diagnostics call       %9.1f us  (%.1f .. %.1f)" % (statistics.median(dg), min(dg), max(dg)), flush=True)
                for mask in (3, 1, 2):
                    planes = len(stats.planes_of(mask))
                    nbytes = (3 * esz + 16 * planes) * cells
                    e.stats_begin(mask, 0.5)
                    e.stats_sample()                     # the first launch loads the code
                    us = [events(e, e.stats_sample, a.calls) for _ in range(a.reps)]
                    m = statistics.median(us)
                    rate = nbytes / (m * 1e-6) / 1e12
                    print("  k_stats mask %d             %9.1f us  (%.1f .. %.1f)  %6.2f TB/s on %d bytes a cell = %.2f of k_jacobi's rate" % (
                        mask, m, min(us), max(us), rate, 3 * esz + 16 * planes, rate / jrate), flush=True)
                    e.stats_begin(0, 0.0)
            last = n == max(a.grids) and dtype == "f64"
            if not last or a.only == "kernel":
                e.close()
                continue

            def counters():
                return e.get_counter("tm_steps"), e.get_counter("tm_chained_batches")

            def leg(fn):
                c0 = counters()
                ms = 1e3 * wall(fn, e) / S
                c1 = counters()
                return ms, (c1[0] - c0[0], c1[1] - c0[1])

            e.stats_begin(3, 0.5)
            e.step(64); e.step_stats(64, 8)              # the graphs of both legs
            base, rec, forms = [], {k: [] for k in a.every}, {}
            for _ in range(a.reps):
                ms, forms["step"] = leg(lambda: e.step(S))
                base.append(ms)
                for k in a.every:
                    ms, forms[k] = leg(lambda: e.step_stats(S, k))
                    rec[k].append(ms)
            b = statistics.median(base)
            print("  %d steps per leg, both groups" % S, flush=True)
            print("  step                               %9.4f ms per step  (%.4f .. %.4f)  tm_steps %d, tm_chained_batches %d" % (
                (b, min(base), max(base)) + forms["step"]), flush=True)
            for k in a.every:
                m = statistics.median(rec[k])
                print("  step_stats every = %-4d            %9.4f ms per step  (%.4f .. %.4f)  %+.1f %%, %+.1f us per sample  tm_steps %d, tm_chained_batches %d" % (
                    (k, m, min(rec[k]), max(rec[k]), 100.0 * (m / b - 1.0), 1e3 * (m - b) * k) + forms[k]), flush=True)
            e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
