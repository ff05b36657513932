#!/usr/bin/env python3
"""Time vof_depths and vof_step_gauges: -ic 1 (one process, one handle per grid).

    python tools/time_gauges.py
    python tools/time_gauges.py --grids 1024 --dtypes f64 --steps 512

  depths        us per vof_depths call (the pass, the fold, the summary, the copies of depth_i, depth_j, top, one wait) at each
                grid and dtype, beside vof_diagnostics on the same state (three array passes against one) and the host route
                (vof_get_field("F") and the two NumPy sums); wall clock around `--calls` calls each, `--reps` times
  step          ms per step of vof_step(steps): the parent commit's form
  step_gauges   ms per step of vof_step_gauges(steps, every) at every = 1, 8, 32 with `--gauges` gauges on the largest grid in
                fp64, on the same handle in the same process, alternating with `step` and with vof_step_diag(steps, every),
                `--reps` times each; the median and the spread are printed, and the counters tm_steps and tm_chained_batches
                of every leg

No threshold: the numbers go to profiles/gauges.md.
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
    ap.add_argument("--gauges", type=int, default=16)
    ap.add_argument("--every", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    S = a.steps

    def per_call(fn, e, calls):
        us = []
        for _ in range(a.reps):
            us.append(1e6 * wall(lambda: [fn() for _ in range(calls)], e) / calls)
        return statistics.median(us), min(us), max(us)

    def host_route(e):
        F = e.get("F")[1:-1, 1:-1].astype(np.float64)
        return F.sum(axis=1), F.sum(axis=0)

    for n in a.grids:
        for dtype in a.dtypes:
            e = Engine(api, make_desc(api, n, n, dtype, "f32", device=a.device))
            e.set_init_F(1)
            e.step(a.warm)
            e.depths(); e.diagnostics()                  # the buffers; the first launches load the code object
            print("# %d x %d %s dam-break, %d warm steps" % (n, n, dtype, a.warm), flush=True)
            for name, fn, calls in (("vof_depths", e.depths, a.calls), ("vof_diagnostics", e.diagnostics, a.calls),
                                    ("get_field(F) + NumPy", lambda: host_route(e), max(a.calls // 10, 2))):
                print("  %-22s %10.1f us per call  (%.1f .. %.1f), %d calls per leg" % ((name,) + per_call(fn, e, calls) + (calls,)), flush=True)
            last = n == max(a.grids) and dtype == "f64"
            if not last:
                e.close()
                continue

            def counters():
                return e.get_counter("tm_steps"), e.get_counter("tm_chained_batches")

            def leg(fn):
                c0 = counters()
                ms = 1e3 * wall(fn, e) / S
                c1 = counters()
                return ms, (c1[0] - c0[0], c1[1] - c0[1])

            Lx, Ly = e.get_param("Lx"), e.get_param("Ly")
            k = np.arange(a.gauges, dtype=np.float64)
            e.gauges_set(np.stack([(k + 0.5) * Lx / a.gauges, np.full(a.gauges, 0.01 * Ly)], axis=1))
            base, rec, dia, forms = [], {k: [] for k in a.every}, {k: [] for k in a.every}, {}
            for _ in range(a.reps):
                ms, forms["step"] = leg(lambda: e.step(S))
                base.append(ms)
                for k in a.every:
                    ms, forms["g", k] = leg(lambda: e.step_gauges(S, k))
                    rec[k].append(ms)
                    ms, forms["d", k] = leg(lambda: e.step_diag(S, k))
                    dia[k].append(ms)
            b = statistics.median(base)
            print("  %d steps per leg, %d gauges" % (S, a.gauges), flush=True)
            print("  step                               %9.4f ms per step  (%.4f .. %.4f)  tm_steps %d, tm_chained_batches %d" % (
                (b, min(base), max(base)) + forms["step"]), flush=True)
            for what, times, key in (("step_gauges", rec, "g"), ("step_diag  ", dia, "d")):
                for k in a.every:
                    m = statistics.median(times[k])
                    print("  %s every = %-4d           %9.4f ms per step  (%.4f .. %.4f)  %+.1f %%, %+.1f us per record  tm_steps %d, tm_chained_batches %d" % (
                        (what, k, m, min(times[k]), max(times[k]), 100.0 * (m / b - 1.0), 1e3 * (m - b) * k) + forms[key, k]), flush=True)
            e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
