#!/usr/bin/env python3
"""Time vof_tracers_advance and vof_step_tracers: -ic 1, 4096^2 fp64 (one process, one handle).

    python tools/time_tracers.py
    python tools/time_tracers.py --n 2048 --dtype f32 --steps 512 --tracers 10000 1000000

  advance       us per vof_tracers_advance call for each tracer count, one device event pair around `--calls` back-to-back
                calls on settled ghost cells (k_tracer_advance alone: the verb enqueues only)
  step          ms per step of vof_step(steps): the parent commit's form
  step_tracers  ms per step of vof_step_tracers(steps, every) at every = 1, 8, 32 with `--step-tracers` tracers, on the
                same handle in the same process, alternating with `step`, `--reps` times each; the median and the spread
                are printed, and the counters tm_steps and tm_chained_batches of every leg (the form and the batches of
                the steps: an advance ends a chain of k_tm batches, vof_step alone does not)

Wall clock around work that ends in a device synchronise for the steps; device events (vof_timer_start / _stop) for the
advances.  No threshold: the numbers go to profiles/tracers.md.
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
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--steps", type=int, default=1024)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tracers", type=int, nargs="+", default=[10 ** 4, 10 ** 5, 10 ** 6])
    ap.add_argument("--step-tracers", type=int, default=10 ** 5)
    ap.add_argument("--every", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d import tracers
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    n, S = a.n, a.steps
    e = Engine(api, make_desc(api, n, n, a.dtype, "f32", device=a.device))
    e.set_init_F(1)
    e.step(a.warm)
    e.sync()
    dt = e.get_param("dt")
    print("# %d x %d %s dam-break, %d warm steps" % (n, n, a.dtype, a.warm), flush=True)
    for want in a.tracers:
        count = len(tracers.seed(e, want, "all"))
        e.tracers_advance(dt)                          # settles the ghost cells; the first launch loads the code object
        e.sync()
        us = []
        for _ in range(a.reps):
            e.timer_start()
            for _ in range(a.calls):
                e.tracers_advance(dt)
            us.append(1e3 * e.timer_stop() / a.calls)
        m = statistics.median(us)
        _, summ = e.tracers(rows=False)
        print("  advance, %8d tracers   %9.2f us per call  (%.2f .. %.2f), %d calls per event pair; %.2f ns per tracer; lost %d, in liquid %d" % (
            count, m, min(us), max(us), a.calls, 1e3 * m / count, summ["LOST"], summ["IN_LIQUID"]), flush=True)

    def counters():
        return e.get_counter("tm_steps"), e.get_counter("tm_chained_batches")

    def leg(fn):
        c0 = counters()
        ms = 1e3 * wall(fn, e) / S
        c1 = counters()
        return ms, (c1[0] - c0[0], c1[1] - c0[1])

    count = len(tracers.seed(e, a.step_tracers, "all"))
    base, rec, forms = [], {k: [] for k in a.every}, {}
    for _ in range(a.reps):
        ms, forms["step"] = leg(lambda: e.step(S))
        base.append(ms)
        for k in a.every:
            ms, forms[k] = leg(lambda: e.step_tracers(S, k))
            rec[k].append(ms)
    b = statistics.median(base)
    print("  %d steps per leg, %d tracers" % (S, count), flush=True)
    print("  step                               %9.4f ms per step  (%.4f .. %.4f)  tm_steps %d, tm_chained_batches %d" % (
        (b, min(base), max(base)) + forms["step"]), flush=True)
    for k in a.every:
        m = statistics.median(rec[k])
        print("  step_tracers every = %-4d          %9.4f ms per step  (%.4f .. %.4f)  %+.1f %%, %+.1f us per advance  tm_steps %d, tm_chained_batches %d" % (
            (k, m, min(rec[k]), max(rec[k]), 100.0 * (m / b - 1.0), 1e3 * (m - b) * k) + forms[k]), flush=True)
    e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
