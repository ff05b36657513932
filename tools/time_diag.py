#!/usr/bin/env python3
"""Time vof_diagnostics and vof_step_diag: -ic 1, 1024^2 and 4096^2, fp64 and fp32 (one process, one handle per case).

    python tools/time_diag.py
    python tools/time_diag.py --n 4096 --dtype f64 --steps 400

  diagnostics   us per vof_diagnostics call, one device event pair around `--calls` back-to-back calls on settled ghost
                cells: k_diag + k_diag_finish, and the verb's 128-byte read-back and synchronise (the verb waits; the
                recording path of vof_step_diag does not: its cost per row is the last column of the step_diag lines)
  step          ms per step of vof_step(steps): the parent commit's form
  step_diag     ms per step of vof_step_diag(steps, every) at every = 1, 10, 100, on the same box in the same process,
                alternating with `step`, `--reps` times each; the median and the spread are printed

Wall clock around work that ends in a device synchronise for the steps; device events (vof_timer_start / _stop) for the
diagnostics.  No threshold: the numbers go to profiles/diag.md.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))


def fresh(api, n, dtype, device, warm):
    from vof2d.engine import Engine, make_desc
    e = Engine(api, make_desc(api, n, n, dtype, "f32", device=device))
    e.set_init_F(1)
    e.step(warm)
    e.sync()
    return e


def wall(fn, e):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--dtype", nargs="+", default=["f64", "f32"])
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--every", type=int, nargs="+", default=[1, 10, 100])
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d._lib import hip_api
    from vof2d import diag
    api = hip_api()
    S = a.steps
    for n in a.n:
        for dtype in a.dtype:
            e = fresh(api, n, dtype, a.device, a.warm)
            esz = 8 if dtype == "f64" else 4
            mb = 3.0 * (n + 2) * (n + 2) * esz / 1e6
            print("# %d x %d %s dam-break, %d warm steps; F, u, v are %.0f MB" % (n, n, dtype, a.warm, mb), flush=True)
            raw = e.diagnostics()                      # settles the ghost cells, allocates the buffers
            d = diag.derive(raw, e.get_param("dx"), e.get_param("dy"), e.get_param("dt"), n, n)
            print("  step %d: volume %.6e xc %.5f yc %.5f div_max %.3e cfl %.3e F in [%.3e, %.6f]" % (
                raw["ISTEP"], d["volume"], d["xc"], d["yc"], d["div_max"], d["cfl"], d["F_min"], d["F_max"]), flush=True)
            us = []
            for _ in range(a.reps):
                e.timer_start()
                for _ in range(a.calls):
                    e.diagnostics()
                us.append(1e3 * e.timer_stop() / a.calls)
            print("  diagnostics, enqueue + read-back   %9.2f us per call  (%.2f .. %.2f), %d calls per event pair; the 3 arrays in that time: %.2f TB/s" % (
                statistics.median(us), min(us), max(us), a.calls, mb / statistics.median(us)), flush=True)   # MB per us = TB/s
            # alternating, on the same handle: what a row costs where nothing waits is step_diag minus step
            base, rec = [], {k: [] for k in a.every}
            for _ in range(a.reps):
                base.append(1e3 * wall(lambda: e.step(S), e) / S)
                for k in a.every:
                    rec[k].append(1e3 * wall(lambda: e.step_diag(S, k), e) / S)
            b = statistics.median(base)
            print("  step                               %9.4f ms per step  (%.4f .. %.4f)" % (b, min(base), max(base)), flush=True)
            for k in a.every:
                m = statistics.median(rec[k])
                print("  step_diag every = %-4d             %9.4f ms per step  (%.4f .. %.4f)  %+.1f %%, %+.1f us per row" % (
                    k, m, min(rec[k]), max(rec[k]), 100.0 * (m / b - 1.0), 1e3 * (m - b) * k), flush=True)
            e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
