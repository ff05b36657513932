#!/usr/bin/env python3
"""Time vof_energy beside vof_diagnostics, and what --energy-every costs a run (one process, one handle per case).

    python tools/time_energy.py
    python tools/time_energy.py --n 4096 --dtype f64 --case 1:1000 2:1000 --calls 20
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 tools/time_energy.py ...   (then tools/kernel_times.py on
                                                                                                       the kernel_stats.csv: k_energy, k_diag)

  --case IC:STEPS   the state: -ic IC after STEPS steps (default: the dam break at step 1000, the rising bubble at step 1000)
  energy, diagnostics   us per call, one device event pair around `--calls` back-to-back calls on settled ghost cells: the pass, the
                one-block finish, and the verb's 128-byte read-back and synchronise
  step          ms per step of vof_step(--steps)
  energy every  ms per step of the loop the command line runs with --energy-every N: vof_step(N), vof_energy, --steps / N times; on
                the same box in the same process, alternating with `step`, `--reps` times each; the median and the spread are printed
  step_energy   the same rows recorded on the device (vof_step_energy): nothing waits before the end

Wall clock around work that ends in a device synchronise for the steps; device events (vof_timer_start / _stop) for the verbs.
No threshold: the numbers go to profiles/energy.md.
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
    ap.add_argument("--n", type=int, nargs="+", default=[4096])
    ap.add_argument("--dtype", nargs="+", default=["f64"])
    ap.add_argument("--case", nargs="+", default=["1:1000", "2:1000"])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d import energy
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    S, N = a.steps, a.every
    for n in a.n:
        for dtype in a.dtype:
            for case in a.case:
                ic, warm = (int(x) for x in case.split(":"))
                e = Engine(api, make_desc(api, n, n, dtype, "f32", device=a.device))
                e.set_init_F(ic)
                e.step(warm)
                e.sync()
                mb = 4.0 * (n + 2) * (n + 2) * (8 if dtype == "f64" else 4) / 1e6
                print("# %d x %d %s -ic %d at step %d; F, u, v, p are %.0f MB" % (n, n, dtype, ic, warm, mb), flush=True)
                raw = e.energy()                           # settles the ghost cells, allocates the buffers
                e.diagnostics()
                seg = e.interface()[1]["SEGMENTS"]
                d = energy.derive(raw, e.get_param("dx"), e.get_param("dy"), e.get_param("gx"), e.get_param("gy"), e.get_param("sigma"))
                print("  mixed cells with an orientation: %d (%.3f %% of the cells)" % (seg, 100.0 * seg / (n * n)))
                print("  " + " ".join("%s %.6e" % (k, d[k]) for k in energy.DERIVED), flush=True)
                for name, call in (("energy", e.energy), ("diagnostics", e.diagnostics)):
                    us = []
                    for _ in range(a.reps):
                        e.timer_start()
                        for _ in range(a.calls):
                            call()
                        us.append(1e3 * e.timer_stop() / a.calls)
                    print("  %-12s enqueue + read-back  %9.2f us per call  (%.2f .. %.2f), %d calls per event pair" % (
                        name, statistics.median(us), min(us), max(us), a.calls), flush=True)

                def with_energy():
                    for _ in range(S // N):
                        e.step(N)
                        e.energy()
                base, loop, rec = [], [], []
                for _ in range(a.reps):
                    base.append(1e3 * wall(lambda: e.step(S), e) / S)
                    loop.append(1e3 * wall(with_energy, e) / S)
                    rec.append(1e3 * wall(lambda: e.step_energy(S, N), e) / S)
                b = statistics.median(base)
                print("  step                              %9.4f ms per step  (%.4f .. %.4f)" % (b, min(base), max(base)), flush=True)
                for name, t in (("energy every %d (the CLI's loop)" % N, loop), ("step_energy every %d" % N, rec)):
                    m = statistics.median(t)
                    print("  %-33s %9.4f ms per step  (%.4f .. %.4f)  %+.1f %%, %+.1f us per row" % (
                        name, m, min(t), max(t), 100.0 * (m / b - 1.0), 1e3 * (m - b) * N), flush=True)
                e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
