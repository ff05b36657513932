#!/usr/bin/env python3
"""What the dye costs (vof_dye_advance, vof_step_dye, vof_dye_stats; profiles/dye.md).

One process, one handle per grid, dtype and initial condition (-ic 1 dam break, -ic 2 rising bubble), `--warm` steps first,
the dye seeded equal to F (the transport of the dye then does the work the transport of F does).  Every figure is a wall
clock around work that ends in a device synchronise, `--reps` repetitions, median and spread; the candidates of a
comparison alternate on the same handle.
  advance     `--calls` back-to-back vof_dye_advance with knob dye_fused = 1 (k_dye + the boundary launch) and with
              dye_fused = 0 (k_fct_x, k_fct_y, k_post + the boundary launch: kernels of the parent commit); the bytes of
              k_dye's four array passes (C, u, v in, C out) over the time of a fused advance as a share of the HBM peak
              (8.0 TB/s; the call's time, so the boundary launch and the gaps between launches count against it)
  steps       vof_step(n) and vof_step_dye(n) alternating, ms per step, with the change of the counter tm_steps
  stats       vof_dye_stats against the host route (vof_dye_get, vof_get_field of F, u, v and the NumPy sums)

    python tools/time_dye.py [--n 4096] [--dtypes f64,f32] [--ics 1,2] [--steps 256] [--calls 50] [--reps 3] [--only advance]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
HBM_PEAK = 8.0e12   # bytes per second (MI355X, HBM3E)


def timed(e, fn):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return time.perf_counter() - t0


def med(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2], xs[0], xs[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--dtypes", default="f64,f32")
    ap.add_argument("--ics", default="1,2")
    ap.add_argument("--warm", type=int, default=64)
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="advance: that leg alone (for a kernel trace)")
    a = ap.parse_args()
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    names = {1: "dam-break", 2: "rising bubble", 3: "falling drop"}
    for dtype in a.dtypes.split(","):
        for ic in (int(x) for x in a.ics.split(",")):
            e = Engine(api, make_desc(api, a.n, a.n, dtype, "f32", device=0))
            e.set_init_F(ic)
            e.step(a.warm)
            e.dye_set(e.get("F"))
            esz = 8 if dtype == "f64" else 4
            print("# %d x %d %s %s, %d warm steps, dye = F" % (a.n, a.n, dtype, names[ic], a.warm), flush=True)
            # ---- one advance, fused against the two launches
            # (both sweep orders: the handle's istep decides, vof_set_istep moves it for the leg)
            istep0 = e.istep
            t = {(f, p): [] for f in (1, 0) for p in (0, 1)}
            for rep in range(a.reps + 1):
                for par in (0, 1):
                    e.istep = istep0 + ((istep0 + par) & 1)
                    for fused in (1, 0):
                        e.set_param("dye_fused", fused)
                        e.dye_advance()                                 # (first launch of the form after the knob moved)
                        dt = timed(e, lambda: [e.dye_advance() for _ in range(a.calls)]) / a.calls
                        if rep:                                         # (the first repetition: warm-up)
                            t[(fused, par)].append(dt * 1e6)
            e.istep = istep0
            moved = 4.0 * a.n * a.n * esz
            for par, order in ((0, "y then x"), (1, "x then y")):
                f1, f0 = med(t[(1, par)]), med(t[(0, par)])
                print("  dye_advance  %s  dye_fused = 1   %8.1f us per call  (%.1f .. %.1f)   4 passes = %.0f MB: %.2f TB/s, %.0f %% of the HBM peak" % (
                    (order,) + f1 + (moved / 1e6, moved / (f1[0] * 1e-6) / 1e12, 100.0 * moved / (f1[0] * 1e-6) / HBM_PEAK)), flush=True)
                print("  dye_advance  %s  dye_fused = 0   %8.1f us per call  (%.1f .. %.1f)   fused / two launches = %.2f" % ((order,) + f0 + (f1[0] / f0[0],)), flush=True)
            e.set_param("dye_fused", 1)
            if a.only == "advance":
                e.close()
                continue
            # ---- steps with and without the dye
            ts, td, tm = [], [], []
            for rep in range(a.reps + 1):
                c0 = e.get_counter("tm_steps")
                x = timed(e, lambda: e.step(a.steps)) / a.steps
                c1 = e.get_counter("tm_steps")
                y = timed(e, lambda: e.step_dye(a.steps)) / a.steps
                if rep:
                    ts.append(x * 1e3); td.append(y * 1e3); tm.append(c1 - c0)
            s, d = med(ts), med(td)
            print("  vof_step                     %8.4f ms per step  (%.4f .. %.4f)   tm_steps +%d per leg of %d" % (s + (tm[-1], a.steps)), flush=True)
            print("  vof_step_dye                 %8.4f ms per step  (%.4f .. %.4f)   %+.1f %%, %+.1f us per step" % (d + (100.0 * (d[0] / s[0] - 1.0), (d[0] - s[0]) * 1e3)), flush=True)
            # ---- a row of statistics against the host route
            row = med([timed(e, lambda: [e.dye_stats() for _ in range(20)]) / 20 * 1e6 for _ in range(a.reps)])

            def host():
                Cd, F, u, v = e.dye_get().astype(np.float64), e.get("F").astype(np.float64), e.get("u").astype(np.float64), e.get("v").astype(np.float64)
                c = Cd[1:-1, 1:-1]
                uc, vc = (u[1:-1, 1:-1] + u[2:, 1:-1]) * 0.5, (v[1:-1, 1:-1] + v[1:-1, 2:]) * 0.5
                return (c.sum(), (c * c).sum(), (c * np.clip(F[1:-1, 1:-1], 0, 1)).sum(), (c * uc).sum(), (c * vc).sum(), c.min(), c.max(), (c - F[1:-1, 1:-1]).max())
            hst = med([timed(e, host) * 1e6 for _ in range(a.reps)])
            print("  vof_dye_stats                %8.1f us per call  (%.1f .. %.1f), 20 calls per leg" % row, flush=True)
            print("  get + NumPy                  %8.1f us per call  (%.1f .. %.1f)" % hst, flush=True)
            e.close()


if __name__ == "__main__":
    main()
