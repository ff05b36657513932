#!/usr/bin/env python3
"""Time vof_regrid, and the route without it: the four fields read to the host, np.repeat, vof_set_field.

    python tools/time_regrid.py
    python tools/time_regrid.py --grid 1024 --factor 2 --host

Per case (refinement with PLIC, refinement without, coarsening back; -ic 1 after --spin steps on the source grid):
  vof_regrid   us per call without a summary (the call does not wait): a hipEvent pair on dst's stream around ONE call, 20 times,
               median and spread; and around `--calls` calls in a row, per call.  The call is its kernels (k_regrid_refine or
               k_regrid_coarsen, k_regrid_ring, k_set_bc) and, on a handle whose batch form follows the rule, the count of gas cells
               vof_set_init_F posts too (k_gas_cells and an 8-byte copy).  The bytes: 4 source fields read once, 5 arrays written.
  host         with --host: ms for vof_get_field of F, u, v, p, np.repeat along both axes and vof_set_field of the four, under a
               host clock (every call ends in a device synchronise).

No threshold: the numbers go to profiles/regrid.md (kernel times: rocprofv3 --kernel-trace --stats around this script, a run of its own).
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "taichi-2d-vof_amd")]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=1024, help="the coarse grid")
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--spin", type=int, default=200)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    n, N = a.grid, a.grid * a.factor
    esz = 8 if a.dtype == "f64" else 4
    print("# %d x %d <-> %d x %d %s, -ic 1 after %d steps; one call between an event pair, 20 times; %d calls between a pair, 20 times"
          % (n, n, N, N, a.dtype, a.spin, a.calls), flush=True)
    for name, s, d, plic in (("refine, PLIC", n, N, True), ("refine, no PLIC", n, N, False), ("coarsen", N, n, True)):
        src = Engine(api, make_desc(api, s, s, a.dtype, "f32", device=a.device))
        dst = Engine(api, make_desc(api, d, d, a.dtype, "f32", device=a.device))
        src.set_init_F(1)
        src.step(a.spin)
        summ = dst.regrid_from(src, plic=plic)
        for _ in range(5):                                   # the first call of a form loads its code
            dst.regrid_from(src, plic=plic, summary=False)
        dst.sync()
        one, many = [], []
        for _ in range(20):
            dst.timer_start()
            dst.regrid_from(src, plic=plic, summary=False)
            one.append(1e3 * dst.timer_stop())
        for _ in range(20):
            dst.timer_start()
            for _ in range(a.calls):
                dst.regrid_from(src, plic=plic, summary=False)
            many.append(1e3 * dst.timer_stop() / a.calls)
        moved = (4 * s * s + 5 * d * d) * esz
        print("  %-16s %8.1f us per call (%.1f .. %.1f); %8.1f us per call of %d in a row; %.1f MB read + written = %.2f TB/s of the call; "
              "cells from a line %d, volume %.12g -> %.12g"
              % (name, statistics.median(one), min(one), max(one), statistics.median(many), a.calls, moved / 1e6,
                 moved / (statistics.median(one) * 1e-6) / 1e12, summ["PLIC_CELLS"], summ["F_SRC"] / (s * s), summ["F_DST"] / (d * d)), flush=True)
        if a.host and d > s:
            r = d // s
            took = []
            for _ in range(5):
                dst.sync()
                t0 = time.perf_counter()
                for f in ("F", "u", "v", "p"):
                    x = src.get(f)
                    y = np.empty((d + 2, d + 2), dtype=x.dtype)
                    y[1:-1, 1:-1] = np.repeat(np.repeat(x[1:-1, 1:-1], r, axis=0), r, axis=1)
                    dst.set(f, y)
                dst.set_BC()
                dst.sync()
                took.append(1e3 * (time.perf_counter() - t0))
            print("  %-16s %8.2f ms (%.2f .. %.2f): vof_get_field x 4, np.repeat, vof_set_field x 4, vof_set_BC" % ("  on the host", statistics.median(took), min(took), max(took)), flush=True)
        src.close(); dst.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
