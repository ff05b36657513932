#!/usr/bin/env python3
"""Time vof_interface against copying F to the host: -ic 1 after `--warm` steps, 1024^2 and 4096^2 (one process, one handle
per case).

    python tools/time_interface.py
    python tools/time_interface.py --n 4096 --dtype f64 --warm 100

  interface     us per Engine.interface() call (count + scan, the summary's read-back, emit, the rows' read-back; the call
                remembers its capacity, so this is one vof_interface per call) and per sizing call (rows = NULL: count + scan
                and the summary only)
  get F         us per Engine.get("F"): the copy a driver needs today before it can contour on the host
  segments      rows returned and their bytes, against the bytes of F

Wall clock around calls that end in a device synchronise, median of `--reps` groups of `--calls` calls, in the same
process on the same handle, alternating.  No threshold: the numbers go to profiles/interface.md.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))


def per_call(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return 1e6 * (time.perf_counter() - t0) / calls


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--dtype", nargs="+", default=["f64"])
    ap.add_argument("--warm", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d import _abi
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    for n in a.n:
        for dtype in a.dtype:
            e = Engine(api, make_desc(api, n, n, dtype, "f32", device=a.device))
            e.set_init_F(1)
            e.step(a.warm)
            e.sync()
            esz = 8 if dtype == "f64" else 4
            fbytes = (n + 2) * (n + 2) * esz
            rows, summ = e.interface()                 # settles the ghost cells, allocates the buffers, learns the capacity
            e.interface()
            print("# %d x %d %s dam-break after %d steps; F is %.1f MB" % (n, n, dtype, a.warm, fbytes / 1e6), flush=True)
            print("  segments %d (degenerate %d), length %.6e; rows returned: %d bytes = 1 / %.0f of F" % (
                summ["SEGMENTS"], summ["DEGENERATE"], summ["LENGTH"], rows.nbytes, fbytes / max(rows.nbytes, 1)), flush=True)
            s = (C.c_double * _abi.VOF_IFACE_SUM_N)()
            t = {"interface": [], "sizing": [], "get": []}
            for _ in range(a.reps):
                t["interface"].append(per_call(e.interface, a.calls))
                t["sizing"].append(per_call(lambda: api.interface(e.handle, 1e-6, None, 0, s), a.calls))
                t["get"].append(per_call(lambda: e.get("F"), max(a.calls // 4, 1)))
            for key, label in (("interface", "interface (rows + summary)"), ("sizing", "interface (summary only)"), ("get", "get F (copy to the host)")):
                print("  %-28s %10.1f us per call  (%.1f .. %.1f)" % (label, statistics.median(t[key]), min(t[key]), max(t[key])), flush=True)
            print("  get F / interface            %10.1f x" % (statistics.median(t["get"]) / statistics.median(t["interface"])), flush=True)
            e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
