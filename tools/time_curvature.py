#!/usr/bin/env python3
"""Time vof_curvature beside vof_interface on the same handle and state: -ic 1 after `--warm` steps (default: 4096^2 fp64 after 1000).

    python tools/time_curvature.py
    python tools/time_curvature.py --n 1024 --dtype f32 --warm 100

  rows + summary   us per Engine.curvature() / Engine.interface() call (count + scan, the summary's read-back, emit, the rows'
                   read-back; the calls remember their capacity, so this is one verb call each)
  summary only     us per sizing call (rows = NULL: count + scan and the summary only) -- the pass over F with the gathers of the
                   mixed cells (the count pass computes the rows for its sums), without the emit pass and the copy of the rows

Wall clock around calls that end in a device synchronise, median of `--reps` groups of `--calls` calls, in the same process on
the same handle, the two verbs alternating.  No threshold: the numbers go to profiles/curvature.md.
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
    ap.add_argument("--n", type=int, nargs="+", default=[4096])
    ap.add_argument("--dtype", nargs="+", default=["f64"])
    ap.add_argument("--warm", type=int, default=1000)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d import _abi, curvature
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    for n in a.n:
        for dtype in a.dtype:
            e = Engine(api, make_desc(api, n, n, dtype, "f32", device=a.device))
            e.set_init_F(1)
            e.step(a.warm)
            e.sync()
            fbytes = (n + 2) * (n + 2) * (8 if dtype == "f64" else 4)
            for _ in range(2):                         # settles the ghost cells, allocates the buffers, learns the capacities
                rows, summ = e.curvature()
                seg, isum = e.interface()
            d = curvature.derive(summ)
            print("# %d x %d %s dam-break after %d steps; F is %.1f MB" % (n, n, dtype, a.warm, fbytes / 1e6), flush=True)
            print("  curvature rows %d (valid %d = %.3f, degenerate %d), %d bytes; interface segments %d, %d bytes" % (
                summ["ROWS"], summ["VALID"], d["valid_share"], summ["DEGENERATE"], rows.nbytes, isum["SEGMENTS"], seg.nbytes), flush=True)
            print("  kappa (valid rows) mean %.4e rms %.4e; kappa_csf (all rows) mean %.4e rms %.4e" % (d["k_mean"], d["k_rms"], d["csf_mean"], d["csf_rms"]), flush=True)
            sc, si = (C.c_double * _abi.VOF_CURV_SUM_N)(), (C.c_double * _abi.VOF_IFACE_SUM_N)()
            t = {"curvature": [], "interface": [], "curvature_sizing": [], "interface_sizing": []}
            for _ in range(a.reps):
                t["curvature"].append(per_call(e.curvature, a.calls))
                t["interface"].append(per_call(e.interface, a.calls))
                t["curvature_sizing"].append(per_call(lambda: api.curvature(e.handle, 1e-6, None, 0, sc), a.calls))
                t["interface_sizing"].append(per_call(lambda: api.interface(e.handle, 1e-6, None, 0, si), a.calls))
            for key, label in (("curvature", "curvature (rows + summary)"), ("interface", "interface (rows + summary)"),
                               ("curvature_sizing", "curvature (summary only)"), ("interface_sizing", "interface (summary only)")):
                print("  %-28s %10.1f us per call  (%.1f .. %.1f)" % (label, statistics.median(t[key]), min(t[key]), max(t[key])), flush=True)
            print("  curvature / interface        %10.2f x (rows + summary)  %10.2f x (summary only)" % (
                statistics.median(t["curvature"]) / statistics.median(t["interface"]),
                statistics.median(t["curvature_sizing"]) / statistics.median(t["interface_sizing"])), flush=True)
            e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
