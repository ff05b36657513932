#!/usr/bin/env python3
"""Time vof_blobs against what a driver must do today -- copy F, u, v to the host and label there: 1024^2 and 4096^2 fp64,
the dam break at step 0 and after `--warm` steps, a checkerboard (the most blobs) and a one-cell-wide spiral (the longest
chain), one process, one handle per size.

    python tools/time_blobs.py
    python tools/time_blobs.py --n 4096 --warm 1000

  blobs         us per vof_blobs call that returns min(BLOBS, --cap) rows and the summary (every launch, both read-backs of the
                call, the copy of the rows)
  + labels      the same call with the labels copied out as well
  sizing        rows = NULL: labelling, numbering, records and the summary only (no sum pass)
  get F, u, v   us for the three Engine.get calls: the copies alone
  host label    seconds for scipy.ndimage.label on F >= 0.5 where scipy is importable (once; the sums would come on top)

Wall clock around calls that end in a device synchronise, median of `--reps` groups of `--calls` calls, in the same
process on the same handle, alternating.  No threshold: the numbers go to profiles/blobs.md.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))


def per_call(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return 1e6 * (time.perf_counter() - t0) / calls


def checkerboard(n):
    return ((np.arange(n)[:, None] + np.arange(n)[None, :]) % 2 == 0).astype(np.float64)


def spiral(n):
    """Square rings at even distance from the wall, each opened below its top-left corner and tied to the next ring inwards:
    one path of about n^2 / 2 cells."""
    i, j = np.arange(n)[:, None], np.arange(n)[None, :]
    d = np.minimum(np.minimum(i, j), np.minimum(n - 1 - i, n - 1 - j))
    m = (d % 2 == 0).astype(np.float64)
    for k in range(0, n // 2 - 2, 2):
        m[k + 1, k] = 0.0
        m[k + 2, k + 1] = 1.0
    return m


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--warm", type=int, default=1000)
    ap.add_argument("--cap", type=int, default=4096, help="rows asked for (a checkerboard has n^2 / 2 blobs: 128 bytes each)")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    from vof2d import _abi
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    try:
        from scipy import ndimage
    except ImportError:
        ndimage = None
    api = hip_api()
    ptr, iptr = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    for n in a.n:
        e = Engine(api, make_desc(api, n, n, a.dtype, "f32", device=a.device))
        e.set_init_F(1)
        fbytes = (n + 2) * (n + 2) * (8 if a.dtype == "f64" else 4)
        rows = np.empty((a.cap, _abi.VOF_BLOB_N))
        lab = np.empty((n, n), dtype=np.int32)
        s = (C.c_double * _abi.VOF_BLOB_SUM_N)()

        def pattern(m):
            F = np.zeros((n + 2, n + 2))
            F[1:-1, 1:-1] = m
            e.set("F", F)

        cases = [("dam break, step 0", lambda: None), ("dam break, step %d" % a.warm, lambda: e.step(a.warm)),
                 ("checkerboard", lambda: pattern(checkerboard(n))), ("spiral", lambda: pattern(spiral(n)))]
        for name, prepare in cases:
            prepare()
            e.sync()
            call = lambda: api.blobs(e.handle, 0, 0.5, rows.ctypes.data_as(ptr), a.cap, None, 0, s)
            with_labels = lambda: api.blobs(e.handle, 0, 0.5, rows.ctypes.data_as(ptr), a.cap, lab.ctypes.data_as(iptr), lab.nbytes, s)
            sizing = lambda: api.blobs(e.handle, 0, 0.5, None, 0, None, 0, s)
            assert with_labels() == 0 and call() == 0       # allocates the buffers
            print("# %d x %d %s, %s: %d liquid blobs, %d member cells, the largest %d; F, u, v are 3 x %.1f MB" % (
                n, n, a.dtype, name, s[0], s[1], s[2], fbytes / 1e6), flush=True)
            t = {"blobs": [], "labels": [], "sizing": [], "get": []}
            for _ in range(a.reps):
                t["blobs"].append(per_call(call, a.calls))
                t["labels"].append(per_call(with_labels, a.calls))
                t["sizing"].append(per_call(sizing, a.calls))
                t["get"].append(per_call(lambda: (e.get("F"), e.get("u"), e.get("v")), max(a.calls // 3, 1)))
            for key, label in (("blobs", "blobs (rows + summary)"), ("labels", "blobs + labels"), ("sizing", "blobs (summary only)"),
                               ("get", "get F, u, v (copies alone)")):
                print("  %-28s %10.1f us per call  (%.1f .. %.1f)" % (label, statistics.median(t[key]), min(t[key]), max(t[key])), flush=True)
            print("  get F, u, v / blobs          %10.2f x" % (statistics.median(t["get"]) / statistics.median(t["blobs"])), flush=True)
            if ndimage is not None:
                F = e.get("F")[1:-1, 1:-1]
                t0 = time.perf_counter()
                _, count = ndimage.label(F >= 0.5)
                print("  scipy.ndimage.label on the host %8.3f s (%d pieces)" % (time.perf_counter() - t0, count), flush=True)
                assert count == int(s[0])
        e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
