#!/usr/bin/env python3
"""Time vof_set_scene against the route without it: the array built on the host by NumPy, then vof_set_field.

    python tools/time_scene.py
    python tools/time_scene.py --grid 1024 --shapes 1 16 --host-rows 64

Per shape count (seeded lists of discs, rotated boxes, rotated ellipses and triangles scattered over the domain, a half-plane pool
first; S = --samples):
  set_scene   ms per call with the knob scene_shortcuts at 1 and at 0, alternating: a hipEvent pair on the handle's stream around
              `--calls` back-to-back calls (each call uploads the list, zeroes two counters, runs k_scene and reads the counters
              back), `--reps` times, median and spread; and the same calls under a host clock (a call ends in a device
              synchronise).  The bytes of both knob values are compared (F, ghost cells included).
  host        seconds for tests/_scene_np.py -- full sampling in NumPy, the restatement the tests judge by -- to build the
              (nx+2, ny+2) array, and ms for the vof_set_field that uploads it.  Full sampling on the host is slow: beyond
              `--host-full` shapes only `--host-rows` rows (16 / shapes of them beyond 16 shapes, at least 8) are built and the time is
              scaled to all rows (the line says so);
              the rows that were built are compared with the device's.

No threshold: the numbers go to profiles/scene.md.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "taichi-2d-vof_amd"), os.path.join(ROOT, "tests")]


def shapes_of(n, L, seed):
    from vof2d import scene
    rng = np.random.default_rng(seed)
    out = [scene.halfplane(0.0, 0.3 * L, -0.1, 1.0, "liquid")]
    while len(out) < n:
        k = len(out)
        x, y, r, ang = rng.uniform(0, L), rng.uniform(0, L), rng.uniform(0.01 * L, 0.06 * L), rng.uniform(-180, 180)
        phase = "gas" if k % 3 == 0 else "liquid"
        out.append((scene.disc(x, y, r, phase), scene.box(x, y, r, 0.5 * r, ang, phase), scene.ellipse(x, y, r, 0.4 * r, ang, phase),
                    scene.triangle((x, y), (x + 2 * r, y + 0.5 * r), (x + 0.3 * r, y + 1.5 * r), phase))[k % 4])
    return scene.pack(out[:n])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grid", type=int, default=4096)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--shapes", type=int, nargs="+", default=[1, 16, 256])
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-full", type=int, default=1, help="up to this many shapes the host builds every row")
    ap.add_argument("--host-rows", type=int, default=64, help="rows the host builds beyond that (scaled to all rows)")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import _scene_np as snp
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    n, S = a.grid, a.samples
    e = Engine(api, make_desc(api, n, n, a.dtype, "f32", device=a.device))
    dx, dy, L = e.get_param("dx"), e.get_param("dy"), e.get_param("Lx")
    print("# %d x %d %s, S = %d, %d calls between an event pair, %d repetitions" % (n, n, a.dtype, S, a.calls, a.reps), flush=True)
    for count in a.shapes:
        recs = shapes_of(count, L, 100 + count)
        got = {}
        ev, wall = {1: [], 0: []}, {1: [], 0: []}
        for knob in (1, 0):                                # the first call of a form loads its code
            e.set_param("scene_shortcuts", knob)
            summ = e.set_scene(recs, S, True)
            got[knob] = e.get("F")
        same = got[0].tobytes() == got[1].tobytes()
        for _ in range(a.reps):
            for knob in (1, 0):
                e.set_param("scene_shortcuts", knob)
                e.sync()
                t0 = time.perf_counter()
                e.timer_start()
                for _ in range(a.calls):
                    e.set_scene(recs, S, True)
                ev[knob].append(e.timer_stop() / a.calls)
                wall[knob].append(1e3 * (time.perf_counter() - t0) / a.calls)
        print("  %4d shapes: painted %d, mixed %d; shortcuts 1 and 0 give %s bytes" % (count, summ["PAINTED"], summ["MIXED"], "the same" if same else "DIFFERENT"), flush=True)
        for knob in (1, 0):
            print("    vof_set_scene, shortcuts %d   %10.3f ms per call by events (%.3f .. %.3f), %10.3f ms by the host clock (%.3f .. %.3f)" % (
                knob, statistics.median(ev[knob]), min(ev[knob]), max(ev[knob]), statistics.median(wall[knob]), min(wall[knob]), max(wall[knob])), flush=True)
        if a.no_host:
            continue
        rows = n + 2 if count <= a.host_full else min(max(8, a.host_rows * 16 // max(count, 16)), n + 2)
        row0 = 0 if rows == n + 2 else (n + 2 - rows) // 2
        base = np.zeros((rows, n + 2), dtype=e.np_dtype)
        t0 = time.perf_counter()
        want, _, _ = snp.paint(base, recs, S, True, dx, dy, row_lo=row0)
        host = time.perf_counter() - t0
        ok = want.tobytes() == got[1][row0:row0 + rows].tobytes()
        full = np.zeros((n + 2, n + 2), dtype=e.np_dtype)
        full[row0:row0 + rows] = want
        up = []
        for _ in range(a.reps):
            e.sync()
            t0 = time.perf_counter()
            e.set("F", full)
            e.sync()
            up.append(1e3 * (time.perf_counter() - t0))
        scaled = host * (n + 2) / rows
        print("    NumPy on the host             %10.1f s for %d of %d rows%s; its rows equal the device's: %s" % (
            host, rows, n + 2, "" if rows == n + 2 else " = %.0f s scaled to all rows" % scaled, ok), flush=True)
        print("    vof_set_field of the array    %10.3f ms (%.3f .. %.3f)" % (statistics.median(up), min(up), max(up)), flush=True)
    e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
