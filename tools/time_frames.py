#!/usr/bin/env python3
"""Time vof_frame and vof_step_frames: -ic 1, fp64, `--warm` steps in (one process, one handle per grid).

    python tools/time_frames.py
    python tools/time_frames.py --kernels        # under rocprofv3 --kernel-trace --stats: the per-kernel times

  frame         us per vof_frame call (the words zeroed, k_frame_cols, k_frame_fold, k_frame_paint, one copy of the picture
                and the summary, one wait) for F, SPEED and VORT at `--blocks` cells per pixel, with and without the contour,
                beside vof_depths on the same state (it also reads F once) and the parent's routes to the same picture on the
                host: vof_get_field("F") and a reshape-mean; vof_get_vis_field + vis.colour_image at the grids of `--vis-grids`
                (four times the field on the way, an RGBA array of doubles at the end); wall clock around `--calls` calls each,
                `--reps` times; the algorithmic bytes of k_frame_cols and their share of `--peak` TB/s
  step          ms per step of vof_step(steps) against vof_step_frames(steps, every) on the same handle, alternating, `--reps`
                times each; the added ms per frame
  --kernels     nothing but `--calls` calls of every frame form and of vof_depths behind a warm-up: run it under a kernel trace

No threshold: the numbers go to profiles/frames.md.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))

FIELDS_READ = {"F": 1, "SPEED": 2, "VORT": 2}      # arrays k_frame_cols reads once (the contour adds F where it is not the quantity)


def wall(fn, e):
    e.sync()
    t0 = time.perf_counter()
    fn()
    e.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--grids", type=int, nargs="+", default=[4096])
    ap.add_argument("--vis-grids", type=int, nargs="+", default=[2048])
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--blocks", type=int, nargs="+", default=[8, 4])
    ap.add_argument("--warm", type=int, default=300)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--every", type=int, default=100)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--peak", type=float, default=8.0, help="TB/s the shares are quoted against")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    import numpy as np
    from vof2d._lib import hip_api
    from vof2d.engine import Engine, make_desc
    api = hip_api()
    esz = 8 if a.dtype == "f64" else 4
    forms = [(q, b, c) for b in a.blocks for q in ("F", "SPEED", "VORT") for c in (False, True)]

    def per_call(fn, e, calls):
        us = []
        for _ in range(a.reps):
            us.append(1e6 * wall(lambda: [fn() for _ in range(calls)], e) / calls)
        return statistics.median(us), min(us), max(us)

    for n in sorted(set(a.grids) | (set() if a.kernels else set(a.vis_grids))):
        e = Engine(api, make_desc(api, n, n, a.dtype, "f32", device=a.device))
        e.set_init_F(1)
        e.step(a.warm)
        e.depths()
        for q, b, c in forms:                       # the buffers; the first launches load the code object
            e.frame(q, b, contour=c)
        print("# %d x %d %s dam-break, %d warm steps" % (n, n, a.dtype, a.warm), flush=True)
        if a.kernels:
            for q, b, c in forms:
                for _ in range(a.calls):
                    e.frame(q, b, contour=c, rgb=False)
            for _ in range(a.calls):
                e.depths()
            e.close()
            continue
        if n in a.grids:
            print("  %-34s %10.1f us per call  (%.1f .. %.1f)" % (("vof_depths",) + per_call(e.depths, e, a.calls)), flush=True)
            for q, b, c in forms:
                fields = FIELDS_READ[q] + (1 if c and q != "F" else 0)
                mb = (fields * n * n * esz + (2 if c and q != "F" else 1) * 2 * (n // b) * n * 8) / 1e6
                med, lo, hi = per_call(lambda: e.frame(q, b, contour=c), e, a.calls)
                print("  vof_frame %-5s %d x %d %-8s      %10.1f us per call  (%.1f .. %.1f)  k_frame_cols moves %.1f MB: %.1f us at %.0f TB/s" % (
                    q, b, b, "contour" if c else "", med, lo, hi, mb, mb / a.peak, a.peak), flush=True)

            def host_mean(b):
                F = e.get("F")[1:-1, 1:-1].astype(np.float64)
                return F.reshape(n // b, b, n // b, b).mean(axis=(1, 3))
            for b in a.blocks:
                print("  get_field(F) + reshape-mean %d x %d    %10.1f us per call  (%.1f .. %.1f)" % ((b, b) + per_call(lambda: host_mean(b), e, 2)), flush=True)
        if n in a.vis_grids:
            from vof2d import vis
            print("  get_vis_field(vof) + colour_image    %10.1f us per call  (%.1f .. %.1f)" % per_call(lambda: vis.colour_image(e.vis_field("vof"), 0), e, 2), flush=True)
            print("  vof_frame F at %d x %d               %10.1f us per call  (%.1f .. %.1f)" % ((a.blocks[0], a.blocks[0]) + per_call(lambda: e.frame("F", a.blocks[0]), e, a.calls)),
                  flush=True)
        if n == max(a.grids):
            S, N = a.steps, a.every
            base, rec = [], {}
            for _ in range(a.reps):
                base.append(1e3 * wall(lambda: e.step(S), e) / S)
                for q, c in (("F", False), ("VORT", True)):
                    rec.setdefault((q, c), []).append(1e3 * wall(lambda: e.step_frames(S, N, q, a.blocks[0], contour=c), e) / S)
            b0 = statistics.median(base)
            print("  %d steps per leg" % S, flush=True)
            print("  vof_step                              %9.4f ms per step  (%.4f .. %.4f)" % (b0, min(base), max(base)), flush=True)
            for (q, c), t in rec.items():
                m = statistics.median(t)
                print("  vof_step_frames every %d %-5s %-8s %9.4f ms per step  (%.4f .. %.4f)  %+.2f %%, %+.3f ms per frame" % (
                    N, q, "contour" if c else "", m, min(t), max(t), 100.0 * (m / b0 - 1.0), (m - b0) * N), flush=True)
        e.close()
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
