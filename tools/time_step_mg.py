#!/usr/bin/env python3
"""Time vof_step_mg against the loop of verbs it is defined by, and against vof_step for scale: one process per grid,
fp64 unless --dtype f32, -ic 1, `--steps` steps (default 200) after `--warm` warm ones (default 20), K = 1, 2, 3, both
modes of the coarsest-level solve.  Wall clock around work that ends in a device synchronise; `--reps` repetitions, each on
a fresh handle taken through the same warm steps; the median and the spread are printed.

    python tools/time_step_mg.py --n 1024
    python tools/time_step_mg.py --n 4096 --reps 2

  step_mg     vof_step_mg(steps, K): one call, one read-back at the end
  verbs       the definition of include/vof2d.h issued verb by verb through the ABI every library since vof_solve_p_mg has
              (this tool runs on a checkout without vof_step_mg too: the step_mg rows are then left out)
  step        vof_step(steps): the reference's ten sweeps, for scale

Also printed, per K: the last and the worst residual of the timed steps (relative criterion) -- how many cycles a stepped
run needs -- and the same quantity after the same number of vof_step steps.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))


def fresh(api, n, dtype, device, block):
    from vof2d.engine import Engine, make_desc
    e = Engine(api, make_desc(api, n, n, dtype, "f32", device=device))
    e.set_init_F(1)
    if block:
        e.set_param("mg_coarse_block", 1)
    return e


def verb_steps(e, n, K):
    res = []
    for _ in range(n):
        e.istep = e.istep + 1
        e.cal_nu_rho(); e.get_normal_young(); e.advect_upwind(); e.set_BC()
        res.append(e.solve_p_mg(-1.0, K, K, "rel", True)[1])
        e.update_uv(); e.set_BC(); e.solve_VOF_rudman(e.istep); e.post_process_f(); e.set_BC()
    return res


def timed(fn, e):
    e.sync()
    t0 = time.perf_counter()
    out = fn()
    e.sync()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warm", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cycles", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-verbs", action="store_true")
    a = ap.parse_args()
    from vof2d._lib import hip_api
    api = hip_api()
    have = hasattr(api, "step_mg")
    n, S, W = a.n, a.steps, a.warm
    print("# %d x %d %s dam-break, %d steps after %d warm ones, %d repetitions; ms per step: median (min .. max)" % (n, n, a.dtype, S, W, a.reps), flush=True)

    def row(name, times, note=""):
        ms = [1e3 * t / S for t in times]
        print("%-34s %8.4f  (%.4f .. %.4f)  %s" % (name, statistics.median(ms), min(ms), max(ms), note), flush=True)

    times = []
    for _ in range(a.reps):
        e = fresh(api, n, a.dtype, a.device, 0)
        e.step(W)
        t, _ = timed(lambda: e.step(S), e)
        res = e.solve_p_mg(1e300, 1, 1, "rel", build_rhs=False)[1]
        times.append(t)
        e.close()
    row("step (ten sweeps)", times, "residual after the last step %.3e" % res)
    for K in a.cycles:
        for block in ((0, 1) if have else (0,)):
            mode = "block" if block else "launches"
            if have:
                times = []
                for _ in range(a.reps):
                    e = fresh(api, n, a.dtype, a.device, block)
                    in_effect = e.get_param("mg_coarse_block")
                    e.step_mg(W, K)
                    t, (last, worst, at) = timed(lambda: e.step_mg(S, K, "rel"), e)
                    times.append(t)
                    e.close()
                row("step_mg K = %d, %s" % (K, mode), times, "last %.3e worst %.3e (step %d)%s" % (last, worst, at, "" if in_effect == block else " [knob not in effect]"))
            if a.no_verbs:
                continue
            times = []
            for _ in range(a.reps):
                e = fresh(api, n, a.dtype, a.device, block)
                verb_steps(e, W, K)
                t, res = timed(lambda: verb_steps(e, S, K), e)
                times.append(t)
                e.close()
            row("verbs   K = %d, %s" % (K, mode), times, "last %.3e worst %.3e (step %d)" % (res[-1], max(res), W + 1 + res.index(max(res))))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
