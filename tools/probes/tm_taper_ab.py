#!/usr/bin/env python3
"""Same-box A/B of k_tm chunk layouts and library builds: every run a process of its own, the cases alternating.

    python3 tools/probes/tm_taper_ab.py [--n 4096] [--reps 6] [-ic 1] [--dt 0] parent:none base:off base:rule base:3641:26,3849:13

A case is LIBRARY:LAYOUT.  LIBRARY as in tools/variant_ab.py ("base" = the product library, anything else
build/variants/libvof2d_NAME.so -- "parent": the parent commit's build, copied there).  LAYOUT: "none" (no knob is touched: a
library without the knobs), "off" (tm_taper = 0), "rule" (tm_taper = -1) or up to three first_row:chunk_rows of the tail
segments (tm_taper = 1), or "shares:S1,S2,S3": the layout L::tm_chunk_rows' rule would cut with these shares (per cent of the
resident pairs per tail segment, chunk lengths R / 2, R / 4, R / 6 with a floor of 8 rows; fp64, 1536 resident pairs), set
through the explicit knobs -- for sweeping the rule's constants without a build per candidate.  Per run: ms/step over steps 21-220 (bench.py's window) and 61-460, then k_tm us per launch from
the in-situ profile of steps 461-510, the number of segments of the last k_tm launch and a digest of the state."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def rule_layout(n, shares, cap=1536, div=(2, 4, 6), floor=8):
    """L::tm_body_rows and the rule of L::tm_chunk_rows, restated: "first_row:chunk_rows,..." or "off" """
    ntf = (n + 111) // 112
    k = max(2, (n * ntf + cap * 25) // (cap * 50))
    chunks = max(1, k * cap * 97 // 100 // ntf)
    R = min(96, max(16, (n + chunks - 1) // chunks))
    if ((n + R - 1) // R) * ntf <= cap:
        return "off"
    lo, out = n + 1, []
    for j in (2, 1, 0):
        ln = max(R // div[j], floor)
        lo -= ((shares[j] * cap + 50 * ntf) // (100 * ntf)) * ln
        out.insert(0, "%d:%d" % (lo, ln))
    return "off" if lo < 1 + R else ",".join(out)


def child(a):
    from variant_ab import lib_path
    from vof2d import _abi
    from vof2d.engine import Engine, make_desc
    name, layout = a.child.split(":", 1)
    api = _abi.bind(ctypes.CDLL(lib_path(name), mode=ctypes.RTLD_GLOBAL), "vof_")
    kw = {"dt": a.dt} if a.dt > 0 else {}
    e = Engine(api, make_desc(api, a.n, a.n, a.dtype, "f32", device=0, **kw))
    for k, v in (kv.split("=") for kv in a.param):
        e.set_param(k, float(v))
    if layout.startswith("shares:"):
        layout = rule_layout(a.n, [int(x) for x in layout[7:].split(",")])
    if layout == "off":
        e.set_param("tm_taper", 0)
    elif layout == "rule":
        e.set_param("tm_taper", -1)
    elif layout != "none":
        for j, s in enumerate(layout.split(",")):
            at, rows = s.split(":")
            e.set_param("tm_tail_at%d" % (j + 1), int(at))
            e.set_param("tm_tail_rows%d" % (j + 1), int(rows))
        e.set_param("tm_taper", 1)
    e.set_init_F(a.ic)
    e.step(20)
    ms = []
    for k in (40, 160, 240):
        e.sync()
        t0 = time.perf_counter()
        e.step(k)
        e.sync()
        ms.append(1e3 * (time.perf_counter() - t0))
    prof = e.profile_steps(50)
    h = hashlib.sha256()
    for f in ("F", "u", "v", "p"):
        h.update((e.get(f) + 0.0).tobytes())
    seg = e.get_counter("tm_segments") if layout != "none" else 0
    print(json.dumps({"bench": (ms[0] + ms[1]) / 200, "long": (ms[1] + ms[2]) / 400, "tm": [prof.get(k, (0, 0))[0] for k in ("k_tm", "k_tm_uv")],
                      "jp": prof.get("k_jacobi_pair", (0, 0))[0], "segments": seg, "tm_steps": e.get_counter("tm_steps"), "state": h.hexdigest()[:12]}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("cases", nargs="*", default=["base:off", "base:rule"])
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--dtype", default="f64")
    ap.add_argument("-ic", type=int, default=1)
    ap.add_argument("--dt", type=float, default=0.0)
    ap.add_argument("--param", action="append", default=[])
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {c: [] for c in a.cases}
    for rep in range(a.reps):
        for c in a.cases:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", c, "--n", str(a.n), "--dtype", a.dtype, "-ic", str(a.ic), "--dt", str(a.dt)]
            cmd += sum((["--param", p] for p in a.param), [])
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                print(c, "FAILED rc", r.returncode, r.stderr[-600:], flush=True)
                if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
                    return 1      # a fault: nothing more on the GPU
                continue
            res[c].append(json.loads(r.stdout.strip().splitlines()[-1]))
    print("workload: %d^2 %s ic %d dt %g %s; ms/step over steps 21-220 | 61-460; k_tm / k_tm_uv / k_jacobi_pair us per launch in steps 461-510" % (
        a.n, a.dtype, a.ic, a.dt, " ".join(a.param)))
    for c, runs in res.items():
        if not runs:
            continue
        for w in ("bench", "long"):
            v = [r[w] for r in runs]
            print("%-40s %-5s min %.4f median %.4f max %.4f | %s" % (c, w, min(v), statistics.median(v), max(v), " ".join("%.4f" % x for x in v)))
        print("%-40s k_tm %s | k_tm_uv %s | k_jacobi_pair %s | segments %s tm_steps %s state %s" % (
            c, " ".join("%.1f" % r["tm"][0] for r in runs), " ".join("%.1f" % r["tm"][1] for r in runs), " ".join("%.1f" % r["jp"] for r in runs),
            sorted(set(r["segments"] for r in runs)), sorted(set(r["tm_steps"] for r in runs)), sorted(set(r["state"] for r in runs))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
