#!/usr/bin/env python3
"""How does a k_tm launch end, and what do shorter chunks in the rows handed out last do to it?  Diagnostic build
(make -C taichi-2d-vof_amd/csrc wavetimes).  All layouts run on ONE engine and ONE state per `--at` step
(vof_debug_time_kernel: the state is not advanced), so the engines' speed lottery does not enter.

    python3 tools/probes/tm_tail.py [--n 4096] [--at 30,96,704] [--layout off] [--layout 3500:26,3900:13] ...

A layout is "off" (one segment, knob tm_taper = 0), "rule" (tm_taper = -1; timed only, not mapped) or up to three
"first_row:chunk_rows" of the tail segments (tm_taper = 1, knobs tm_tail_at* / tm_tail_rows*).  Per state and layout:
us per launch behind a cache flush (`--reps` launches, each timed alone) and back to back, then from the per-wave stamps
of one launch: the span, sum of durations / (span x slots), the time from "waves in flight first below 90 % of their peak"
to the end, and which pairs are alive in that window (segment, chunk row, interior or not)."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "taichi-2d-vof_amd"))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=4096)
ap.add_argument("--at", default="30,96,704")
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("-ic", type=int, default=1)
ap.add_argument("--dt", type=float, default=0.0)
ap.add_argument("--layout", action="append", default=[])
ap.add_argument("--slots", type=int, default=1536, help="resident pairs (256 CUs x 6)")
ap.add_argument("--no-map", action="store_true")
a = ap.parse_args()
from vof2d import _abi
from vof2d.engine import Engine, make_desc

lib = C.CDLL(os.path.join(ROOT, "taichi-2d-vof_amd", "csrc", "build", "variants", "libvof2d_wavetimes.so"))
api = _abi.bind(lib, "vof_")
tk = lib.vof_debug_time_kernel
tk.restype = C.c_int
tk.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_float)]
dbg = lib.vof_debug_wave_times
dbg.restype = C.c_int
dbg.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_uint32]
kw = {"dt": a.dt} if a.dt > 0 else ({"dt": 1e-6} if a.n > 4096 else {})
e = Engine(api, make_desc(api, a.n, a.n, "f64", "f32", device=0, **kw))
e.set_param("fuse_tm", 1)
e.set_init_F(a.ic)
NTF = (a.n + 111) // 112
XCD_GROUP = 10   # kXcdGroup, kernels/common.h


def body_rows(rows):   # L::tm_body_rows
    k = max(2, (rows * NTF + a.slots * 25) // (a.slots * 50))
    chunks = max(1, k * a.slots * 97 // 100 // NTF)
    return min(96, max(16, (rows + chunks - 1) // chunks))


def segments(layout):   # [(first, last, R)] as L::tm_chunk_rows cuts rows 1 .. n
    R = body_rows(a.n)
    if layout == "off":
        return [(1, a.n, R)]
    tail = [tuple(int(x) for x in s.split(":")) for s in layout.split(",")]
    ats = [t[0] for t in tail] + [a.n + 1]
    return [(1, ats[0] - 1, R)] + [(ats[i], ats[i + 1] - 1, tail[i][1]) for i in range(len(tail))]


def set_layout(layout):
    for j in range(3):
        e.set_param("tm_tail_at%d" % (j + 1), 0)
    if layout in ("off", "rule"):
        e.set_param("tm_taper", 0 if layout == "off" else -1)
        return
    for j, s in enumerate(layout.split(",")):
        at, rows = s.split(":")
        e.set_param("tm_tail_at%d" % (j + 1), int(at))
        e.set_param("tm_tail_rows%d" % (j + 1), int(rows))
    e.set_param("tm_taper", 1)


def t(abl, reps):
    us = C.c_float(0)
    rc = tk(e._h, 1, abl, 0, reps, C.byref(us))
    assert rc == 0, rc
    return us.value


def xcd_grouped_block(b, n):
    win = 8 * XCD_GROUP
    base = (b // win) * win
    if base + win > n:
        return b
    o = b - base
    return base + (o & 7) * XCD_GROUP + (o >> 3)


def tail_map(layout):
    segs = segments(layout)
    chunks = []   # (segment, first row, last row) in launch order
    for k, (f, l, R) in enumerate(segs):
        chunks += [(k, r, min(r + R - 1, l)) for r in range(f, l + 1, R)]
    npairs = len(chunks) * NTF
    cap = 1 << 15
    assert 2 * npairs <= cap
    assert dbg(e._h, 14, None, cap) == 0
    t(0, 1)
    st = np.zeros((cap, 2), np.uint64)
    assert dbg(e._h, 14, st.ctypes.data, cap) == 0
    assert dbg(e._h, -1, None, cap) == 0
    m = st[:, 1] > 0
    ids = np.nonzero(m)[0]
    assert len(ids) == 2 * npairs, (len(ids), npairs)
    t0 = st[m, 0].astype(np.int64); t1 = st[m, 1].astype(np.int64)
    base = t0.min()
    t0 = (t0 - base) / 100.0; t1 = (t1 - base) / 100.0   # us
    span = t1.max()
    ev = np.concatenate([np.stack([t0, np.ones_like(t0)], 1), np.stack([t1, -np.ones_like(t1)], 1)])
    ev = ev[np.argsort(ev[:, 0], kind="stable")]
    fl = np.cumsum(ev[:, 1])
    peak = fl.max()
    at_peak = int(np.argmax(fl >= peak))
    below = np.nonzero(fl[at_peak:] < 0.9 * peak)[0]
    t90 = ev[at_peak + below[0], 0] if len(below) else span
    below = np.nonzero(fl[at_peak:] < 0.5 * peak)[0]
    t50 = ev[at_peak + below[0], 0] if len(below) else span
    print("   %d pairs in %d segments %s: span %.1f us, peak %d waves, sum of durations / (span x peak) = %.3f, below 90 %% of the peak for the last %.1f us, below 50 %% for the last %.1f" % (
        npairs, len(segs), segs, span, int(peak), (t1 - t0).sum() / (span * peak), span - t90, span - t50))
    edges = np.linspace(0, span, 21)
    mid = (edges[:-1] + edges[1:]) / 2
    print("   waves in flight (20 slices): " + " ".join("%d" % int(((t0 <= x) & (t1 > x)).sum()) for x in mid))
    # the pairs alive after t90 (by their transport wave), by chunk and kind
    alive = {}
    ends = {}
    for w, s0, s1 in zip(ids, t0, t1):
        if w & 1:
            continue
        pair = xcd_grouped_block(int(w) >> 1, npairs)
        ch, tj = pair // NTF, pair % NTF
        k, ma, mb = chunks[ch]
        c0 = 1 - 8 + tj * 112
        interior = ma - 8 >= 1 and mb + 7 <= a.n and c0 >= 2 and c0 + 127 <= a.n
        ends.setdefault(ch, []).append((s0, s1))
        if s1 > t90:
            key = (k, ch, ma, mb)
            alive.setdefault(key, [0, 0, 0.0])
            alive[key][0 if interior else 1] += 1
            alive[key][2] = max(alive[key][2], s1)
    print("   alive in that window: (segment, chunk row, rows): interior + other pairs, last end us")
    print("     " + "; ".join("(%d, %d, %d-%d): %d + %d, %.0f" % (k[0], k[1], k[2], k[3], v[0], v[1], v[2]) for k, v in sorted(alive.items())))
    g = max(1, len(chunks) // 20)
    print("   chunk rows in groups of %d: mean start / mean duration us: %s" % (g, " ".join(
        "%.0f/%.0f" % (np.mean([s for c in range(q, min(q + g, len(chunks))) for s, _ in ends[c]]),
                       np.mean([s1 - s for c in range(q, min(q + g, len(chunks))) for s, s1 in ends[c]])) for q in range(0, len(chunks), g))), flush=True)


done = 0
layouts = a.layout or ["off"]
for at in [int(x) for x in a.at.split(",")]:
    e.step(at - done)
    done = at
    e.sync()
    print("== %d^2 fp64 ic %d after %d steps, %d tile columns, body chunks of %d rows" % (a.n, a.ic, at, NTF, body_rows(a.n)), flush=True)
    for rnd in range(2):     # every layout twice, in turns
        for lay in layouts:
            set_layout(lay)
            print(" %-28s round %d: k_tm behind a cache flush %.1f us, back to back %.1f us, segments %d" % (
                lay, rnd, t(256, a.reps), t(0, a.reps), e.get_counter("tm_segments")), flush=True)
    if not a.no_map:
        for lay in layouts:
            if lay == "rule":
                continue
            set_layout(lay)
            print(" wave map of one launch, layout %s:" % lay)
            tail_map(lay)
