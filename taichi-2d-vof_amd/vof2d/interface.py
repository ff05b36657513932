"""The interface as PLIC segments extracted on the device (vof_interface; include/vof2d.h): the slots of a row and of the
summary, how the lists of several strips combine, and chaining the segments into polylines for a plot.

`Engine.interface()` returns (rows, summary): an (n, VOF_IFACE_N) float64 array in ascending (i, j) order and a dict keyed
by SUMMARY.  Liquid lies to the left of (X0, Y0) -> (X1, Y1); (NX, NY) is the unit normal, liquid -> gas.
"""
import numpy as np

from ._abi import VOF_IFACE_N, VOF_IFACE_SUM_N

I, J, X0, Y0, X1, Y1, NX, NY = range(VOF_IFACE_N)
NAMES = ("I", "J", "X0", "Y0", "X1", "Y1", "NX", "NY")
SUMMARY = ("SEGMENTS", "DEGENERATE", "LENGTH", "ISTEP")
COUNTS = ("SEGMENTS", "DEGENERATE")


def summary_of(summ):
    """The summary (a sequence of VOF_IFACE_SUM_N doubles, or a dict already) as {name: value}; the counts as ints."""
    if isinstance(summ, dict):
        return summ
    if len(summ) != VOF_IFACE_SUM_N:
        raise ValueError("a summary has %d values, not %d" % (VOF_IFACE_SUM_N, len(summ)))
    out = {name: float(summ[k]) for k, name in enumerate(SUMMARY)}
    out.update({k: int(out[k]) for k in COUNTS + ("ISTEP",)})
    return out


def combine(parts):
    """(rows, summary) of the whole domain from the (rows, summary) of its strips in rank order: the rows concatenated,
    the counts and the lengths added in that order; ISTEP must agree."""
    parts = [(np.asarray(r, dtype=np.float64).reshape(-1, VOF_IFACE_N), summary_of(s)) for r, s in parts]
    if not parts:
        raise ValueError("combine needs at least one part")
    out = dict(parts[0][1])
    for _, s in parts[1:]:
        if s["ISTEP"] != out["ISTEP"]:
            raise ValueError("parts of different steps: istep %r and %r" % (out["ISTEP"], s["ISTEP"]))
        for k in COUNTS + ("LENGTH",):
            out[k] = out[k] + s[k]
    return np.concatenate([r for r, _ in parts], axis=0), out


def polylines(rows, tol=None):
    """Chain the segments whose end points coincide within `tol` into polylines: a list of (m, 2) arrays of points, each
    walked with the liquid on its left.  Host work for plotting, no bit contract: PLIC segments of neighbouring cells do
    not meet in general, so `tol` decides what counts as joined (default: a quarter of the median segment length)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, VOF_IFACE_N)
    n = len(rows)
    if n == 0:
        return []
    a, b = rows[:, [X0, Y0]], rows[:, [X1, Y1]]
    if tol is None:
        tol = 0.25 * float(np.median(np.hypot(*(b - a).T)))
    tol = max(float(tol), 0.0)
    cell = tol if tol > 0.0 else 1.0
    # the start points binned on a grid of the tolerance: the successor of a segment is the nearest unused start near its end
    bins = {}
    for k in range(n):
        bins.setdefault((int(np.floor(a[k, 0] / cell)), int(np.floor(a[k, 1] / cell))), []).append(k)
    nxt = np.full(n, -1, dtype=np.int64)
    has_prev = np.zeros(n, dtype=bool)
    for k in range(n):
        bx, by = int(np.floor(b[k, 0] / cell)), int(np.floor(b[k, 1] / cell))
        best, best_d = -1, None
        for cx in (bx - 1, bx, bx + 1):
            for cy in (by - 1, by, by + 1):
                for m in bins.get((cx, cy), ()):
                    if m == k or has_prev[m]:
                        continue
                    d = float(np.hypot(a[m, 0] - b[k, 0], a[m, 1] - b[k, 1]))
                    if d <= tol and (best_d is None or d < best_d):
                        best, best_d = m, d
        if best >= 0:
            nxt[k] = best
            has_prev[best] = True
    out, seen = [], np.zeros(n, dtype=bool)
    for start in list(np.flatnonzero(~has_prev)) + list(range(n)):   # open chains from their heads, then what is left: closed loops
        if seen[start]:
            continue
        pts, k = [a[start]], start
        while k >= 0 and not seen[k]:
            seen[k] = True
            pts.append(b[k])
            k = nxt[k]
        out.append(np.array(pts))
    return out
