"""Droplets and bubbles labelled and measured on the device (vof_blobs; include/vof2d.h): the slots of a row and of the
summary, the physical quantities of a blob, and how the lists of several strips join into the domain's.

`Engine.blobs()` returns (rows, summary[, labels]): an (n, VOF_BLOB_N) float64 array in ascending order of the blobs' first
cells, a dict keyed by SUMMARY and the (owned interior rows, ny) int32 array of blob indices (-1: not a member).
"""
import numpy as np

from ._abi import VOF_BLOB_GAS, VOF_BLOB_LIQUID, VOF_BLOB_N, VOF_BLOB_SUM_N

I0, J0, CELLS, IMIN, IMAX, JMIN, JMAX, SUM_W, SUM_WI, SUM_WJ, SUM_WU, SUM_WV = range(12)
NAMES = ("I0", "J0", "CELLS", "IMIN", "IMAX", "JMIN", "JMAX", "SUM_W", "SUM_WI", "SUM_WJ", "SUM_WU", "SUM_WV")
SUMS = (SUM_W, SUM_WI, SUM_WJ, SUM_WU, SUM_WV)
SUMMARY = ("BLOBS", "MEMBER_CELLS", "MAX_CELLS", "ISTEP")
PHASES = {"liquid": VOF_BLOB_LIQUID, "gas": VOF_BLOB_GAS, VOF_BLOB_LIQUID: VOF_BLOB_LIQUID, VOF_BLOB_GAS: VOF_BLOB_GAS}
CSV_HEADER = "istep,blob,cells,volume,xc,yc,uc,vc,imin,imax,jmin,jmax"


def summary_of(summ):
    """The summary (a sequence of VOF_BLOB_SUM_N doubles, or a dict already) as {name: int}."""
    if isinstance(summ, dict):
        return summ
    if len(summ) != VOF_BLOB_SUM_N:
        raise ValueError("a summary has %d values, not %d" % (VOF_BLOB_SUM_N, len(summ)))
    return {name: int(summ[k]) for k, name in enumerate(SUMMARY)}


def derived(rows, dx, dy):
    """The physical quantities of every blob as a dict of arrays: volume = SUM_W dx dy, the centroid xc = (SUM_WI / SUM_W - 0.5) dx,
    yc = (SUM_WJ / SUM_W - 0.5) dy, the velocity uc = SUM_WU / SUM_W, vc = SUM_WV / SUM_W; NaN where SUM_W == 0."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, VOF_BLOB_N)
    w = rows[:, SUM_W]
    with np.errstate(all="ignore"):
        inv = np.where(w == 0.0, np.nan, 1.0 / np.where(w == 0.0, 1.0, w))
        return {"volume": w * dx * dy,
                "xc": (rows[:, SUM_WI] * inv - 0.5) * dx, "yc": (rows[:, SUM_WJ] * inv - 0.5) * dy,
                "uc": rows[:, SUM_WU] * inv, "vc": rows[:, SUM_WV] * inv}


def csv_lines(rows, istep, dx, dy):
    """One line of CSV_HEADER per blob."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, VOF_BLOB_N)
    d = derived(rows, dx, dy)
    return ["%d,%d,%d,%r,%r,%r,%r,%r,%d,%d,%d,%d" % (istep, b, r[CELLS], float(d["volume"][b]), float(d["xc"][b]), float(d["yc"][b]),
                                                   float(d["uc"][b]), float(d["vc"][b]), r[IMIN], r[IMAX], r[JMIN], r[JMAX])
            for b, r in enumerate(rows)]


def combine(parts, ny):
    """(rows, summary, labels) of the whole domain from the (rows, summary, labels) of its strips in rank order (every strip
    with ALL its rows and its labels).  Two blobs are one where the last row of a strip and the first row of the next hold
    members at the same j: a union-find over the strips' blobs, fed from those two rows of labels.  Of a joined blob the
    integer slots combine exactly (CELLS added, the extent by min / max, the smaller first cell) and the five sums are added
    in rank order; the list is sorted by first cell again and the labels renumbered."""
    parts = [(np.asarray(r, dtype=np.float64).reshape(-1, VOF_BLOB_N), summary_of(s), np.asarray(l, dtype=np.int32).reshape(-1, ny))
             for r, s, l in parts]
    if not parts:
        raise ValueError("combine needs at least one part")
    for r, s, _ in parts:
        if s["ISTEP"] != parts[0][1]["ISTEP"]:
            raise ValueError("parts of different steps: istep %r and %r" % (parts[0][1]["ISTEP"], s["ISTEP"]))
        if len(r) != s["BLOBS"]:
            raise ValueError("combine needs every row of every part (%d of %d given)" % (len(r), s["BLOBS"]))
    base = np.cumsum([0] + [len(r) for r, _, _ in parts])          # a strip's blob b is number base[strip] + b
    allrows = np.concatenate([r for r, _, _ in parts], axis=0)
    parent = np.arange(len(allrows))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for k in range(len(parts) - 1):
        lo_l, hi_l = parts[k][2], parts[k + 1][2]
        if len(lo_l) == 0 or len(hi_l) == 0:
            continue
        a, b = lo_l[-1].astype(np.int64), hi_l[0].astype(np.int64)
        both = (a >= 0) & (b >= 0)
        for x, y in set(zip((a[both] + base[k]).tolist(), (b[both] + base[k + 1]).tolist())):
            rx, ry = find(x), find(y)
            if rx != ry:
                parent[max(rx, ry)] = min(rx, ry)      # (strips in rank order: the smaller number holds the smaller first cell)
    roots = np.array([find(x) for x in range(len(allrows))], dtype=np.int64)
    order = np.flatnonzero(roots == np.arange(len(allrows)))         # ascending number = ascending first cell
    new_of_root = np.full(len(allrows), -1, dtype=np.int64)
    new_of_root[order] = np.arange(len(order))
    new_of = new_of_root[roots] if len(allrows) else roots
    out = np.zeros((len(order), VOF_BLOB_N))
    seen = np.zeros(len(order), dtype=bool)
    for x in range(len(allrows)):                                    # rank order
        r, o = allrows[x], out[new_of[x]]
        if not seen[new_of[x]]:
            o[:] = r
            seen[new_of[x]] = True
            continue
        o[CELLS] += r[CELLS]
        o[IMIN], o[JMIN] = min(o[IMIN], r[IMIN]), min(o[JMIN], r[JMIN])
        o[IMAX], o[JMAX] = max(o[IMAX], r[IMAX]), max(o[JMAX], r[JMAX])
        for k in SUMS:
            o[k] = o[k] + r[k]
    labels = []
    for k, (_, _, l) in enumerate(parts):
        m = np.full(l.shape, -1, dtype=np.int32)
        mem = l >= 0
        m[mem] = new_of[l[mem].astype(np.int64) + base[k]]
        labels.append(m)
    summary = {"BLOBS": len(out), "MEMBER_CELLS": sum(s["MEMBER_CELLS"] for _, s, _ in parts),
               "MAX_CELLS": int(out[:, CELLS].max()) if len(out) else 0, "ISTEP": parts[0][1]["ISTEP"]}
    return out, summary, np.concatenate(labels, axis=0)
