"""NumPy restatement of vof_depths and of a gauge's row for the tests, written from the comment blocks of include/vof2d.h and
from the order stated at the head of taichi-2d-vof_amd/csrc/kernels/depths.h.

`restate(F, ...)` takes the array F as vof_get_field returns it (rows indexed [i - row0], ghost columns included: ny + 2
columns) and returns the exact terms and integers: which cells are summed, the top of every row, the fronts.  Sums of the
terms are judged against math.fsum within n 2^-52 fsum(|t|) -- the bound of tests/_diag_np.py: summing n doubles in any
order errs by at most (n - 1) 2^-53 sum|t_i| to first order, a factor of two is left for the higher-order terms.

`ordered(...)` replays the stated lane / wave / tile / chunk order in float64, addition by addition (the sums are
additions only: contraction cannot change them), and is the yardstick for the bytes of depth_i, depth_j and SUM.

`gauge_rows(...)` restates a gauge's row with the sample of tests/_tracers_np.py (the expression the header states for the
tracers) and the depth_i / top it is given.
"""
import math

import numpy as np

import _tracers_np as tnp
from _interface_np import chunk_rows
from _reduce_np import TILE

SUM_N, GAUGE_N = 8, 8                                   # VOF_DEPTH_SUM_N, VOF_GAUGE_N
ROWS, ISTEP, FRONT_LO, FRONT_HI, TOP_J, SUM = range(6)   # slots of the summary
X, Y, U, V, F, P, DEPTH, TOP = range(8)                  # slots of a gauge's row


def depths_chunk_rows(nx, ny, row_lo=0, row_hi=None):
    """depths_chunk_rows of runtime/rows.h: the cells-per-wave rule with 2 and 32 on the rows the handle can compute."""
    return chunk_rows(nx, ny, row_lo, row_hi, rmin=2, rmax=32)


def partial_counts(rows, ny, R):
    """(partials per (row, tile), partials per (chunk, column)) of a pass over `rows` rows in chunks of R."""
    return rows * ((ny + TILE - 1) // TILE), (rows + R - 1) // R * ny


def restate(Farr, lo=1, hi=None, row0=0):
    """The exact content of vof_depths over the cells i in [lo, hi], j in [1, ny]:
    terms  (rows, ny) float64, the (double)F[i,j] that depth_i sums along j and depth_j along i
    top    (rows,) int32, the largest j with F[i,j] >= 0.5, 0 if none (a NaN is not a member)
    front_lo, front_hi  the smallest / largest i with F[i,1] >= 0.5, 0 if none;  top_j = max(top), 0 over no rows."""
    Fd = np.asarray(Farr).astype(np.float64)
    ny = Fd.shape[1] - 2
    if hi is None:
        hi = Fd.shape[0] - 2 + row0
    terms = Fd[lo - row0: hi + 1 - row0, 1: ny + 1].copy() if hi >= lo else np.zeros((0, ny))
    with np.errstate(invalid="ignore"):
        member = terms >= 0.5
    j = np.arange(1, ny + 1, dtype=np.int32)[None, :]
    top = np.where(member, j, 0).max(axis=1).astype(np.int32) if len(terms) else np.zeros(0, dtype=np.int32)
    wet = np.nonzero(member[:, 0])[0] + lo if len(terms) else np.zeros(0, dtype=int)
    return {"terms": terms, "top": top, "front_lo": int(wet.min()) if len(wet) else 0, "front_hi": int(wet.max()) if len(wet) else 0,
            "top_j": int(top.max()) if len(top) else 0, "rows": len(terms), "first": lo}


def ordered(terms, R):
    """(depth_i, depth_j, SUM) in the order kernels/depths.h states, from the (rows, ny) terms and the chunk length R."""
    t = np.asarray(terms, dtype=np.float64)
    rows, ny = t.shape
    ntj = (ny + TILE - 1) // TILE
    # depth_i 1.: a lane adds its two columns to 0.0 (a column > ny adds nothing)
    lane = np.zeros((rows, ntj * 64))
    for q in range(2):
        cols = np.arange(q, ntj * TILE, 2)
        ok = cols < ny
        add = np.zeros((rows, ntj * 64))
        add[:, ok] = t[:, cols[ok]]
        lane = np.where(ok[None, :], lane + add, lane)
    # 2.: lanes -> wave by __shfl_down, s = 32 .. 1: lane l takes l + s
    w = lane.reshape(rows, ntj, 64)
    s = 32
    while s > 0:
        new = w.copy()
        new[:, :, :64 - s] = w[:, :, :64 - s] + w[:, :, s:]
        w = new
        s >>= 1
    part = w[:, :, 0]
    # 3.: the tiles of a row in ascending order, starting from tile 0's partial
    depth_i = part[:, 0].copy() if rows else np.zeros(0)
    for k in range(1, ntj):
        depth_i = depth_i + part[:, k]
    # depth_j 1.: a lane adds the rows of its chunk to 0.0, ascending; 2.: the chunks to 0.0, ascending
    depth_j = np.zeros(ny)
    for c0 in range(0, rows, R):
        col = np.zeros(ny)
        for r in range(c0, min(c0 + R, rows)):
            col = col + t[r]
        depth_j = depth_j + col
    # SUM: one row after the other
    total = 0.0
    for d in depth_i.tolist():
        total = total + d
    return depth_i, depth_j, total


def bound_of(t):
    """n 2^-52 fsum(|t|): what any order of summing the n terms t may differ from their exact sum by."""
    t = np.asarray(t, dtype=np.float64).ravel()
    return t.size * 2.0 ** -52 * math.fsum(np.abs(t))


def within_bound(value, t):
    """value is the sum of the terms t in some order: NaN if a term is, else within bound_of(t) of math.fsum(t)."""
    t = np.asarray(t, dtype=np.float64).ravel()
    if np.isnan(t).any():
        return value != value
    return abs(value - math.fsum(t)) <= bound_of(t)


def summary(res, total, istep):
    """The SUM_N doubles of the summary from restate()'s result and the ordered SUM."""
    s = np.zeros(SUM_N, dtype=np.float64)
    s[ROWS], s[ISTEP], s[FRONT_LO], s[FRONT_HI], s[TOP_J], s[SUM] = res["rows"], istep, res["front_lo"], res["front_hi"], res["top_j"], total
    return s


def gauge_rows(Fa, ua, va, pa, xy, g, depth_i, top, dy):
    """The (n, GAUGE_N) rows of the gauges at the (n, 2) positions xy on a whole domain: X, Y; U, V, F the tracers' samples;
    P sampled with F's offsets and clamps; DEPTH = depth_i[ig] * dy and TOP = top[ig], ig = floor(X * dxi) + 1 held to [1, nx]."""
    Ff, u, v = tnp.fields(Fa, ua, va)
    pf = tnp.Field("F", pa)                # (F's offsets (0.5, 0.5) and clamps)
    out = np.zeros((len(xy), GAUGE_N), dtype=np.float64)
    for k, (x, y) in enumerate(np.asarray(xy, dtype=np.float64).tolist()):
        ig = math.floor(x * g.dxi) + 1
        ig = 1 if ig < 1 else (g.nx if ig > g.nx else ig)
        out[k] = (x, y, tnp.sample(u, x, y, g), tnp.sample(v, x, y, g), tnp.sample(Ff, x, y, g), tnp.sample(pf, x, y, g),
                  float(depth_i[ig - 1]) * dy, float(top[ig - 1]))
    return out
