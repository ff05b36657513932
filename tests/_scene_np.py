"""vof_set_scene restated in NumPy from the text of include/vof2d.h: every cell sampled in full against every shape, no shortcut,
float64 throughout, one rounding to the field type at the end.  NumPy's elementwise +, -, * round each result on its own, which is
the order the header fixes; a comparison with a NaN is false here as there.  The judge of tests/test_scene*.py.
"""
import numpy as np

N = 8                                    # VOF_SHAPE_N
BOX, ELLIPSE, HALFPLANE, TRIANGLE = range(4)
GAS, LIQUID, KEEP = 0, 1, 2
BAND = 32                                # rows sampled at a time (memory only)


def coords(cells, S, d):
    """(len(cells), S): ((double)(cell - 1) + ((double)a + 0.5) * (1.0 / S)) * d"""
    frac = (np.arange(S, dtype=np.float64) + 0.5) * (1.0 / S)
    return ((np.asarray(cells, dtype=np.float64) - 1.0)[:, None] + frac[None, :]) * np.float64(d)


def _local(a, xs, ys):
    cx, cy, c, s = a[0], a[1], a[4], a[5]
    px, py = xs - cx, ys - cy
    return px * c + py * s, py * c - px * s


def inside(rec, xs, ys):
    """The closed inside test of one record at the samples xs (n, 1) x ys (1, m); (n, m) bools."""
    kind, a = int(rec[0]), [np.float64(x) for x in rec[2:]]
    if kind == BOX:
        lx, ly = _local(a, xs, ys)
        return (np.abs(lx) <= a[2]) & (np.abs(ly) <= a[3])
    if kind == ELLIPSE:
        lx, ly = _local(a, xs, ys)
        t1, t2, t3 = lx * a[3], ly * a[2], a[2] * a[3]
        return t1 * t1 + t2 * t2 <= t3 * t3
    if kind == HALFPLANE:
        return (xs - a[0]) * a[2] + (ys - a[1]) * a[3] <= 0.0
    if kind == TRIANGLE:
        x0, y0, x1, y1, x2, y2 = a
        e0 = (x1 - x0) * (ys - y0) - (y1 - y0) * (xs - x0)
        e1 = (x2 - x1) * (ys - y1) - (y2 - y1) * (xs - x1)
        e2 = (x0 - x2) * (ys - y2) - (y0 - y2) * (xs - x2)
        return ((e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)) | ((e0 <= 0.0) & (e1 <= 0.0) & (e2 <= 0.0))
    raise ValueError("unknown kind %r" % (rec[0],))


def counts(recs, S, dx, dy, rows, ncols):
    """(n_liq, n_keep) of the cells (i, j), i in rows, j in [0, ncols): the samples that ended LIQUID, KEEP."""
    rows = np.asarray(rows)
    n_liq = np.zeros((len(rows), ncols), dtype=np.int64)
    n_keep = np.zeros((len(rows), ncols), dtype=np.int64)
    ys = coords(np.arange(ncols), S, dy).reshape(1, -1)
    with np.errstate(all="ignore"):
        for r0 in range(0, len(rows), BAND):
            band = rows[r0:r0 + BAND]
            xs = coords(band, S, dx).reshape(-1, 1)
            state = np.full((len(band) * S, ncols * S), KEEP, dtype=np.int8)
            for rec in recs:
                state[inside(rec, xs, ys)] = int(rec[1])
            st = state.reshape(len(band), S, ncols, S)
            n_liq[r0:r0 + BAND] = (st == LIQUID).sum(axis=(1, 3))
            n_keep[r0:r0 + BAND] = (st == KEEP).sum(axis=(1, 3))
    return n_liq, n_keep


def paint(F, recs, S, clear, dx, dy, row_lo=0, reported=None, sampled=None):
    """vof_set_scene on the stored rows F (rows row_lo .. row_lo + len(F) - 1, columns 0 .. ny + 1) of either dtype: (the new
    array, PAINTED, MIXED).  reported: the first and last row the handle counts (default: the interior rows of a whole domain).
    sampled: what counts() gave for these rows, shapes and spacings before (the field and the flag do not enter it)."""
    nrows, ncols = F.shape
    ny = ncols - 2
    rows = row_lo + np.arange(nrows)
    recs = np.asarray(recs, dtype=np.float64).reshape(-1, N)
    total = S * S
    n_liq, n_keep = sampled if sampled is not None else counts(recs, S, dx, dy, rows, ncols)
    if clear:
        n_keep = np.zeros_like(n_keep)
    n_gas = total - n_liq - n_keep
    write = n_keep < total
    with np.errstate(all="ignore"):
        old = np.where(n_keep > 0, F.astype(np.float64), 0.0)         # (not read where n_keep == 0)
        acc = np.where(n_keep > 0, n_liq.astype(np.float64) + n_keep.astype(np.float64) * old, n_liq.astype(np.float64))
        val = (acc * (1.0 / total)).astype(F.dtype)
    out = F.copy()
    out[write] = val[write]
    mixed = (n_liq != total) & (n_gas != total) & (n_keep != total)
    lo, hi = reported if reported is not None else (max(row_lo + 1, 1), row_lo + nrows - 2)
    counted = ((rows >= lo) & (rows <= hi))[:, None] & ((np.arange(ncols) >= 1) & (np.arange(ncols) <= ny))[None, :]
    return out, int((write & counted).sum()), int((mixed & counted).sum())
