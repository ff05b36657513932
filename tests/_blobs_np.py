"""NumPy restatement of vof_blobs for the tests (include/vof2d.h; the order of the five sums as stated at the head of
taichi-2d-vof_amd/csrc/kernels/blobs.h, term for term).  Labelling is a flood fill over the member cells visited in ascending
(i, j) order, so a blob is numbered when its first cell is met: the definition, without reference to the device's algorithm.

`restate(F, u, v, phase, thr, ...)` takes the arrays as vof_get_field returns them (rows indexed [i - row0], ghost columns
included) and returns (rows, summary, labels) for the cells i in [lo, hi], j in [1, ny].
"""
import numpy as np

from _reduce_np import TILE

N = 16
I0, J0, CELLS, IMIN, IMAX, JMIN, JMAX, SUM_W, SUM_WI, SUM_WJ, SUM_WU, SUM_WV = range(12)
INTS = (I0, J0, CELLS, IMIN, IMAX, JMIN, JMAX)
SUMS = (SUM_W, SUM_WI, SUM_WJ, SUM_WU, SUM_WV)
CHUNK = 32            # kBlobRows
LIQUID, GAS = 0, 1


def members(F, phase, thr):
    with np.errstate(invalid="ignore"):
        return (F >= thr) if phase == LIQUID else (F < thr)       # a NaN is a member of neither


def label(mem):
    """Blob index of every cell of the boolean array `mem` (-1: not a member): 4-connected components, numbered in
    ascending order of their first cell in (i, j) order."""
    nr, nc = mem.shape
    lab = np.full((nr, nc), -1, dtype=np.int32)
    m = mem.tolist()
    n = 0
    for i0, j0 in zip(*np.nonzero(mem)):                           # row-major: ascending (i, j)
        if lab[i0, j0] >= 0:
            continue
        lab[i0, j0] = n
        stack = [(int(i0), int(j0))]
        while stack:
            i, j = stack.pop()
            for a, b in ((i - 1, j), (i + 1, j), (i, j - 1), (i, j + 1)):
                if 0 <= a < nr and 0 <= b < nc and m[a][b] and lab[a, b] < 0:
                    lab[a, b] = n
                    stack.append((a, b))
        n += 1
    return lab, n


def _lanes_to_wave(w):
    """wave_fold of kernels/reduce.h on (waves, 64, k) lane values: lane l takes l + s, s = 32 .. 1; lane 0's value."""
    s = 32
    while s > 0:
        new = w.copy()
        new[:, :64 - s] = w[:, :64 - s] + w[:, s:]
        w = new
        s >>= 1
    return w[:, 0]


def blob_sums(terms, match, imin, imax, jmin, jmax, lo):
    """The five sums of one blob: terms (rows lo .., columns 1 .. ny, 5), match the cells of the blob; the box in global
    indices.  Chunks of CHUNK rows from imin, the grid's column tiles the box touches, one wave per (chunk, tile)."""
    ny = terms.shape[1]
    t0, t1 = (jmin - 1) // TILE, (jmax - 1) // TILE
    nt = t1 - t0 + 1
    c0, c1 = t0 * TILE, min((t1 + 1) * TILE, ny)
    nrows = imax - imin + 1
    box = np.zeros((nrows, nt * TILE, 5))
    sel = match[imin - lo: imax + 1 - lo, c0:c1]
    box[:, :c1 - c0] = np.where(sel[:, :, None], terms[imin - lo: imax + 1 - lo, c0:c1], 0.0)   # (a skipped cell adds nothing: x + 0.0 has the bits of x here, the sums start from +0)
    box = box.reshape(nrows, nt, 64, 2, 5)
    nch = (nrows + CHUNK - 1) // CHUNK
    acc = np.zeros((nch, nt, 64, 5))
    for ch in range(nch):                                          # a lane adds its cells row by row, column by column
        for r in range(ch * CHUNK, min(ch * CHUNK + CHUNK, nrows)):
            acc[ch] = acc[ch] + box[r, :, :, 0]
            acc[ch] = acc[ch] + box[r, :, :, 1]
    part = _lanes_to_wave(acc.reshape(nch * nt, 64, 5))            # wave = chunk * tiles + tile
    lanes = np.zeros((64, 5))
    for start in range(0, len(part), 64):                          # lane l takes partials l, l + 64, ...
        blk = part[start:start + 64]
        lanes[:len(blk)] = lanes[:len(blk)] + blk
    return _lanes_to_wave(lanes[None])[0]


def cell_terms(F, u, v, phase, lo, hi, row0):
    """(rows lo .. hi, columns 1 .. ny, 5): w, w i, w j, w uc, w vc of every cell, the expressions of kernels/blobs.h."""
    F, u, v = (np.asarray(a).astype(np.float64) for a in (F, u, v))
    ny = F.shape[1] - 2
    r = slice(lo - row0, hi + 1 - row0)
    f = F[r, 1:ny + 1]
    with np.errstate(all="ignore"):
        Fc = np.fmin(np.fmax(f, 0.0), 1.0)
        w = Fc if phase == LIQUID else 1.0 - Fc
        uc = (u[r, 1:ny + 1] + u[lo - row0 + 1: hi + 2 - row0, 1:ny + 1]) * 0.5
        vc = (v[r, 1:ny + 1] + v[r, 2:ny + 2]) * 0.5
        di = np.arange(lo, hi + 1).astype(np.float64)[:, None]
        dj = np.arange(1, ny + 1).astype(np.float64)[None, :]
        return np.stack([w, w * di, w * dj, w * uc, w * vc], axis=2)


def restate(F, u, v, phase, thr, lo=1, hi=None, row0=0, sums=True):
    F64 = np.asarray(F).astype(np.float64)
    ny = F64.shape[1] - 2
    if hi is None:
        hi = F64.shape[0] - 2 + row0
    mem = members(F64[lo - row0: hi + 1 - row0, 1:ny + 1], phase, thr)
    lab, n = label(mem)
    rows = np.zeros((n, N))
    if n:
        ii, jj = np.nonzero(lab >= 0)
        l = lab[ii, jj]
        first = np.full(n, np.iinfo(np.int64).max)
        np.minimum.at(first, l, ii.astype(np.int64) * ny + jj)
        rows[:, I0], rows[:, J0] = lo + first // ny, 1 + first % ny
        rows[:, CELLS] = np.bincount(l, minlength=n)
        for slot, val, fn in ((IMIN, ii + lo, np.minimum), (IMAX, ii + lo, np.maximum), (JMIN, jj + 1, np.minimum), (JMAX, jj + 1, np.maximum)):
            a = np.full(n, val.max() + 1 if fn is np.minimum else -1, dtype=np.int64)
            fn.at(a, l, val)
            rows[:, slot] = a
        if sums:
            with np.errstate(all="ignore"):
                terms = cell_terms(F, u, v, phase, lo, hi, row0)
                for b in range(n):
                    r = rows[b]
                    rows[b, SUM_W:SUM_WV + 1] = blob_sums(terms, lab == b, int(r[IMIN]), int(r[IMAX]), int(r[JMIN]), int(r[JMAX]), lo)
    summary = {"BLOBS": n, "MEMBER_CELLS": int(mem.sum()), "MAX_CELLS": int(rows[:, CELLS].max()) if n else 0}
    return rows, summary, lab


# ---------------------------------------------------------------------------- constructed fields (interior cells, 1 = member of the liquid)
def checkerboard(nx, ny):
    return ((np.arange(nx)[:, None] + np.arange(ny)[None, :]) % 2 == 0).astype(np.float64)


def ring(nx, ny):
    """A closed ring of liquid two cells inside the walls, one cell thick: the gas is in 2 pieces, the liquid in 1."""
    m = np.zeros((nx, ny))
    m[2:nx - 2, 2:ny - 2] = 1.0
    m[3:nx - 3, 3:ny - 3] = 0.0
    return m


def comb(nx, ny):
    """A spine along j in row 1 and teeth along i in every other column; pairs of teeth are joined at the far
    end as well (loops: the unions meet sets that are one already): one blob.  The spine and some joins cross the column-tile boundaries."""
    m = np.zeros((nx, ny))
    m[0, :] = 1.0
    m[:nx - 2, ::2] = 1.0
    for j in range(2, ny - 2, 4):
        m[nx - 3, j:j + 3] = 1.0
    return m


def spiral(n):
    """A one-cell-wide square spiral from the corner inwards, gaps one cell wide: one blob, the longest chain per cell count."""
    m = np.zeros((n, n))
    i, j, di, dj = 0, 0, 0, 1
    m[0, 0] = 1.0
    while True:
        moved = False
        for _ in range(2):
            a, b = i + di, j + dj
            a2, b2 = a + di, b + dj
            ok = 0 <= a < n and 0 <= b < n and m[a, b] == 0 and not (0 <= a2 < n and 0 <= b2 < n and m[a2, b2] == 1)
            if ok:
                # the cell must not touch the spiral sideways either
                side = [(a + dj, b + di), (a - dj, b - di)]
                ok = all(not (0 <= p < n and 0 <= q < n and m[p, q] == 1) for p, q in side)
            if ok:
                i, j = a, b
                m[i, j] = 1.0
                moved = True
                break
            di, dj = dj, -di                                       # turn
        if not moved:
            return m


def with_ghosts(m):
    """(nx, ny) interior values -> the (nx + 2, ny + 2) array vof_set_field takes, ghost cells 0."""
    out = np.zeros((m.shape[0] + 2, m.shape[1] + 2))
    out[1:-1, 1:-1] = m
    return out
