"""NumPy restatement of vof_interface for the tests, term for term in the expression order stated at the head of
taichi-2d-vof_amd/csrc/kernels/interface.h; the order of the LENGTH sum is that of tests/_reduce_np.py.  It is the yardstick for bits.

`restate(F, eps, dx, dy, ...)` takes the array F as vof_get_field returns it (rows indexed [i - row0], ghost columns
included: ny + 2 columns) and returns (rows, summary, unit): the (n, 8) float64 rows in ascending (i, j) order, the summary
{"SEGMENTS", "DEGENERATE", "LENGTH"} and, for the geometric tests, the end points in unit-cell coordinates, (n, 4) =
(xi0, eta0, xi1, eta1) in the order of the row.  Selects are np.where on exactly the kernel's comparison, so a NaN takes
the same branch.
"""
import numpy as np

from _reduce_np import TILE, fixed_order

SCAN_THREADS = 1024   # kScanThreads of kernels/cell_rows.h


def chunk_rows(nx, ny, row_lo=0, row_hi=None, rmin=4, rmax=32):
    """cell_rows_chunk of runtime/cell_rows.h: the cells-per-wave rule on the rows the handle can compute."""
    row_hi = nx + 1 if row_hi is None else row_hi
    rows = min(nx, row_hi - 1) - max(1, row_lo + 1) + 1
    ntj = (ny + TILE - 1) // TILE
    R = min(max(rows * ntj // 4096, rmin), rmax)
    P = 1
    while P * 2 <= R:
        P *= 2
    return max(P, rmin)


def diag_chunk_rows(nx, ny, row_lo=0, row_hi=None):
    """diag_chunk of runtime/diag_reduce.h: the same rule with 2 and 16."""
    return chunk_rows(nx, ny, row_lo, row_hi, rmin=2, rmax=16)


def length_sum(L, R):
    """The LENGTH of the kernels from the per-cell lengths L (rows lo .. hi, columns 1 .. ny; 0 where there is no segment):
    the order of kernels/reduce.h with the 1024 threads of k_cell_rows_scan."""
    return fixed_order(L, R, SCAN_THREADS, "add")


def restate(F, eps, dx, dy, lo=1, hi=None, row0=0, R=None):
    F = np.asarray(F).astype(np.float64)
    ny = F.shape[1] - 2
    if hi is None:
        hi = F.shape[0] - 2 + row0
    if R is None:
        R = chunk_rows(F.shape[0] - 2, ny)
    cx, cy = -1 / (2 * dx), -1 / (2 * dy)
    I = np.arange(lo, hi + 1)

    def f(di, dj):
        return F[lo - row0 + di: hi + 1 - row0 + di, 1 + dj: ny + 1 + dj]

    with np.errstate(all="ignore"):
        F0 = f(0, 0)
        mixed = (eps < F0) & (F0 < 1.0 - eps)
        mx1 = cx * (((f(1, 1) + f(1, 0)) - f(0, 1)) - f(0, 0)); my1 = cy * (((f(1, 1) - f(1, 0)) + f(0, 1)) - f(0, 0))
        mx2 = cx * (((f(1, 0) + f(1, -1)) - f(0, 0)) - f(0, -1)); my2 = cy * (((f(1, 0) - f(1, -1)) + f(0, 0)) - f(0, -1))
        mx3 = cx * (((f(0, 0) + f(0, -1)) - f(-1, 0)) - f(-1, -1)); my3 = cy * (((f(0, 0) - f(0, -1)) + f(-1, 0)) - f(-1, -1))
        mx4 = cx * (((f(0, 1) + f(0, 0)) - f(-1, 1)) - f(-1, 0)); my4 = cy * (((f(0, 1) - f(0, 0)) + f(-1, 1)) - f(-1, 0))
        mxsum = (((mx1 + mx2) + mx3) + mx4) / 4
        mysum = (((my1 + my2) + my3) + my4) / 4
        degen = mixed & (np.abs(mxsum) < 1e-10) & (np.abs(mysum) < 1e-10)
        seg = mixed & ~degen
        ax, by = np.abs(mxsum) * dx, np.abs(mysum) * dy
        s = ax + by
        a, b = ax / s, by / s
        n1, n2 = np.where(a < b, a, b), np.where(a < b, b, a)
        Fm = np.where(F0 <= 0.5, F0, 1.0 - F0)
        alpha = np.where((2.0 * n2) * Fm < n1, np.sqrt(((2.0 * n1) * n2) * Fm), n2 * Fm + n1 * 0.5)
        alpha = np.where(F0 > 0.5, 1.0 - alpha, alpha)
        p_left, q_bottom = (b > 0.0) & (alpha <= b), (a > 0.0) & (alpha <= a)
        pxi, peta = np.where(p_left, 0.0, (alpha - b) / a), np.where(p_left, alpha / b, 1.0)
        qxi, qeta = np.where(q_bottom, alpha / a, 1.0), np.where(q_bottom, 0.0, (alpha - a) / b)
        flip_x, flip_y = mxsum < 0.0, mysum < 0.0
        pxi, qxi = np.where(flip_x, 1.0 - pxi, pxi), np.where(flip_x, 1.0 - qxi, qxi)
        peta, qeta = np.where(flip_y, 1.0 - peta, peta), np.where(flip_y, 1.0 - qeta, qeta)
        di = (I - 1).astype(np.float64)[:, None]
        dj = (np.arange(1, ny + 1) - 1).astype(np.float64)[None, :]
        px, py, qx, qy = (di + pxi) * dx, (dj + peta) * dy, (di + qxi) * dx, (dj + qeta) * dy
        p_first = flip_x != flip_y
        mag = np.sqrt(mxsum * mxsum + mysum * mysum)
        X0, Y0 = np.where(p_first, px, qx), np.where(p_first, py, qy)
        X1, Y1 = np.where(p_first, qx, px), np.where(p_first, qy, py)
        NX, NY = mxsum / mag, mysum / mag
        ddx, ddy = X1 - X0, Y1 - Y0
        length = np.where(seg, np.sqrt(ddx * ddx + ddy * ddy), 0.0)
        u0 = np.where(p_first, pxi, qxi), np.where(p_first, peta, qeta)
        u1 = np.where(p_first, qxi, pxi), np.where(p_first, qeta, peta)
    ii, jj = np.nonzero(seg)                   # row-major: ascending (i, j)
    rows = np.stack([(ii + lo).astype(np.float64), (jj + 1).astype(np.float64), X0[ii, jj], Y0[ii, jj], X1[ii, jj], Y1[ii, jj],
                     NX[ii, jj], NY[ii, jj]], axis=1).reshape(-1, 8)
    unit = np.stack([u0[0][ii, jj], u0[1][ii, jj], u1[0][ii, jj], u1[1][ii, jj]], axis=1).reshape(-1, 4)
    summary = {"SEGMENTS": int(seg.sum()), "DEGENERATE": int(degen.sum()),
               "LENGTH": length_sum(length, R) if hi >= lo else 0.0}
    return rows, summary, unit


# ---------------------------------------------------------------------------- fixtures for the geometric tests
def supersampled(nx, ny, Lx, Ly, inside, n=16):
    """F of (nx + 2, ny + 2) cells, ghosts included (cells outside the domain are sampled like any other), from n x n
    sample points per cell of the indicator `inside(x, y)`."""
    dx, dy = Lx / nx, Ly / ny
    o = (np.arange(n) + 0.5) / n
    x = ((np.arange(nx + 2) - 1)[:, None] + o[None, :]).reshape(-1) * dx
    y = ((np.arange(ny + 2) - 1)[:, None] + o[None, :]).reshape(-1) * dy
    m = inside(x[:, None], y[None, :]).astype(np.float64)
    return m.reshape(nx + 2, n, ny + 2, n).mean(axis=(1, 3)), dx, dy


def clipped_area(a, b, alpha):
    """Area of the unit square inside the half-plane a xi + b eta < alpha (Sutherland-Hodgman, one clip)."""
    sq = [(0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0)]
    d = [a * x + b * y - alpha for x, y in sq]
    poly = []
    for k in range(4):
        p, q, dp, dq = sq[k], sq[(k + 1) % 4], d[k], d[(k + 1) % 4]
        if dp <= 0:
            poly.append(p)
        if (dp < 0 < dq) or (dq < 0 < dp):
            t = dp / (dp - dq)
            poly.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
    area = 0.0
    for k in range(len(poly)):
        (x0, y0), (x1, y1) = poly[k], poly[(k + 1) % len(poly)]
        area += x0 * y1 - x1 * y0
    return 0.5 * area
