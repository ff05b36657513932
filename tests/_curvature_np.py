"""NumPy restatement of vof_curvature for the tests, term for term in the expression order stated at the head of
taichi-2d-vof_amd/csrc/kernels/curvature.h; the order of the sums and extrema is that of tests/_reduce_np.py.  It is the yardstick for bits.

`restate(F, eps, dx, dy)` takes the whole-domain array F as vof_get_field returns it ((nx + 2, ny + 2), ghost cells included) and
returns (rows, summary): the (n, 8) float64 rows I, J, KAPPA, VALID, AXIS, KAPPA_CSF, HP, F in ascending (i, j) order and the summary as
a dict keyed by SUMMARY (ISTEP left out: the field does not know it).  Selects are np.where on exactly the kernel's comparison, so a NaN
takes the same branch.  tests/test_curvature.py judges this restatement against analysis.
"""
import numpy as np

from _interface_np import chunk_rows
from _reduce_np import fixed_order

SCAN_THREADS = 1024   # kScanThreads of kernels/cell_rows.h
I, J, KAPPA, VALID, AXIS, KAPPA_CSF, HP, FVAL = range(8)
SUMMARY = ("ROWS", "DEGENERATE", "VALID", "SUM_K", "SUM_K2", "MIN_K", "MAX_K", "SUM_CSF", "SUM_CSF2", "MIN_CSF", "MAX_CSF")


def restate(F, eps, dx, dy, R=None):
    F = np.asarray(F).astype(np.float64)
    nx, ny = F.shape[0] - 2, F.shape[1] - 2
    if R is None:
        R = chunk_rows(nx, ny)
    cx, cy, kx, ky = -1 / (2 * dx), -1 / (2 * dy), 1 / dx / 2, 1 / dy / 2
    P = 3
    Fp = np.pad(F, P, mode="edge")               # f(ii, jj) = F[clamp(ii), clamp(jj)]: the ghost layer repeated

    def f(di, dj):                               # f(i + di, j + dj) for every cell i in [1, nx], j in [1, ny]
        return Fp[P + 1 + di: P + 1 + di + nx, P + 1 + dj: P + 1 + dj + ny]

    with np.errstate(all="ignore"):
        F0 = f(0, 0)
        mixed = (eps < F0) & (F0 < 1.0 - eps)
        mx1 = cx * (((f(1, 1) + f(1, 0)) - f(0, 1)) - f(0, 0)); my1 = cy * (((f(1, 1) - f(1, 0)) + f(0, 1)) - f(0, 0))
        mx2 = cx * (((f(1, 0) + f(1, -1)) - f(0, 0)) - f(0, -1)); my2 = cy * (((f(1, 0) - f(1, -1)) + f(0, 0)) - f(0, -1))
        mx3 = cx * (((f(0, 0) + f(0, -1)) - f(-1, 0)) - f(-1, -1)); my3 = cy * (((f(0, 0) - f(0, -1)) + f(-1, 0)) - f(-1, -1))
        mx4 = cx * (((f(0, 1) + f(0, 0)) - f(-1, 1)) - f(-1, 0)); my4 = cy * (((f(0, 1) - f(0, 0)) + f(-1, 1)) - f(-1, 0))
        mxsum = (((mx1 + mx2) + mx3) + mx4) / 4      # S(a, b) of every interior cell
        mysum = (((my1 + my2) + my3) + my4) / 4
        degen = mixed & (np.abs(mxsum) < 1e-10) & (np.abs(mysum) < 1e-10)
        row = mixed & ~degen
        ax, by = np.abs(mxsum) * dx, np.abs(mysum) * dy
        along_i = ax > by
        m = np.where(along_i, mxsum, mysum)
        liquid_low = m >= 0                          # tl = -3

        def g(d, t):                                 # the cell t along the axis in column d
            return np.where(along_i, f(t, d), f(d, t))

        H, valid = [], np.ones_like(mixed)
        for d in (-1, 0, 1):
            h = g(d, -3)
            for t in (-2, -1, 0, 1, 2, 3):
                h = h + g(d, t)
            H.append(h)
            lo_end, hi_end = g(d, -3), g(d, 3)
            liq, gas = np.where(liquid_low, lo_end, hi_end), np.where(liquid_low, hi_end, lo_end)
            valid = valid & (liq >= 1.0 - eps) & (gas <= eps)
        hs, ht = np.where(along_i, dx, dy), np.where(along_i, dy, dx)
        hp = ((H[2] - H[0]) * hs) / (2 * ht)
        hpp = (((H[2] - 2 * H[1]) + H[0]) * hs) / (ht * ht)
        q = 1 + hp * hp
        kappa = hpp / (q * np.sqrt(q))
        kappa, hp = np.where(valid, kappa, 0.0), np.where(valid, hp, 0.0)
        # N(a, b): 0 outside [1, nx] x [1, ny]
        tiny = (np.abs(mxsum) < 1e-10) & (np.abs(mysum) < 1e-10)
        mag = np.sqrt(mxsum * mxsum + mysum * mysum)
        Nx = np.pad(np.where(tiny, mxsum, mxsum / mag), 1)
        Ny = np.pad(np.where(tiny, mysum, mysum / mag), 1)
        csf = -(kx * (Nx[2:, 1:-1] - Nx[:-2, 1:-1]) + ky * (Ny[1:-1, 2:] - Ny[1:-1, :-2]))

        ii, jj = np.nonzero(row)                     # row-major: ascending (i, j)
        rows = np.stack([(ii + 1).astype(np.float64), (jj + 1).astype(np.float64), kappa[ii, jj], valid[ii, jj].astype(np.float64),
                         along_i[ii, jj].astype(np.float64), csf[ii, jj], hp[ii, jj], F0[ii, jj]], axis=1).reshape(-1, 8)
        ok = row & valid

        def total(x, where):
            return fixed_order(np.where(where, x, 0.0), R, SCAN_THREADS, "add")

        def most(x, where):                          # a NaN operand counts as +inf (diag_max of kernels/reduce.h)
            return fixed_order(np.where(where, np.where(np.isnan(x), np.inf, x), -np.inf), R, SCAN_THREADS, "fmax")

        summary = {"ROWS": int(row.sum()), "DEGENERATE": int(degen.sum()), "VALID": int(ok.sum()),
                   "SUM_K": total(kappa, ok), "SUM_K2": total(kappa * kappa, ok), "MIN_K": -most(-kappa, ok), "MAX_K": most(kappa, ok),
                   "SUM_CSF": total(csf, row), "SUM_CSF2": total(csf * csf, row), "MIN_CSF": -most(-csf, row), "MAX_CSF": most(csf, row)}
    return rows, summary


# ---------------------------------------------------------------------------- fixtures: a disc integrated analytically
def _disc_cell_area(cx, cy, R, x0, x1, y0, y1):
    """Area of the disc of radius R about (cx, cy) inside the rectangle [x0, x1] x [y0, y1], exact up to rounding: the integral over x of
    clip(cy + s(x), y0, y1) - clip(cy - s(x), y0, y1), s = sqrt(R^2 - (x - cx)^2), split where an arc crosses y0 or y1."""
    a, b = max(x0, cx - R), min(x1, cx + R)
    if a >= b:
        return 0.0
    cuts = {a, b}
    for y in (y0, y1):
        if abs(y - cy) < R:
            w = np.sqrt(R * R - (y - cy) ** 2)
            cuts.update(x for x in (cx - w, cx + w) if a < x < b)
    cuts = sorted(cuts)

    def A(s):                                        # the antiderivative of sqrt(R^2 - s^2)
        s = min(max(s, -R), R)
        return 0.5 * (s * np.sqrt(max(R * R - s * s, 0.0)) + R * R * np.arcsin(s / R))

    area = 0.0
    for p, q in zip(cuts[:-1], cuts[1:]):
        mid = 0.5 * (p + q)
        s = np.sqrt(max(R * R - (mid - cx) ** 2, 0.0))
        arc = A(q - cx) - A(p - cx)
        for sign in (1.0, -1.0):
            gm = cy + sign * s
            part = y0 * (q - p) if gm <= y0 else y1 * (q - p) if gm >= y1 else cy * (q - p) + sign * arc
            area += sign * part
    return area


def disc(nx, ny, dx, dy, cx, cy, R):
    """F of (nx + 2, ny + 2) cells, ghost cells included (cells outside the domain are integrated like any other): the area fraction of
    the disc of radius R about (cx, cy) in every cell, cell (i, j) covering [(i - 1) dx, i dx] x [(j - 1) dy, j dy]."""
    F = np.zeros((nx + 2, ny + 2))
    for i in range(nx + 2):
        x0, x1 = (i - 1) * dx, i * dx
        for j in range(ny + 2):
            y0, y1 = (j - 1) * dy, j * dy
            near = np.hypot(max(x0 - cx, 0.0, cx - x1), max(y0 - cy, 0.0, cy - y1))
            far = np.hypot(max(abs(x0 - cx), abs(x1 - cx)), max(abs(y0 - cy), abs(y1 - cy)))
            F[i, j] = 0.0 if near >= R else 1.0 if far <= R else _disc_cell_area(cx, cy, R, x0, x1, y0, y1) / (dx * dy)
    return F
