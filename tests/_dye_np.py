"""NumPy restatements for the dye tests (vof_dye_*, vof_step_dye; include/vof2d.h).

1. The row of vof_dye_stats, term for term in the expression order stated at the head of k_dye_stats in
   taichi-2d-vof_amd/csrc/kernels/dye.h.  From the arrays C, F, u, v (ghost cells included) it returns the per-cell terms
   of every sum as float64 arrays, and the extrema.  Sums are judged against math.fsum of those terms with the bound of
   tests/_diag_np.py (n 2^-52 fsum|t|: any order of summing n doubles errs by at most (n - 1) 2^-53 sum|t| to first order;
   a factor of two for the higher-order terms) and -- where the caller names the chunk length R of the launch -- held bit
   for bit to the order of tests/_reduce_np.py: a lane holds columns 1 + 128 t + 2 l, + 1 of tile t and adds its cells
   row by row, column by column; k_row_finish folds with 256 threads.  Extrema, CELLS and ISTEP are compared with ==.

2. The twin oracle state that judges a transported dye: a NumPy oracle state (oracle/vof_oracle_np.py) whose F is the
   dye, whose u, v and istep are refreshed from the flow before every advance, and which goes through
   solve_VOF_rudman, post_process_f, set_BC -- the reference's own lines, with C for F.
"""
import math

import numpy as np

import vof_oracle_np as onp
from _diag_np import _max_nan_inf, bound_of
from _reduce_np import fixed_order

SUMS = ("SUM_C", "SUM_CI", "SUM_CJ", "SUM_C2", "SUM_CF", "SUM_CU", "SUM_CV")
EXTREMA = ("MIN_C", "MAX_C", "MAX_EXCESS")


def restate(C, F, u, v):
    """(terms, extrema, cells) over the interior cells i in [1, nx], j in [1, ny]."""
    nx, ny = C.shape[0] - 2, C.shape[1] - 2
    C, F, u, v = (np.asarray(a).astype(np.float64) for a in (C, F, u, v))
    I, J = slice(1, nx + 1), slice(1, ny + 1)
    c, f = C[I, J], F[I, J]
    uw, ue = u[I, J], u[2: nx + 2, J]
    vs, vn = v[I, J], v[I, 2: ny + 2]
    i = np.arange(1, nx + 1, dtype=np.float64)[:, None]
    j = np.arange(1, ny + 1, dtype=np.float64)[None, :]
    Fc = np.fmin(np.fmax(f, 0.0), 1.0)
    uc = (uw + ue) * 0.5
    vc = (vs + vn) * 0.5
    terms = {"SUM_C": c.copy(), "SUM_CI": c * i, "SUM_CJ": c * j, "SUM_C2": c * c, "SUM_CF": c * Fc, "SUM_CU": c * uc, "SUM_CV": c * vc}
    extrema = {"MIN_C": -_max_nan_inf(-c), "MAX_C": _max_nan_inf(c), "MAX_EXCESS": _max_nan_inf(c - f)}
    return terms, extrema, float(c.size)


def check(raw, terms, extrema, cells, istep=None, ctx="", say=None, R=None):
    """Hold a raw row (dict keyed by vof2d.dye.NAMES) to the restatement; every figure goes through `say` first.  R: the rows
    per wave chunk of the k_dye_stats launch (diag_chunk_rows of tests/_interface_np.py); with it every sum must also equal the
    fixed-order sum of its terms, bit for bit."""
    msgs = []
    for k in SUMS:
        t = terms[k].ravel()
        if np.isnan(t).any():
            ok = raw[k] != raw[k]
            line = "%s %s: %r, the terms hold a NaN" % (ctx, k, raw[k])
        else:
            exact, bound = math.fsum(t), bound_of(t)
            ok = abs(raw[k] - exact) <= bound
            line = "%s %s: %r, fsum %r, |d| %.3e, bound %.3e" % (ctx, k, raw[k], exact, abs(raw[k] - exact), bound)
            if R is not None:
                fixed = fixed_order(terms[k], R, 256, "add")
                ok = ok and raw[k] == fixed
                line += ", in the kernels' order %r" % fixed
        if say:
            say(line)
        if not ok:
            msgs.append(line)
    for k in EXTREMA:
        line = "%s %s: %r, restated %r" % (ctx, k, raw[k], extrema[k])
        if say:
            say(line)
        if not raw[k] == extrema[k]:
            msgs.append(line)
    if not raw["CELLS"] == cells:
        msgs.append("%s CELLS: %r, restated %r" % (ctx, raw["CELLS"], cells))
    if istep is not None and not raw["ISTEP"] == istep:
        msgs.append("%s ISTEP: %r, expected %r" % (ctx, raw["ISTEP"], istep))
    assert not msgs, " ; ".join(msgs)


def raw_from(terms, extrema, cells, istep=0):
    """A row as the device would report it, with the sums formed by np.sum (pairwise: one more order of summing)."""
    raw = {"ISTEP": float(istep), "CELLS": float(cells)}
    raw.update({k: float(np.sum(terms[k])) for k in SUMS})
    raw.update(extrema)
    return raw


def row_in_kernel_order(C, F, u, v, R, istep):
    """The 16 doubles of a row as the kernels form them (unused slots 0)."""
    from vof2d import dye
    terms, ext, cells = restate(C, F, u, v)
    row = np.zeros(16)
    row[dye.ISTEP], row[dye.CELLS] = float(istep), cells
    for k in SUMS:
        row[dye.NAMES.index(k)] = fixed_order(terms[k], R, 256, "add")
    for k in EXTREMA:
        row[dye.NAMES.index(k)] = ext[k]
    return row


class Twin:
    """The twin oracle state of a dye: a deep copy of nothing but the grid and constants of the flow, F := C."""

    def __init__(self, C, dtype, coord_cast="f32", **consts):
        C = np.asarray(C)
        self.s = onp.State(onp.Params(C.shape[0] - 2, C.shape[1] - 2, dtype=dtype, coord_cast=coord_cast, **consts))
        self.s.F[...] = C

    @property
    def C(self):
        return self.s.F

    def advance(self, u, v, istep):
        """One transport of the dye on the flow's final u, v of step istep."""
        s = self.s
        s.u[...] = u
        s.v[...] = v
        s.istep = int(istep)
        onp.solve_VOF_rudman(s)
        onp.post_process_f(s)
        onp.set_BC(s)
        return s.F
