"""A dye carried by the transport of F (vof_dye_*, vof_step_dye; include/vof2d.h): the slots of a row of statistics, the
physical quantities a row stands for, and a helper that seeds a dye from F inside a box.

A row is VOF_DYE_N doubles.  `Engine.dye_stats()` returns it as a dict keyed by NAMES; `Engine.step_dye()` returns an
(rows, VOF_DYE_N) array whose rows `raw_of` turns into the same dict.
"""
import math

import numpy as np

from ._abi import VOF_DYE_N

ISTEP, CELLS, SUM_C, SUM_CI, SUM_CJ, SUM_C2, SUM_CF, SUM_CU, SUM_CV, MIN_C, MAX_C, MAX_EXCESS = range(12)
NAMES = ("ISTEP", "CELLS", "SUM_C", "SUM_CI", "SUM_CJ", "SUM_C2", "SUM_CF", "SUM_CU", "SUM_CV", "MIN_C", "MAX_C", "MAX_EXCESS")
DERIVED = ("amount", "xc", "yc", "mean", "variance", "outside_liquid", "u", "v", "C_min", "C_max", "excess_max")


def raw_of(row):
    """One row (a sequence of VOF_DYE_N doubles, or a dict already) as {name: value}."""
    if isinstance(row, dict):
        return row
    if len(row) != VOF_DYE_N:
        raise ValueError("a row of dye statistics has %d values, not %d" % (VOF_DYE_N, len(row)))
    return {name: float(row[k]) for k, name in enumerate(NAMES)}


def derive(raw, dx, dy):
    """What the sums and extrema stand for.  Cell (i, j) has its centre at ((i - 0.5) dx, (j - 0.5) dy).  Without dye
    (SUM_C == 0) the centroid, the share outside the liquid and the dye's velocity are NaN.
      amount          the dye's area integral, SUM_C dx dy
      xc, yc          its centroid
      mean, variance  of C over the cells (variance = <C^2> - <C>^2: 0 for a uniform dye, largest for an unmixed one)
      outside_liquid  1 - SUM_CF / SUM_C: the share of the dye that sits where there is no liquid
      u, v            the dye-weighted mean velocity, SUM_CU / SUM_C and SUM_CV / SUM_C
    """
    r = raw_of(raw)
    s, cells = r["SUM_C"], r["CELLS"]
    per = (lambda x: x / s) if s != 0.0 else (lambda x: math.nan)
    mean = s / cells if cells > 0 else math.nan
    return {
        "amount": s * dx * dy,
        "xc": (per(r["SUM_CI"]) - 0.5) * dx,
        "yc": (per(r["SUM_CJ"]) - 0.5) * dy,
        "mean": mean,
        "variance": r["SUM_C2"] / cells - mean * mean if cells > 0 else math.nan,
        "outside_liquid": 1.0 - per(r["SUM_CF"]),
        "u": per(r["SUM_CU"]),
        "v": per(r["SUM_CV"]),
        "C_min": r["MIN_C"],
        "C_max": r["MAX_C"],
        "excess_max": r["MAX_EXCESS"],
    }


def box(F, dx, dy, x0, x1, y0, y1):
    """A dye equal to F inside the physical box [x0, x1] x [y0, y1] and 0 elsewhere; F is the (nx+2, ny+2) field, ghost
    cells included, and a cell belongs to the box if its centre ((i - 0.5) dx, (j - 0.5) dy) lies in it (ghost cells
    have their centres outside the domain and are judged the same way)."""
    F = np.asarray(F)
    xc = (np.arange(F.shape[0], dtype=np.float64) - 0.5) * float(dx)
    yc = (np.arange(F.shape[1], dtype=np.float64) - 0.5) * float(dy)
    inside = ((xc >= x0) & (xc <= x1))[:, None] & ((yc >= y0) & (yc <= y1))[None, :]
    return np.where(inside, F, F.dtype.type(0))


def boxes(F, dx, dy, rects):
    """The union of several boxes: F inside any of the (x0, x1, y0, y1) of rects, 0 elsewhere."""
    out = np.zeros_like(np.asarray(F))
    for (x0, x1, y0, y1) in rects:
        out = np.maximum(out, box(F, dx, dy, x0, x1, y0, y1))
    return out
