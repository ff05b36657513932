"""Flow diagnostics reduced on the device (vof_diagnostics, vof_step_diag; include/vof2d.h): the slots of a row, how the
partials of several strips combine, and the physical quantities a row stands for.

A row is VOF_DIAG_N doubles.  `Engine.diagnostics()` returns it as a dict keyed by NAMES; `Engine.step_diag()` returns an
(rows, VOF_DIAG_N) array whose rows `raw_of` turns into the same dict.
"""
import math

from ._abi import VOF_DIAG_N

ISTEP, SUM_F, SUM_FI, SUM_FJ, SUM_KE, SUM_DIV2, MAX_DIV, MAX_U, MAX_V, MIN_F, MAX_F, CELLS = range(12)
NAMES = ("ISTEP", "SUM_F", "SUM_FI", "SUM_FJ", "SUM_KE", "SUM_DIV2", "MAX_DIV", "MAX_U", "MAX_V", "MIN_F", "MAX_F", "CELLS")
SUMS = ("SUM_F", "SUM_FI", "SUM_FJ", "SUM_KE", "SUM_DIV2", "CELLS")
MAXIMA = ("MAX_DIV", "MAX_U", "MAX_V", "MAX_F")
DERIVED = ("volume", "xc", "yc", "kinetic_energy", "div_max", "div_l2", "u_max", "v_max", "cfl", "F_min", "F_max")


def raw_of(row):
    """One row (a sequence of VOF_DIAG_N doubles, or a dict already) as {name: value}."""
    if isinstance(row, dict):
        return row
    if len(row) != VOF_DIAG_N:
        raise ValueError("a row of diagnostics has %d values, not %d" % (VOF_DIAG_N, len(row)))
    return {name: float(row[k]) for k, name in enumerate(NAMES)}


def _max(a, b):
    """max in which a NaN counts as +inf (the convention of the kernels)."""
    return math.inf if (a != a or b != b) else max(a, b)


def combine(partials):
    """The row of the whole domain from the rows of its strips: sums (and CELLS) added in rank order, maxima by max,
    MIN_F by min; ISTEP must agree."""
    parts = [raw_of(p) for p in partials]
    if not parts:
        raise ValueError("combine needs at least one partial")
    out = dict(parts[0])
    for p in parts[1:]:
        if p["ISTEP"] != out["ISTEP"]:
            raise ValueError("partials of different steps: istep %r and %r" % (out["ISTEP"], p["ISTEP"]))
        for k in SUMS:
            out[k] = out[k] + p[k]
        for k in MAXIMA:
            out[k] = _max(out[k], p[k])
        out["MIN_F"] = -_max(-out["MIN_F"], -p["MIN_F"])
    # (a single partial goes through the same convention)
    for k in MAXIMA:
        out[k] = _max(out[k], out[k])
    out["MIN_F"] = -_max(-out["MIN_F"], -out["MIN_F"])
    return out


def derive(raw, dx, dy, dt, nx, ny):
    """What the sums and extrema stand for.  Cell (i, j) has its centre at ((i - 0.5) dx, (j - 0.5) dy).  An empty liquid
    (SUM_F == 0) has NaN centroids."""
    r = raw_of(raw)
    sum_f = r["SUM_F"]
    xc = (r["SUM_FI"] / sum_f - 0.5) * dx if sum_f != 0.0 else math.nan
    yc = (r["SUM_FJ"] / sum_f - 0.5) * dy if sum_f != 0.0 else math.nan
    cells = r["CELLS"]
    return {
        "volume": sum_f * dx * dy,
        "xc": xc,
        "yc": yc,
        "kinetic_energy": r["SUM_KE"] * dx * dy,
        "div_max": r["MAX_DIV"],
        "div_l2": math.sqrt(r["SUM_DIV2"] / cells) if cells > 0 and r["SUM_DIV2"] >= 0.0 else math.nan,
        "u_max": r["MAX_U"],
        "v_max": r["MAX_V"],
        "cfl": dt * max(r["MAX_U"] / dx, r["MAX_V"] / dy),
        "F_min": r["MIN_F"],
        "F_max": r["MAX_F"],
    }
