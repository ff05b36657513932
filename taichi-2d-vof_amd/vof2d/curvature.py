"""Height-function curvature of the interface beside the solver's own (vof_curvature; include/vof2d.h): the slots of a row and of
the summary, the quantities derived from the summary and the line of data/curvature.csv.

`Engine.curvature()` returns (rows, summary): an (n, VOF_CURV_N) float64 array in ascending (i, j) order -- the cells and the order of
`Engine.interface()` at the same eps -- and a dict keyed by SUMMARY.  KAPPA is the height-function curvature (0 where VALID is 0),
KAPPA_CSF the solver's own -div of Youngs' normals at the cell; both carry the solver's sign: -1/R for a drop, +1/R for a bubble.
"""
import math

from ._abi import VOF_CURV_N, VOF_CURV_SUM_N

I, J, KAPPA, VALID, AXIS, KAPPA_CSF, HP, F = range(VOF_CURV_N)
NAMES = ("I", "J", "KAPPA", "VALID", "AXIS", "KAPPA_CSF", "HP", "F")
SUMMARY = ("ROWS", "DEGENERATE", "VALID", "SUM_K", "SUM_K2", "MIN_K", "MAX_K", "SUM_CSF", "SUM_CSF2", "MIN_CSF", "MAX_CSF", "ISTEP")
COUNTS = ("ROWS", "DEGENERATE", "VALID", "ISTEP")
DERIVED = ("rows", "degenerate", "valid", "valid_share", "k_mean", "k_rms", "k_min", "k_max", "csf_mean", "csf_rms", "csf_min", "csf_max")
CSV_HEADER = ",".join(("istep",) + DERIVED)


def summary_of(summ):
    """The summary (a sequence of VOF_CURV_SUM_N doubles, or a dict already) as {name: value}; the counts as ints."""
    if isinstance(summ, dict):
        return summ
    if len(summ) != VOF_CURV_SUM_N:
        raise ValueError("a summary has %d values, not %d" % (VOF_CURV_SUM_N, len(summ)))
    out = {name: float(summ[k]) for k, name in enumerate(SUMMARY)}
    out.update({k: int(out[k]) for k in COUNTS})
    return out


def derive(summ):
    """Mean, rms, minimum and maximum of KAPPA over the valid rows and of KAPPA_CSF over all rows, and the share of the rows that
    are valid.  Where there is no operand the value is nan (the summary's own -inf / +inf say the same less plainly)."""
    s = summary_of(summ)
    rows, valid = s["ROWS"], s["VALID"]

    def moments(n, total, squares, least, most):
        if n == 0:
            return (math.nan,) * 4
        return total / n, math.sqrt(squares / n), least, most

    k = moments(valid, s["SUM_K"], s["SUM_K2"], s["MIN_K"], s["MAX_K"])
    c = moments(rows, s["SUM_CSF"], s["SUM_CSF2"], s["MIN_CSF"], s["MAX_CSF"])
    out = {"rows": rows, "degenerate": s["DEGENERATE"], "valid": valid, "valid_share": valid / rows if rows else math.nan}
    out.update(zip(("k_mean", "k_rms", "k_min", "k_max"), k))
    out.update(zip(("csf_mean", "csf_rms", "csf_min", "csf_max"), c))
    return out


def csv_line(summ):
    """The line of data/curvature.csv for this summary: istep, then DERIVED (the counts as integers, the rest by repr)."""
    s = summary_of(summ)
    d = derive(s)
    return ",".join([str(s["ISTEP"])] + [str(d[k]) if k in ("rows", "degenerate", "valid") else repr(float(d[k])) for k in DERIVED])
