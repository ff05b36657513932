"""Passive tracer particles moved with the flow on the device (vof_tracers_set / _advance / _get, vof_step_tracers;
include/vof2d.h): the slots of a row and of the summary, a lattice of start positions, seeding one phase.

`Engine.tracers()` returns (rows, summary): a (COUNT, VOF_TRACER_N) float64 array in the order the tracers were given and a
dict keyed by SUMMARY.  A lost tracer (a non-finite velocity met it) reads NaN in X, Y, U, V, F and is counted in LOST.
"""
import numpy as np

from ._abi import VOF_TRACER_N, VOF_TRACER_SUM_N

X, Y, U, V, F = range(5)
NAMES = ("X", "Y", "U", "V", "F")
SUMMARY = ("COUNT", "LOST", "IN_LIQUID", "ISTEP", "TIME")
COUNTS = ("COUNT", "LOST", "IN_LIQUID")
PHASES = ("liquid", "gas", "all")
CSV_HEADER = "istep,time,count,lost,in_liquid"


def summary_of(summ):
    """The summary (a sequence of VOF_TRACER_SUM_N doubles, or a dict already) as {name: value}; the counts and ISTEP as ints."""
    if isinstance(summ, dict):
        return summ
    if len(summ) != VOF_TRACER_SUM_N:
        raise ValueError("a summary has %d values, not %d" % (VOF_TRACER_SUM_N, len(summ)))
    out = {name: float(summ[k]) for k, name in enumerate(SUMMARY)}
    out.update({k: int(out[k]) for k in COUNTS + ("ISTEP",)})
    return out


def csv_line(summ):
    """One line of data/tracers.csv (CSV_HEADER) from a summary."""
    s = summary_of(summ)
    return "%d,%r,%d,%d,%d" % (s["ISTEP"], s["TIME"], s["COUNT"], s["LOST"], s["IN_LIQUID"])


def lattice(nx, ny, Lx, Ly, n):
    """About n points on a regular lattice, as an (mx * my, 2) float64 array of (x, y), x fastest.

    The lattice has mx x my boxes of the same shape as nearly as integers allow -- mx = round(sqrt(n Lx / Ly)) held to
    [1, n], my = round(n / mx) -- and a point at the centre of every box, ((p + 0.5) Lx / mx, (q + 0.5) Ly / my): the
    offsets of cell centres, strictly inside the domain.  The count mx * my lies within [n / 2, 3 n / 2]: my differs from
    n / mx by at most a half, so mx * my from n by at most mx / 2 <= n / 2.  A lattice finer than the grid is no use: mx
    is capped at nx and my at ny (one tracer per cell and direction), which lowers the count when it applies.  n < 1
    gives no points."""
    n = int(n)
    if n < 1:
        return np.zeros((0, 2), dtype=np.float64)
    if not (nx >= 1 and ny >= 1 and Lx > 0 and Ly > 0):
        raise ValueError("lattice needs nx, ny >= 1 and Lx, Ly > 0")
    mx = min(n, max(1, int(round(np.sqrt(n * float(Lx) / float(Ly))))))
    my = max(1, int(round(n / mx)))
    mx, my = min(mx, int(nx)), min(my, int(ny))
    xs = (np.arange(mx, dtype=np.float64) + 0.5) * (float(Lx) / mx)
    ys = (np.arange(my, dtype=np.float64) + 0.5) * (float(Ly) / my)
    out = np.empty((my, mx, 2), dtype=np.float64)
    out[:, :, 0] = xs[None, :]
    out[:, :, 1] = ys[:, None]
    return out.reshape(-1, 2)


def seed(engine, n, phase="liquid"):
    """Give `engine` the tracers of lattice(..., n) that start in `phase`: the lattice is set, F is read at its points through
    engine.tracers(), and the points with F >= 0.5 (liquid), F < 0.5 (gas) or all of them are set again (the selection is a
    host filter of one read-back: no compaction on the device).  Returns the (count, 2) positions kept."""
    if phase not in PHASES:
        raise ValueError("phase must be one of %s" % (PHASES,))
    pts = lattice(engine.nx, engine.ny, engine.get_param("Lx"), engine.get_param("Ly"), n)
    engine.tracers_set(pts)
    if phase != "all" and len(pts):
        rows, _ = engine.tracers()
        keep = rows[:, F] >= 0.5 if phase == "liquid" else rows[:, F] < 0.5
        pts = np.ascontiguousarray(rows[keep][:, [X, Y]])
        engine.tracers_set(pts)
    return pts
