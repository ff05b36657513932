"""The free-surface profile and fixed sensors read on the device (vof_depths, vof_gauges_set / _get, vof_step_gauges;
include/vof2d.h): the slots of a gauge's row and of the two summaries, the physical quantities the profile stands for, how
the profiles of several strips combine, and the lines of the command-line tool's CSV files.

`Engine.depths()` returns (depth_i, depth_j, top, summary); `Engine.gauges_get()` returns (rows, summary): a
(COUNT, VOF_GAUGE_N) float64 array in the order the gauges were given and a dict keyed by SUMMARY.
"""
import numpy as np

from ._abi import VOF_DEPTH_SUM_N, VOF_GAUGE_N, VOF_GAUGE_SUM_N

X, Y, U, V, F, P, DEPTH, TOP = range(8)
NAMES = ("X", "Y", "U", "V", "F", "P", "DEPTH", "TOP")
SUMMARY = ("COUNT", "ISTEP", "RECORDS")
DEPTH_SUMMARY = ("ROWS", "ISTEP", "FRONT_LO", "FRONT_HI", "TOP_J", "SUM")
GAUGES_CSV_HEADER = "istep,gauge," + ",".join(n.lower() for n in NAMES)
DEPTHS_CSV_HEADER = "istep,front_lo,front_hi,top,volume"
assert len(NAMES) == VOF_GAUGE_N


def summary_of(summ):
    """The gauges' summary (a sequence of VOF_GAUGE_SUM_N doubles, or a dict already) as {name: int}."""
    if isinstance(summ, dict):
        return summ
    if len(summ) != VOF_GAUGE_SUM_N:
        raise ValueError("a summary has %d values, not %d" % (VOF_GAUGE_SUM_N, len(summ)))
    return {name: int(summ[k]) for k, name in enumerate(SUMMARY)}


def depth_summary_of(summ):
    """The summary of vof_depths (a sequence of VOF_DEPTH_SUM_N doubles, or a dict already) as {name: value}: SUM a float,
    the rest ints."""
    if isinstance(summ, dict):
        return summ
    if len(summ) != VOF_DEPTH_SUM_N:
        raise ValueError("a summary has %d values, not %d" % (VOF_DEPTH_SUM_N, len(summ)))
    out = {name: float(summ[k]) for k, name in enumerate(DEPTH_SUMMARY)}
    out.update({k: int(out[k]) for k in DEPTH_SUMMARY if k != "SUM"})
    return out


def derive(depth_i, summary, dx, dy, first=1):
    """What the profile stands for.  Row r is the global row i = first + r; cell i covers [(i - 1) dx, i dx].
      x          the centres x_i = (i - 0.5) dx of the rows
      depth      depth_i * dy: the liquid depth over the floor at x_i, in metres
      front_lo   the left edge (FRONT_LO - 1) dx and
      front_hi   the right edge FRONT_HI dx of the wetted floor, in metres; NaN where the floor is dry
      volume     SUM dx dy"""
    s = depth_summary_of(summary)
    d = np.asarray(depth_i, dtype=np.float64)
    i = np.arange(first, first + len(d), dtype=np.float64)
    dry = s["FRONT_HI"] == 0
    return {
        "x": (i - 0.5) * dx,
        "depth": d * dy,
        "front_lo": float("nan") if dry else (s["FRONT_LO"] - 1) * dx,
        "front_hi": float("nan") if dry else s["FRONT_HI"] * dx,
        "volume": s["SUM"] * dx * dy,
    }


def combine(parts):
    """The profile of the whole domain from those of its strips, (depth_i, depth_j, top, summary) each, in rank order:
    depth_i and top concatenated, the depth_j partials and SUM added in rank order, ROWS added, the smallest non-zero
    FRONT_LO, the largest FRONT_HI and TOP_J; ISTEP must agree."""
    parts = [(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), np.asarray(c, dtype=np.int32), depth_summary_of(s)) for a, b, c, s in parts]
    if not parts:
        raise ValueError("combine needs at least one part")
    out = dict(parts[0][3])
    dj = parts[0][1].copy()
    for _, b, _, s in parts[1:]:
        if s["ISTEP"] != out["ISTEP"]:
            raise ValueError("parts of different steps: istep %r and %r" % (out["ISTEP"], s["ISTEP"]))
        if b.shape != dj.shape:
            raise ValueError("parts of different ny")
        dj = dj + b
        out["ROWS"] += s["ROWS"]
        out["SUM"] = out["SUM"] + s["SUM"]
        los = [v for v in (out["FRONT_LO"], s["FRONT_LO"]) if v != 0]
        out["FRONT_LO"] = min(los) if los else 0
        out["FRONT_HI"] = max(out["FRONT_HI"], s["FRONT_HI"])
        out["TOP_J"] = max(out["TOP_J"], s["TOP_J"])
    return np.concatenate([p[0] for p in parts]), dj, np.concatenate([p[2] for p in parts]), out


def parse_positions(pairs=(), path=None):
    """The (n, 2) positions of `--gauge X,Y` options followed by those of a `--gauges-file` (one `x y` per line; blank lines
    and lines that start with # are skipped)."""
    pts = []
    for text in pairs or ():
        xy = text.replace(",", " ").split()
        if len(xy) != 2:
            raise ValueError("a gauge is X,Y: %r" % (text,))
        pts.append((float(xy[0]), float(xy[1])))
    if path:
        with open(path) as f:
            for n, line in enumerate(f, 1):
                line = line.strip()
                if not line or line.startswith("#"):
                    continue
                xy = line.replace(",", " ").split()
                if len(xy) != 2:
                    raise ValueError("%s:%d: expected `x y`, got %r" % (path, n, line))
                pts.append((float(xy[0]), float(xy[1])))
    return np.array(pts, dtype=np.float64).reshape(-1, 2)


def gauges_csv_lines(istep, rows):
    """The lines of data/gauges.csv (GAUGES_CSV_HEADER) of one record: one per gauge."""
    return ["%d,%d,%s" % (istep, k, ",".join(repr(float(v)) for v in row)) for k, row in enumerate(np.asarray(rows, dtype=np.float64))]


def depths_csv_line(summary, dx, dy):
    """One line of data/depths.csv (DEPTHS_CSV_HEADER) from a summary of vof_depths."""
    s = depth_summary_of(summary)
    return "%d,%d,%d,%d,%r" % (s["ISTEP"], s["FRONT_LO"], s["FRONT_HI"], s["TOP_J"], s["SUM"] * dx * dy)
