"""Per-cell statistics over a run (vof_stats_*, vof_step_stats; include/vof2d.h): the groups, the planes in slot order, the
slots of the summary and the quantities the planes stand for.

A plane is an (nx, ny) float64 array indexed [i-1, j-1] (`Engine.stats_plane`); `Engine.stats_summary()` returns the summary
as a dict keyed by SUMMARY.  `derive` forms the means, variances, the Reynolds stress, the liquid-phase velocity, the wet
fraction, the largest speed and the arrival time from whatever planes it is given and the sample count.
"""
import numpy as np

from ._abi import VOF_STATS_ENVELOPE, VOF_STATS_MOMENTS, VOF_STATS_PLANES, VOF_STATS_SUM_N

MOMENTS, ENVELOPE = VOF_STATS_MOMENTS, VOF_STATS_ENVELOPE
GROUPS = {"MOMENTS": MOMENTS, "ENVELOPE": ENVELOPE}
PLANES = ("SUM_F", "SUM_F2", "SUM_U", "SUM_V", "SUM_UU", "SUM_VV", "SUM_UV", "SUM_FU", "SUM_FV", "MAX_F", "MAX_SPEED2", "WET", "ARRIVAL")
GROUP_PLANES = {MOMENTS: PLANES[:9], ENVELOPE: PLANES[9:]}
SUMMARY = ("SAMPLES", "ISTEP_FIRST", "ISTEP_LAST", "MASK", "LEVEL", "CELLS", "EVER_WET", "MAX_SPEED2")
DERIVED = {MOMENTS: ("F_mean", "u_mean", "v_mean", "F_var", "u_var", "v_var", "uv", "u_liquid", "v_liquid"),
           ENVELOPE: ("F_max", "max_speed", "wet_fraction", "arrival_time")}
assert len(PLANES) == VOF_STATS_PLANES


def mask_of(groups):
    """The mask of an int, a group name, a comma-separated string or a sequence of group names (any letter case)."""
    if isinstance(groups, (int, np.integer)):
        return int(groups)
    names = groups.split(",") if isinstance(groups, str) else list(groups)
    mask = 0
    for n in names:
        key = str(n).strip().upper()
        if key not in GROUPS:
            raise ValueError("unknown statistics group %r (known: %s)" % (n, ", ".join(GROUPS)))
        mask |= GROUPS[key]
    return mask


def slot_of(slot):
    """The slot number of a plane given by number or by name."""
    return PLANES.index(slot) if isinstance(slot, str) else int(slot)


def planes_of(mask):
    """The names of the planes of the groups in `mask`, in slot order."""
    return tuple(p for g in (MOMENTS, ENVELOPE) if mask & g for p in GROUP_PLANES[g])


def summary_of(row):
    """The summary (a sequence of VOF_STATS_SUM_N doubles, or a dict already) as {name: value}."""
    if isinstance(row, dict):
        return row
    if len(row) != VOF_STATS_SUM_N:
        raise ValueError("a summary of the statistics has %d values, not %d" % (VOF_STATS_SUM_N, len(row)))
    return {name: float(row[k]) for k, name in enumerate(SUMMARY)}


def derive(planes, samples, dt=1.0):
    """What the planes stand for after `samples` samples; planes: {name: (nx, ny) array}, of one group or of both.
      F_mean, u_mean, v_mean      S / N of the clamped F and of the cell-centred u, v
      F_var, u_var, v_var         max(S2 / N - mean^2, 0)
      uv                          the Reynolds stress u'v' = SUM_UV / N - u_mean v_mean
      u_liquid, v_liquid          the liquid-phase mean velocity SUM_FU / SUM_F, SUM_FV / SUM_F; NaN where SUM_F == 0
      F_max, max_speed            MAX_F, sqrt(MAX_SPEED2)
      wet_fraction                WET / N
      arrival_time                ARRIVAL * dt; NaN where the front never arrived
    Without a sample (N == 0) the quantities divided by N are NaN."""
    n = float(samples)
    out = {}
    with np.errstate(divide="ignore", invalid="ignore"):
        per = (lambda a: np.asarray(a, dtype=np.float64) / n) if n > 0 else (lambda a: np.full(np.shape(a), np.nan))
        if "SUM_F" in planes:
            sf = np.asarray(planes["SUM_F"], dtype=np.float64)
            fm, um, vm = per(sf), per(planes["SUM_U"]), per(planes["SUM_V"])
            out.update(F_mean=fm, u_mean=um, v_mean=vm,
                       F_var=np.maximum(per(planes["SUM_F2"]) - fm * fm, 0.0),
                       u_var=np.maximum(per(planes["SUM_UU"]) - um * um, 0.0),
                       v_var=np.maximum(per(planes["SUM_VV"]) - vm * vm, 0.0),
                       uv=per(planes["SUM_UV"]) - um * vm)
            dry = sf == 0.0
            safe = np.where(dry, 1.0, sf)
            out["u_liquid"] = np.where(dry, np.nan, np.asarray(planes["SUM_FU"], dtype=np.float64) / safe)
            out["v_liquid"] = np.where(dry, np.nan, np.asarray(planes["SUM_FV"], dtype=np.float64) / safe)
        if "ARRIVAL" in planes:
            arr = np.asarray(planes["ARRIVAL"], dtype=np.float64)
            out.update(F_max=np.asarray(planes["MAX_F"], dtype=np.float64), max_speed=np.sqrt(np.asarray(planes["MAX_SPEED2"], dtype=np.float64)),
                       wet_fraction=per(planes["WET"]), arrival_time=np.where(arr >= 0.0, arr * float(dt), np.nan))
    return out
