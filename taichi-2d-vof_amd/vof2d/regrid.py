"""vof_regrid: the slots of the summary and the factors two grids stand in (runtime/regrid_check.h, mirrored)."""
from . import _abi

PLIC = _abi.VOF_REGRID_PLIC
MAX_FACTOR = _abi.VOF_REGRID_MAX_FACTOR
SUMMARY = ("RX", "RY", "DIR", "PLIC_CELLS", "DEGENERATE", "F_SRC", "F_DST", "ISTEP")
assert len(SUMMARY) == _abi.VOF_REGRID_SUM_ISTEP + 1 <= _abi.VOF_REGRID_SUM_N


def summary_of(values):
    """The summary of vof_regrid as a dict keyed by SUMMARY."""
    return {name: values[k] for k, name in enumerate(SUMMARY)}


def factors(src_nx, src_ny, dst_nx, dst_ny):
    """(rx, ry, direction) of a state on src_nx x src_ny cells carried onto dst_nx x dst_ny: direction +1 refined, -1 coarsened,
    0 the same grid.  ValueError where vof_regrid answers VOF_EINVAL: the grids are refined along one axis and coarsened along
    the other, a ratio is no integer or is larger than MAX_FACTOR."""
    src_nx, src_ny, dst_nx, dst_ny = int(src_nx), int(src_ny), int(dst_nx), int(dst_ny)
    if min(src_nx, src_ny, dst_nx, dst_ny) < 1:
        raise ValueError("a grid has an extent < 1")
    up, down = dst_nx >= src_nx and dst_ny >= src_ny, dst_nx <= src_nx and dst_ny <= src_ny
    if not up and not down:
        raise ValueError("the grids are refined along one axis and coarsened along the other")
    (bx, sx), (by, sy) = ((dst_nx, src_nx), (dst_ny, src_ny)) if up else ((src_nx, dst_nx), (src_ny, dst_ny))
    if bx % sx or by % sy:
        raise ValueError("nx and ny of one grid must be integer multiples of the other's")
    rx, ry = bx // sx, by // sy
    if rx > MAX_FACTOR or ry > MAX_FACTOR:
        raise ValueError("a factor is larger than %d" % MAX_FACTOR)
    return rx, ry, (0 if rx == ry == 1 else (1 if up else -1))
