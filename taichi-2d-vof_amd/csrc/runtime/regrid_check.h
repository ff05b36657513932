// runtime/regrid_check.h -- vof_regrid: the factors two grids stand in, and what is refused before anything changes (the handles'
// own state apart: strips and phased steps are the entry point's business)
//
// Plain C++ (no HIP): the host runtime includes it through runtime/regrid.h, the CPU tests compile it on its own
// (tests/host/regrid_check.cpp).  vof2d/regrid.py (factors) mirrors it.
#pragma once
#include <stdint.h>

#include "../../../include/vof2d.h"

namespace vof {

struct RegridFactors { int rx, ry, dir; };   // dir: +1 refined, -1 coarsened, 0 the same grid

// NULL and *f filled if a state on src_nx x src_ny cells can be carried onto dst_nx x dst_ny, else what is wrong: both extents of
// one grid are integer multiples, at most VOF_REGRID_MAX_FACTOR, of the other's
inline const char* regrid_factors(int src_nx, int src_ny, int dst_nx, int dst_ny, RegridFactors* f) {
  if (src_nx < 1 || src_ny < 1 || dst_nx < 1 || dst_ny < 1) return "a grid has an extent < 1";
  const bool up = dst_nx >= src_nx && dst_ny >= src_ny, down = dst_nx <= src_nx && dst_ny <= src_ny;
  if (!up && !down) return "the grids are refined along one axis and coarsened along the other";
  const int big_x = up ? dst_nx : src_nx, small_x = up ? src_nx : dst_nx, big_y = up ? dst_ny : src_ny, small_y = up ? src_ny : dst_ny;
  if (big_x % small_x != 0 || big_y % small_y != 0) return "nx and ny of one grid must be integer multiples of the other's";
  const int rx = big_x / small_x, ry = big_y / small_y;
  if (rx > VOF_REGRID_MAX_FACTOR || ry > VOF_REGRID_MAX_FACTOR) return "a factor is larger than VOF_REGRID_MAX_FACTOR";
  f->rx = rx; f->ry = ry;
  f->dir = (rx == 1 && ry == 1) ? 0 : (up ? 1 : -1);
  return nullptr;
}

// NULL if vof_regrid may go on with these arguments (the handles' state apart), else the message of its VOF_EINVAL
inline const char* regrid_check(int src_nx, int src_ny, double src_Lx, double src_Ly, int dst_nx, int dst_ny, double dst_Lx, double dst_Ly, int32_t flags,
                                double eps, RegridFactors* f) {
  if (flags & ~VOF_REGRID_PLIC) return "flags has a bit outside VOF_REGRID_PLIC";
  if (!(src_Lx == dst_Lx) || !(src_Ly == dst_Ly)) return "the handles differ in Lx or Ly";
  if (const char* const msg = regrid_factors(src_nx, src_ny, dst_nx, dst_ny, f)) return msg;
  if ((flags & VOF_REGRID_PLIC) && !(eps >= 0.0 && eps < 0.5)) return "eps must lie in [0, 0.5)";
  return nullptr;
}

}  // namespace vof
