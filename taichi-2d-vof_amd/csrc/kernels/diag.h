// kernels/diag.h -- flow diagnostics reduced on the device (k_diag, kDiagRow): volume, centroid, kinetic energy, divergence, extrema
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_diagnostics).  One pass over F, u, v on the
// cells i in [g.ilo, g.ihi] (the caller passes the handle's owned interior rows there), j in [1, ny].  Every operand is
// converted to double first; then, per cell, in this order (a NumPy restatement follows it term for term,
// tests/_diag_np.py):
//   f  = F[i,j]                      uw = u[i,j]    ue = u[i+1,j]    vs = v[i,j]    vn = v[i,j+1]
//   SUM_F    += f
//   SUM_FI   += f * i                (global integer index as a double)
//   SUM_FJ   += f * j
//   uc = (uw + ue) * 0.5             vc = (vs + vn) * 0.5                            (interp_velocity, 2dvof.py:492)
//   Fc = fmin(fmax(f, 0), 1)         rho = rho_g * (1 - Fc) + rho_l * Fc             (the order of 2dvof.py:202, a plain clamp)
//   SUM_KE   += (rho * 0.5) * (uc * uc + vc * vc)
//   div = (ue - uw) * dxi + (vn - vs) * dyi
//   SUM_DIV2 += div * div            MAX_DIV = max(MAX_DIV, |div|)
//   MAX_U = max(MAX_U, |uw|, |ue|)   MAX_V = max(MAX_V, |vs|, |vn|)
//   MAX_F = max(MAX_F, f)            MIN_F = -max(-f)
// A NaN operand of a maximum counts as +inf (cg_amax, diag_max of kernels/reduce.h; a NaN F therefore reads MAX_F = +inf, MIN_F = -inf);
// the sums propagate it.  No contraction (-ffp-contract=off): each term is the bits of the line above.
//
// Order of the sums, fixed: a lane adds its cells row by row, column by column; from there the reduction of kernels/reduce.h, five sums and
// five maxima wide: one partial of kDiagPart doubles per block, folded by k_row_finish (kernels/cells.h, one block of 256 threads) into the row
// kDiagRow describes.  No atomics, no LDS beyond the reduction.  The march is reduced_rows of kernels/cells.h: 3 array passes.
#pragma once
#include "cells.h"

namespace vof {

// slots of a row of diagnostics (= VOF_DIAG_* of include/vof2d.h)
enum : int { DG_ISTEP = 0, DG_SUM_F, DG_SUM_FI, DG_SUM_FJ, DG_SUM_KE, DG_SUM_DIV2, DG_MAX_DIV, DG_MAX_U, DG_MAX_V, DG_MIN_F, DG_MAX_F, DG_CELLS, DG_N = 16 };
constexpr int kDiagSums = 5, kDiagPart = 10;   // doubles per block in the partials buffer: five sums, then five maxima (|div|, |u|, |v|, -F, F)
constexpr RowMap<kDiagSums, kDiagPart - kDiagSums> kDiagRow = {DG_N, {{ROW_ISTEP, 0}, {ROW_VALUE, 0}, {ROW_VALUE, 1}, {ROW_VALUE, 2}, {ROW_VALUE, 3}, {ROW_VALUE, 4},
    {ROW_VALUE, 5}, {ROW_VALUE, 6}, {ROW_VALUE, 7}, {ROW_MINUS, 8}, {ROW_VALUE, 9}, {ROW_CELLS, 0}},
    {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -__builtin_huge_val(), -__builtin_huge_val()}};
static_assert(DG_SUM_F == 1 && DG_MAX_V == 8 && DG_MIN_F == 9 && DG_MAX_F == 10 && DG_CELLS == 11, "kDiagRow lists the slots in this order");

// ------------------------------------------------------------------ the pass over F, u, v
template <typename T, int V>
__global__ __launch_bounds__(256) void k_diag(Geom g, const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v, int R,
                                               double dxi, double dyi, double rho_g, double rho_l, double* __restrict__ part) {
  const double ninf = -__builtin_huge_val();
  double acc[kDiagPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, ninf, ninf};
  reduced_rows<kDiagSums, kDiagPart - kDiagSums, false, T, V>(g, nullptr, F, u, v, R, acc, part, [&](const Cell& c, double) {
    acc[0] += c.f;
    acc[1] += c.f * c.i;
    acc[2] += c.f * c.j;
    const double uc = face_mean(c.w, c.e), vc = face_mean(c.s, c.n);
    const double Fc = clamp01(c.f);
    const double rho = rho_g * (1.0 - Fc) + rho_l * Fc;
    acc[3] += (rho * 0.5) * (uc * uc + vc * vc);
    const double div = (c.e - c.w) * dxi + (c.n - c.s) * dyi;
    acc[4] += div * div;
    acc[5] = cg_amax(acc[5], div);
    acc[6] = cg_amax(cg_amax(acc[6], c.w), c.e);
    acc[7] = cg_amax(cg_amax(acc[7], c.s), c.n);
    acc[8] = diag_max(acc[8], -c.f);
    acc[9] = diag_max(acc[9], c.f);
  });
}

}  // namespace vof
