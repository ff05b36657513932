// kernels/diag.h -- flow diagnostics reduced on the device (k_diag, k_diag_finish): volume, centroid, kinetic energy, divergence, extrema
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
// Order of the sums, fixed: a lane adds its cells row by row, column by column; from there the reduction of
// kernels/reduce.h, five sums and five maxima wide: one partial of kDiagPart doubles per block, folded by k_diag_finish
// (one block of 256 threads).  No atomics, no LDS beyond the reduction.
// Traffic: F and v rows are loaded once, the u row i + 1 of one iteration is the row i of the next: 3 array passes.
#pragma once
#include "cg.h"

namespace vof {

// slots of a row of diagnostics (= VOF_DIAG_* of include/vof2d.h)
enum : int { DG_ISTEP = 0, DG_SUM_F, DG_SUM_FI, DG_SUM_FJ, DG_SUM_KE, DG_SUM_DIV2, DG_MAX_DIV, DG_MAX_U, DG_MAX_V, DG_MIN_F, DG_MAX_F, DG_CELLS, DG_N = 16 };
constexpr int kDiagSums = 5, kDiagPart = 10;   // doubles per block in the partials buffer: five sums, then five maxima (|div|, |u|, |v|, -F, F)

// ------------------------------------------------------------------ the pass over F, u, v
template <typename T, int V>
__global__ __launch_bounds__(256) void k_diag(Geom g, const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v, int R,
                                               double dxi, double dyi, double rho_g, double rho_l, double* __restrict__ part) {
  int j0, ra, rb;
  const bool active = cg_tile<V>(g, R, j0, ra, rb);
  const double ninf = -__builtin_huge_val();
  double acc[kDiagPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, ninf, ninf};
  if (active) {
    const int ny = g.ny;
    const int64_t pitch = g.pitch;
    size_t o = at(g, ra, j0);
    T uw[V];
    load_c<T, V>(uw, u + o);
    for (int i = ra; i <= rb; ++i) {
      T f[V], ue[V];
      Row<T, V> vr;
      load_s<T, V>(f, F + o);
      load_c<T, V>(ue, u + o + pitch);
      load_row<T, V>(vr, v + o);
      const double di = (double)i;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        if (j0 + q <= ny) {
          const double fd = (double)f[q], w = (double)uw[q], e = (double)ue[q], s = (double)vr.c[q], n = (double)right_of(vr, q);
          acc[0] += fd;
          acc[1] += fd * di;
          acc[2] += fd * (double)(j0 + q);
          const double uc = (w + e) * 0.5, vc = (s + n) * 0.5;
          const double Fc = __builtin_fmin(__builtin_fmax(fd, 0.0), 1.0);
          const double rho = rho_g * (1.0 - Fc) + rho_l * Fc;
          acc[3] += (rho * 0.5) * (uc * uc + vc * vc);
          const double div = (e - w) * dxi + (n - s) * dyi;
          acc[4] += div * div;
          acc[5] = cg_amax(acc[5], div);
          acc[6] = cg_amax(cg_amax(acc[6], w), e);
          acc[7] = cg_amax(cg_amax(acc[7], s), n);
          acc[8] = diag_max(acc[8], -fd);
          acc[9] = diag_max(acc[9], fd);
        }
      }
#pragma unroll
      for (int q = 0; q < V; ++q) uw[q] = ue[q];
      o += pitch;
    }
  }
  block_publish<kDiagSums, kDiagPart - kDiagSums>(acc, part);
}

// ------------------------------------------------------------------ the block partials -> one row of diagnostics
// ONE block of 256 threads, the shape of k_cg_finish: fold_partials of kernels/reduce.h, then threads 0 .. DG_N - 1 store
// one slot each of the row (unused slots read 0).  The launch boundary in front of it is what makes the partials of
// every other block visible.
__global__ __launch_bounds__(256) void k_diag_finish(const double* __restrict__ part, int nblocks, double* __restrict__ row, double istep, double cells) {
  __shared__ double red[256][kDiagPart];
  const int t = threadIdx.x;
  const double ninf = -__builtin_huge_val();
  const double init[kDiagPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, ninf, ninf};
  fold_partials<256, kDiagSums, kDiagPart - kDiagSums>(part, nblocks, init, red);
  if (t >= DG_N) return;
  double x = 0.0;
  if (t == DG_ISTEP) x = istep;
  else if (t >= DG_SUM_F && t <= DG_MAX_V) x = red[0][t - DG_SUM_F];
  else if (t == DG_MIN_F) x = -red[0][8];
  else if (t == DG_MAX_F) x = red[0][9];
  else if (t == DG_CELLS) x = cells;
  row[t] = x;
}

}  // namespace vof
