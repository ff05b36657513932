// kernels/curvature.h -- height-function interface curvature on the device (CurvVerb of kernels/cell_rows.h): Youngs' sums pick the axis, 7 x 3 heights, the solver's own CSF curvature beside it
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_curvature).  Whole-domain handles only.  The cells are
// i in [1, nx], j in [1, ny].  Every operand is converted to double first; then, per cell, in this order (a NumPy restatement follows
// it term for term, tests/_curvature_np.py).  f(ii, jj) = F[clamp(ii, 0, nx + 1), clamp(jj, 0, ny + 1)]: a stencil that reaches past
// the one stored ghost layer repeats that layer.  cx = -1 / (2 dx), cy = -1 / (2 dy), kx = 1 / dx / 2, ky = 1 / dy / 2 (the folded
// constants of 2dvof.py:287-288, :308), every sum left to right, `c ? x : y` a select on exactly that comparison (a NaN takes `y`).
// S(a, b) = (mxsum, mysum) of the cell (a, b) from its 3 x 3 neighbourhood, with g(di, dj) = f(a + di, b + dj):
//   mx1 = cx * (((g(1,1) + g(1,0)) - g(0,1)) - g(0,0))     my1 = cy * (((g(1,1) - g(1,0)) + g(0,1)) - g(0,0))       (:287-288)
//   mx2 = cx * (((g(1,0) + g(1,-1)) - g(0,0)) - g(0,-1))   my2 = cy * (((g(1,0) - g(1,-1)) + g(0,0)) - g(0,-1))     (:289-290)
//   mx3 = cx * (((g(0,0) + g(0,-1)) - g(-1,0)) - g(-1,-1)) my3 = cy * (((g(0,0) - g(0,-1)) + g(-1,0)) - g(-1,-1))   (:291-292)
//   mx4 = cx * (((g(0,1) + g(0,0)) - g(-1,1)) - g(-1,0))   my4 = cy * (((g(0,1) - g(0,0)) + g(-1,1)) - g(-1,0))     (:293-294)
//   mxsum = (((mx1 + mx2) + mx3) + mx4) / 4                mysum = (((my1 + my2) + my3) + my4) / 4                  (:296-297)
// The cell (i, j), with F = f(i, j) and (mxsum, mysum) = S(i, j) -- the expressions of iface_cell (kernels/interface.h):
//   mixed      = eps < F && F < 1 - eps                                              (a NaN F is not mixed: no row, not counted)
//   degenerate = |mxsum| < 1e-10 && |mysum| < 1e-10                                  (:300; counted, no row)
//   ax = |mxsum| * dx    by = |mysum| * dy    AXIS = ax > by ? 1 : 0                 (1: heights are summed along i; the tie: along j)
//   H[d], d = -1, 0, 1:  AXIS 0: (((((f(i+d,j-3) + f(i+d,j-2)) + f(i+d,j-1)) + f(i+d,j)) + f(i+d,j+1)) + f(i+d,j+2)) + f(i+d,j+3)
//                        AXIS 1: the same over f(i-3,j+d) .. f(i+3,j+d)              (the raw F, t = -3 .. 3 ascending)
//   m = AXIS ? mxsum : mysum    tl = m >= 0 ? -3 : 3                                 (the normal points liquid -> gas: tl is the liquid end)
//   VALID = for every d: (end cell t = tl) >= 1 - eps && (end cell t = -tl) <= eps   (the written comparisons: a NaN fails them)
//   (hs, ht) = AXIS ? (dx, dy) : (dy, dx)
//   hp  = ((H[1] - H[-1]) * hs) / (2 * ht)
//   hpp = (((H[1] - 2 * H[0]) + H[-1]) * hs) / (ht * ht)
//   q = 1 + hp * hp      KAPPA = hpp / (q * sqrt(q))      HP = hp;     not VALID: KAPPA = 0, HP = 0
//   H is the liquid's height measured from the liquid end of the column whichever end that is, so a convex liquid (a drop) has
//   hpp < 0 from every side: KAPPA is -1 / R for a drop and +1 / R for a bubble, the solver's sign, without a case split.
// KAPPA_CSF, the solver's own curvature at (i, j) (:287-309 with the bracketing of k_normals / k_kappa, kernels/verbs.h), in double:
//   N(a, b) = (0, 0) if (a, b) lies outside [1, nx] x [1, ny] (the reference never writes those); else with (sx, sy) = S(a, b):
//             |sx| < 1e-10 && |sy| < 1e-10 ? (sx, sy) : (sx / mag, sy / mag), mag = sqrt(sx * sx + sy * sy)            (:300-306)
//   KAPPA_CSF = -(kx * (N(i+1,j).x - N(i-1,j).x) + ky * (N(i,j+1).y - N(i,j-1).y))                                      (:308)
// On an f64 handle that is, bit for bit, kappa[i, j] directly after vof_get_normal_young on the same F.
// A row: I, J, KAPPA, VALID (1.0 or 0.0), AXIS (1.0 or 0.0), KAPPA_CSF, HP, F.
// No contraction: each term is the bits of the line above in either build -- every product whose result an addition or subtraction
// takes goes through mul_rounded (kernels/cells.h).
//
// The rows, in ascending (i, j), come out of the three launches of kernels/cell_rows.h (count, scan, emit), CurvVerb below being the verb.  The
// march hands curv_cell the rows i - 1, i, i + 1 of F from its registers; the lanes that hold a mixed cell gather the rest of their stencils
// (7 x 3 heights, the plus-shaped 5 x 5 of KAPPA_CSF) with clamped-index loads of rows the march has just streamed.
// The reduced values, CVP_NS sums then CVP_NM maxima: a lane adds, row by row, column by column, 1 per degenerate cell, 1 per VALID row,
// KAPPA and KAPPA * KAPPA of every VALID row, KAPPA_CSF and KAPPA_CSF * KAPPA_CSF of every row, and takes the maxima of -KAPPA, KAPPA
// (VALID rows), -KAPPA_CSF, KAPPA_CSF (all rows) with "a NaN counts as +inf" (diag_max); from there the reduction of
// kernels/reduce.h, folded by the scan (one block of 1024 threads).  A minimum is the negated maximum of the
// negatives.  With no operand a sum reads 0, a maximum what the fold starts from, -inf, and a minimum +inf.
#pragma once
#include "cells.h"
#include "cell_rows.h"

namespace vof {

// slots of a row and of the summary (= VOF_CURV_* of include/vof2d.h)
enum : int { CV_I = 0, CV_J, CV_KAPPA, CV_VALID, CV_AXIS, CV_KAPPA_CSF, CV_HP, CV_F, CV_N = 8 };
enum : int { CVS_ROWS = 0, CVS_DEGENERATE, CVS_VALID, CVS_SUM_K, CVS_SUM_K2, CVS_MIN_K, CVS_MAX_K, CVS_SUM_CSF, CVS_SUM_CSF2, CVS_MIN_CSF, CVS_MAX_CSF,
              CVS_ISTEP, CVS_N = 16 };
// the reduced values: CVP_NS sums, then CVP_NM maxima
enum : int { CVP_DEGENERATE = 0, CVP_VALID, CVP_SUM_K, CVP_SUM_K2, CVP_SUM_CSF, CVP_SUM_CSF2, CVP_NS = 6,
              CVP_NEG_MIN_K = 6, CVP_MAX_K, CVP_NEG_MIN_CSF, CVP_MAX_CSF, CVP_N = 10, CVP_NM = CVP_N - CVP_NS };

struct CurvConsts { double eps, one_m_eps, cx, cy, dx, dy, kx, ky; };

// S of the cell whose 3 x 3 neighbourhood is fm = row a - 1, f0 = row a, fp = row a + 1, each [b - 1, b, b + 1]
__device__ __forceinline__ void young_sums(const CurvConsts& c, const double (&fm)[3], const double (&f0)[3], const double (&fp)[3], double& mxsum,
                                           double& mysum) {
  const double mx1 = mul_rounded(c.cx, ((fp[2] + fp[1]) - f0[2]) - f0[1]), my1 = mul_rounded(c.cy, ((fp[2] - fp[1]) + f0[2]) - f0[1]);
  const double mx2 = mul_rounded(c.cx, ((fp[1] + fp[0]) - f0[1]) - f0[0]), my2 = mul_rounded(c.cy, ((fp[1] - fp[0]) + f0[1]) - f0[0]);
  const double mx3 = mul_rounded(c.cx, ((f0[1] + f0[0]) - fm[1]) - fm[0]), my3 = mul_rounded(c.cy, ((f0[1] - f0[0]) + fm[1]) - fm[0]);
  const double mx4 = mul_rounded(c.cx, ((f0[2] + f0[1]) - fm[2]) - fm[1]), my4 = mul_rounded(c.cy, ((f0[2] - f0[1]) + fm[2]) - fm[1]);
  mxsum = (((mx1 + mx2) + mx3) + mx4) * 0.25;   // (/ 4: the same bits)
  mysum = (((my1 + my2) + my3) + my4) * 0.25;
}

// f(ii, jj): the clamped-index load of a lane that holds a mixed cell (a row the march has just streamed: an L2 hit)
template <typename T>
__device__ __forceinline__ double curv_f(const Geom& g, const T* __restrict__ F, int ii, int jj) {
  ii = ii < 0 ? 0 : ii > g.nx + 1 ? g.nx + 1 : ii;
  jj = jj < 0 ? 0 : jj > g.ny + 1 ? g.ny + 1 : jj;
  return (double)F[at(g, ii, jj)];
}

// N(a, b).  Without a branch, so that the loads of the four calls of a cell are in flight together: a cell outside the interior
// loads the neighbourhood of the nearest interior cell (stored: no clamp of the single loads) and selects 0 at the end.
template <typename T>
__device__ __forceinline__ void young_unit(const CurvConsts& c, const Geom& g, const T* __restrict__ F, int a, int b, double& ux, double& uy) {
  const bool inside = a >= 1 && a <= g.nx && b >= 1 && b <= g.ny;
  a = a < 1 ? 1 : a > g.nx ? g.nx : a;
  b = b < 1 ? 1 : b > g.ny ? g.ny : b;
  const T* const p = F + at(g, a, b);
  const int64_t pitch = g.pitch;
  const double fm[3] = {(double)p[-pitch - 1], (double)p[-pitch], (double)p[-pitch + 1]};
  const double f0[3] = {(double)p[-1], (double)p[0], (double)p[1]};
  const double fp[3] = {(double)p[pitch - 1], (double)p[pitch], (double)p[pitch + 1]};
  double sx, sy;
  young_sums(c, fm, f0, fp, sx, sy);
  const bool tiny = __builtin_fabs(sx) < 1e-10 && __builtin_fabs(sy) < 1e-10;
  const double mag = __builtin_sqrt(mul_rounded(sx, sx) + mul_rounded(sy, sy));
  ux = inside ? (tiny ? sx : sx / mag) : 0.0;
  uy = inside ? (tiny ? sy : sy / mag) : 0.0;
}

// KAPPA_CSF of the cell (a, b) of the interior, everything gathered from F (four neighbourhoods of 3 x 3: 36 loads, issued together).
// Shared with kernels/energy.h, which needs it at both cells of a face the interface crosses.
template <typename T>
__device__ __forceinline__ double kappa_csf(const CurvConsts& c, const Geom& g, const T* __restrict__ F, int a, int b) {
  double xe, xw, yn, ys, other;
  young_unit<T>(c, g, F, a + 1, b, xe, other);
  young_unit<T>(c, g, F, a - 1, b, xw, other);
  young_unit<T>(c, g, F, a, b + 1, other, yn);
  young_unit<T>(c, g, F, a, b - 1, other, ys);
  return -(mul_rounded(c.kx, xe - xw) + mul_rounded(c.ky, yn - ys));
}

// the cell (i, j): fm, f0, fp as in young_sums (from the march's registers), everything else gathered from F.
// Returns 0: not mixed, 1: degenerate, 2: a row (s[CV_*] filled).
template <typename T>
__device__ __forceinline__ int curv_cell(const CurvConsts& c, const Geom& g, const T* __restrict__ F, const double (&fm)[3], const double (&f0)[3],
                                         const double (&fp)[3], int i, int j, double (&s)[CV_N]) {
  const double Fc = f0[1];
  if (!(c.eps < Fc && Fc < c.one_m_eps)) return 0;
  double mxsum, mysum;
  young_sums(c, fm, f0, fp, mxsum, mysum);
  if (__builtin_fabs(mxsum) < 1e-10 && __builtin_fabs(mysum) < 1e-10) return 1;
  const double ax = __builtin_fabs(mxsum) * c.dx, by = __builtin_fabs(mysum) * c.dy;
  const bool along_i = ax > by;
  const double m = along_i ? mxsum : mysum;
  const int tl = m >= 0.0 ? -3 : 3;
  const int si = along_i ? 1 : 0, sj = 1 - si;   // the step of t; d steps the other index
  double H[3];
  bool valid = true;
#pragma unroll
  for (int d = -1; d <= 1; ++d) {
    double f[7];   // (the seven loads of a column are issued together: a running sum over dependent loads pays the latency seven times)
#pragma unroll
    for (int t = -3; t <= 3; ++t) f[t + 3] = curv_f<T>(g, F, i + si * t + sj * d, j + sj * t + si * d);
    double h = f[0];
#pragma unroll
    for (int t = -2; t <= 3; ++t) h += f[t + 3];
    const double liquid = tl < 0 ? f[0] : f[6], gas = tl < 0 ? f[6] : f[0];
    valid = valid && liquid >= c.one_m_eps && gas <= c.eps;
    H[d + 1] = h;
  }
  const double hs = along_i ? c.dx : c.dy, ht = along_i ? c.dy : c.dx;
  const double hp = ((H[2] - H[0]) * hs) / (2.0 * ht);
  const double hpp = (((H[2] - mul_rounded(2.0, H[1])) + H[0]) * hs) / (ht * ht);
  const double q = 1.0 + mul_rounded(hp, hp);
  const double kappa = hpp / (q * __builtin_sqrt(q));
  s[CV_I] = (double)i; s[CV_J] = (double)j;
  s[CV_KAPPA] = valid ? kappa : 0.0; s[CV_VALID] = valid ? 1.0 : 0.0;
  s[CV_AXIS] = along_i ? 1.0 : 0.0; s[CV_KAPPA_CSF] = kappa_csf<T>(c, g, F, i, j);
  s[CV_HP] = valid ? hp : 0.0; s[CV_F] = Fc;
  return 2;
}

// ------------------------------------------------------------------ the verb of kernels/cell_rows.h
struct CurvVerb {
  enum : int { ROW_N = CV_N, SUM_N = CVS_N, NS = CVP_NS, NM = CVP_NM };
  using Consts = CurvConsts;
  template <typename T>
  static __device__ __forceinline__ int cell(const CurvConsts& c, const Geom& g, const T* __restrict__ F, const double (&fm)[3], const double (&f0)[3],
                                             const double (&fp)[3], int i, int j, double (&s)[CV_N]) {
    return curv_cell<T>(c, g, F, fm, f0, fp, i, j, s);
  }
  struct Tally {
    static constexpr double NONE = -__builtin_huge_val();
    double acc[CVP_N] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, NONE, NONE, NONE, NONE};
    int ndeg = 0, nvalid = 0;
    __device__ __forceinline__ void row(const double (&s)[CV_N]) {
      const double kc = s[CV_KAPPA_CSF];
      acc[CVP_SUM_CSF] += kc;
      acc[CVP_SUM_CSF2] += mul_rounded(kc, kc);
      acc[CVP_NEG_MIN_CSF] = diag_max(acc[CVP_NEG_MIN_CSF], -kc);
      acc[CVP_MAX_CSF] = diag_max(acc[CVP_MAX_CSF], kc);
      if (s[CV_VALID] != 0.0) {
        const double k = s[CV_KAPPA];
        ++nvalid;
        acc[CVP_SUM_K] += k;
        acc[CVP_SUM_K2] += mul_rounded(k, k);
        acc[CVP_NEG_MIN_K] = diag_max(acc[CVP_NEG_MIN_K], -k);
        acc[CVP_MAX_K] = diag_max(acc[CVP_MAX_K], k);
      }
    }
    __device__ __forceinline__ void degenerate() { ++ndeg; }
    __device__ __forceinline__ void publish(double* __restrict__ part) {
      acc[CVP_DEGENERATE] = (double)ndeg;
      acc[CVP_VALID] = (double)nvalid;
      block_publish<CVP_NS, CVP_NM>(acc, part);
    }
  };
  // (the slots between CVS_MAX_CSF and CVS_ISTEP, and behind it: 0)
  static __device__ __forceinline__ double summary(int t, double nrows, const double (&red)[CVP_N], double istep) {
    switch (t) {
      case CVS_ROWS: return nrows;
      case CVS_DEGENERATE: return red[CVP_DEGENERATE];
      case CVS_VALID: return red[CVP_VALID];
      case CVS_SUM_K: return red[CVP_SUM_K];
      case CVS_SUM_K2: return red[CVP_SUM_K2];
      case CVS_MIN_K: return -red[CVP_NEG_MIN_K];
      case CVS_MAX_K: return red[CVP_MAX_K];
      case CVS_SUM_CSF: return red[CVP_SUM_CSF];
      case CVS_SUM_CSF2: return red[CVP_SUM_CSF2];
      case CVS_MIN_CSF: return -red[CVP_NEG_MIN_CSF];
      case CVS_MAX_CSF: return red[CVP_MAX_CSF];
      case CVS_ISTEP: return istep;
      default: return 0.0;
    }
  }
};

}  // namespace vof
