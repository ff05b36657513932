// kernels/interface.h -- PLIC interface segments extracted on the device (IfaceVerb of kernels/cell_rows.h): Youngs' normal, the line in the cell
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_interface).  The cells are i in [g.ilo, g.ihi]
// (the caller passes the handle's owned interior rows there), j in [1, ny].  Every operand is converted to double first;
// then, per cell, in this order (a NumPy restatement follows it term for term, tests/_interface_np.py).  With
// f(di, dj) = F[i + di, j + dj], cx = -1 / (2 dx), cy = -1 / (2 dy) (the folded constants of 2dvof.py:287-288), every sum
// left to right, `c ? x : y` a select on exactly that comparison (a NaN takes the `y` branch):
//   mixed  = eps < f(0,0) && f(0,0) < 1 - eps                                       (a NaN F is not mixed: no row, not counted)
//   mx1 = cx * (((f(1,1) + f(1,0)) - f(0,1)) - f(0,0))     my1 = cy * (((f(1,1) - f(1,0)) + f(0,1)) - f(0,0))       (:287-288)
//   mx2 = cx * (((f(1,0) + f(1,-1)) - f(0,0)) - f(0,-1))   my2 = cy * (((f(1,0) - f(1,-1)) + f(0,0)) - f(0,-1))     (:289-290)
//   mx3 = cx * (((f(0,0) + f(0,-1)) - f(-1,0)) - f(-1,-1)) my3 = cy * (((f(0,0) - f(0,-1)) + f(-1,0)) - f(-1,-1))   (:291-292)
//   mx4 = cx * (((f(0,1) + f(0,0)) - f(-1,1)) - f(-1,0))   my4 = cy * (((f(0,1) - f(0,0)) + f(-1,1)) - f(-1,0))     (:293-294)
//   mxsum = (((mx1 + mx2) + mx3) + mx4) / 4                mysum = (((my1 + my2) + my3) + my4) / 4                  (:296-297)
//   degenerate = |mxsum| < 1e-10 && |mysum| < 1e-10        (:300; counted, no row)
//   ax = |mxsum| * dx    by = |mysum| * dy    s = ax + by    a = ax / s    b = by / s
//   n1 = a < b ? a : b   n2 = a < b ? b : a   Fm = F <= 0.5 ? F : 1 - F
//   alpha = (2 * n2) * Fm < n1 ? sqrt(((2 * n1) * n2) * Fm) : n2 * Fm + n1 * 0.5;      F > 0.5: alpha = 1 - alpha
//   P = (b > 0 && alpha <= b) ? (0, alpha / b) : ((alpha - b) / a, 1)               (the end on xi = 0, else on eta = 1)
//   Q = (a > 0 && alpha <= a) ? (alpha / a, 0) : (1, (alpha - a) / b)               (the end on eta = 0, else on xi = 1)
//   mxsum < 0: xi -> 1 - xi for both;   mysum < 0: eta -> 1 - eta for both
//   x = ((i - 1) + xi) * dx    y = ((j - 1) + eta) * dy
//   In the frame of a, b >= 0 the liquid (a xi + b eta < alpha) holds the corner (0, 0): it is on the left going from Q to
//   P.  Each mirror turns that round, so (X0, Y0) -> (X1, Y1) is Q -> P unless exactly one of mxsum, mysum is < 0: P -> Q.
//   mag = sqrt(mxsum * mxsum + mysum * mysum)    NX = mxsum / mag    NY = mysum / mag
//   ddx = X1 - X0    ddy = Y1 - Y0    len = sqrt(ddx * ddx + ddy * ddy)
// No contraction (-ffp-contract=off): each term is the bits of the line above.
//
// The rows, in ascending (i, j), come out of the three launches of kernels/cell_rows.h (count, scan, emit), IfaceVerb below being the verb.
// Order of the LENGTH sum, fixed: a lane adds the lengths of its cells row by row, column by column; from there the
// reduction of kernels/reduce.h, two sums wide: one partial of kIfacePart doubles per block, folded by the scan (one
// block of 1024 threads).  The degenerate count travels the same way as a double (exact).
#pragma once
#include "cells.h"
#include "cell_rows.h"

namespace vof {

// slots of a row and of the summary (= VOF_IFACE_* of include/vof2d.h)
enum : int { IF_I = 0, IF_J, IF_X0, IF_Y0, IF_X1, IF_Y1, IF_NX, IF_NY, IF_N = 8 };
enum : int { IFS_SEGMENTS = 0, IFS_DEGENERATE, IFS_LENGTH, IFS_ISTEP, IFS_N = 4 };
constexpr int kIfacePart = 2;   // doubles per block in the partials buffer: the length, the degenerate cells

struct IfaceConsts { double eps, one_m_eps, cx, cy, dx, dy; };

// The line of a mixed cell in the frame of a, b >= 0: the liquid is a xi + b eta < alpha; flip_x, flip_y: the mirrors that take the
// frame back to the cell's (mxsum < 0, mysum < 0).  What iface_cell cuts into a segment and k_regrid_refine (kernels/regrid.h) into
// the F of a cell's children.
struct IfaceLine { double mxsum, mysum, a, b, alpha; bool flip_x, flip_y; };

// the line of the cell from its 3 x 3 neighbourhood fm = row i - 1, f0 = row i, fp = row i + 1, each [j - 1, j, j + 1].
// Returns 0: not mixed, 1: degenerate, 2: a line (l filled).
__device__ __forceinline__ int iface_line(const IfaceConsts& c, const double (&fm)[3], const double (&f0)[3], const double (&fp)[3], IfaceLine& l) {
  const double F = f0[1];
  if (!(c.eps < F && F < c.one_m_eps)) return 0;
  const double mx1 = c.cx * (((fp[2] + fp[1]) - f0[2]) - f0[1]), my1 = c.cy * (((fp[2] - fp[1]) + f0[2]) - f0[1]);
  const double mx2 = c.cx * (((fp[1] + fp[0]) - f0[1]) - f0[0]), my2 = c.cy * (((fp[1] - fp[0]) + f0[1]) - f0[0]);
  const double mx3 = c.cx * (((f0[1] + f0[0]) - fm[1]) - fm[0]), my3 = c.cy * (((f0[1] - f0[0]) + fm[1]) - fm[0]);
  const double mx4 = c.cx * (((f0[2] + f0[1]) - fm[2]) - fm[1]), my4 = c.cy * (((f0[2] - f0[1]) + fm[2]) - fm[1]);
  const double mxsum = (((mx1 + mx2) + mx3) + mx4) * 0.25, mysum = (((my1 + my2) + my3) + my4) * 0.25;   // (/ 4: the same bits)
  if (__builtin_fabs(mxsum) < 1e-10 && __builtin_fabs(mysum) < 1e-10) return 1;
  const double ax = __builtin_fabs(mxsum) * c.dx, by = __builtin_fabs(mysum) * c.dy;
  const double sum = ax + by;
  const double a = ax / sum, b = by / sum;
  const double n1 = a < b ? a : b, n2 = a < b ? b : a;
  const double Fm = F <= 0.5 ? F : 1.0 - F;
  double alpha = (2.0 * n2) * Fm < n1 ? __builtin_sqrt(((2.0 * n1) * n2) * Fm) : n2 * Fm + n1 * 0.5;
  if (F > 0.5) alpha = 1.0 - alpha;
  l.mxsum = mxsum; l.mysum = mysum; l.a = a; l.b = b; l.alpha = alpha;
  l.flip_x = mxsum < 0.0; l.flip_y = mysum < 0.0;
  return 2;
}

// the cell (i, j) from the same neighbourhood.  Returns 0: not mixed, 1: degenerate, 2: a segment (s[IF_*] filled).
__device__ __forceinline__ int iface_cell(const IfaceConsts& c, const double (&fm)[3], const double (&f0)[3], const double (&fp)[3], int i, int j,
                                          double (&s)[IF_N]) {
  IfaceLine l;
  const int kind = iface_line(c, fm, f0, fp, l);
  if (kind != 2) return kind;
  const double mxsum = l.mxsum, mysum = l.mysum, a = l.a, b = l.b, alpha = l.alpha;
  const bool p_left = b > 0.0 && alpha <= b, q_bottom = a > 0.0 && alpha <= a;
  double pxi = p_left ? 0.0 : (alpha - b) / a, peta = p_left ? alpha / b : 1.0;
  double qxi = q_bottom ? alpha / a : 1.0, qeta = q_bottom ? 0.0 : (alpha - a) / b;
  const bool flip_x = l.flip_x, flip_y = l.flip_y;
  if (flip_x) { pxi = 1.0 - pxi; qxi = 1.0 - qxi; }
  if (flip_y) { peta = 1.0 - peta; qeta = 1.0 - qeta; }
  const double di = (double)(i - 1), dj = (double)(j - 1);
  const double px = (di + pxi) * c.dx, py = (dj + peta) * c.dy, qx = (di + qxi) * c.dx, qy = (dj + qeta) * c.dy;
  const bool p_first = flip_x != flip_y;
  const double mag = __builtin_sqrt(mxsum * mxsum + mysum * mysum);
  s[IF_I] = (double)i; s[IF_J] = (double)j;
  s[IF_X0] = p_first ? px : qx; s[IF_Y0] = p_first ? py : qy;
  s[IF_X1] = p_first ? qx : px; s[IF_Y1] = p_first ? qy : py;
  s[IF_NX] = mxsum / mag; s[IF_NY] = mysum / mag;
  return 2;
}

// ------------------------------------------------------------------ the verb of kernels/cell_rows.h
// The reduced values: slot 0 the length, slot 1 the degenerate cells (as a double: exact).
struct IfaceVerb {
  enum : int { ROW_N = IF_N, SUM_N = IFS_N, NS = kIfacePart, NM = 0 };
  using Consts = IfaceConsts;
  template <typename T>
  static __device__ __forceinline__ int cell(const IfaceConsts& c, const Geom&, const T*, const double (&fm)[3], const double (&f0)[3],
                                             const double (&fp)[3], int i, int j, double (&s)[IF_N]) {
    return iface_cell(c, fm, f0, fp, i, j, s);
  }
  struct Tally {
    double acc[kIfacePart] = {0.0, 0.0};
    int ndeg = 0;
    __device__ __forceinline__ void row(const double (&s)[IF_N]) {
      const double ddx = s[IF_X1] - s[IF_X0], ddy = s[IF_Y1] - s[IF_Y0];
      acc[0] += __builtin_sqrt(ddx * ddx + ddy * ddy);
    }
    __device__ __forceinline__ void degenerate() { ++ndeg; }
    __device__ __forceinline__ void publish(double* __restrict__ part) {
      acc[1] = (double)ndeg;
      block_publish<kIfacePart, 0>(acc, part);
    }
  };
  static __device__ __forceinline__ double summary(int t, double segments, const double (&red)[kIfacePart], double istep) {
    return t == IFS_SEGMENTS ? segments : t == IFS_DEGENERATE ? red[1] : t == IFS_LENGTH ? red[0] : istep;
  }
};

}  // namespace vof
