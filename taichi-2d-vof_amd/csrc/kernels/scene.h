// kernels/scene.h -- an initial state painted from shapes: an ordered list of boxes, ellipses, half-planes and triangles rasterised into F with S x S samples a cell (k_scene)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_set_scene).  All geometry is in doubles whatever the
// field type; every product below goes through mul_rounded (kernels/cells.h), whose result no contraction reaches, so the FMA build
// gives the same bytes.  A NumPy restatement follows it term for term (tests/_scene_np.py).
//
//   the cell    (i, j) covers [(i-1) dx, i dx] x [(j-1) dy, j dy] (find_area, 2dvof.py:105-106); a ghost cell is a cell like any
//               other, outside the domain.  dx, dy: the doubles of the host (vof_get_param)
//   the samples S in {1, 2, 4, 8, 16} per axis; sample (a, b), a, b in [0, S):
//                 xs = ((double)(i-1) + ((double)a + 0.5) * (1.0/S)) * dx      ys = ((double)(j-1) + ((double)b + 0.5) * (1.0/S)) * dy
//               the bracket is exact (S is a power of two): one rounding, the product's
//   the shapes  a record is SHR_N = 8 doubles: KIND, PHASE, A0 .. A5
//     BOX        cx, cy, hx, hy, c, s    px = xs - cx;  py = ys - cy;  lx = px*c + py*s;  ly = py*c - px*s
//                                        inside if |lx| <= hx and |ly| <= hy
//     ELLIPSE    the same fields, lx, ly the same;  t1 = lx*hy;  t2 = ly*hx;  t3 = hx*hy
//                                        inside if t1*t1 + t2*t2 <= t3*t3
//     HALFPLANE  px0, py0, nx, ny        inside if (xs - px0)*nx + (ys - py0)*ny <= 0
//     TRIANGLE   x0, y0, x1, y1, x2, y2  e0 = (x1-x0)*(ys-y0) - (y1-y0)*(xs-x0)
//                                        e1 = (x2-x1)*(ys-y1) - (y2-y1)*(xs-x1)
//                                        e2 = (x0-x2)*(ys-y2) - (y0-y2)*(xs-x2)
//                                        inside if e0 >= 0, e1 >= 0 and e2 >= 0, or e0 <= 0, e1 <= 0 and e2 <= 0
//               every difference, product and sum is rounded on its own, in the order written; a comparison with a NaN is false
//   painting    every sample starts as KEEP; the shapes are applied in list order, a sample inside a shape takes its phase
//   the cell's new value   n_liq, n_gas, n_keep: its samples in each state (with the CLEAR flag KEEP counts as GAS: n_keep = 0)
//               n_keep == S*S: the cell is not written
//               otherwise  F_new = (T)(((double)n_liq + (double)n_keep * (double)F_old) * (1.0/(S*S))); where n_keep == 0 the
//               term of F_old is left out and F_old is not read.  Written to F and to its sweep twin
//   the counts  PAINTED: cells with n_keep < S*S;  MIXED: cells with none of n_liq, n_gas, n_keep equal to S*S -- both over
//               the interior cells (j in [1, ny]) of the rows the handle reports (rep_lo .. rep_hi)
//
// One lane per stored cell (the grid of k_init_F).  The states of a group of up to 64 samples -- whole sample rows b: all of a
// cell up to S = 8, four groups of four rows at S = 16 -- are two bit masks in registers, LIQUID and GAS; the shape loop runs once
// per group, the record is read with a wave-uniform index (scalar loads), a shape's inside mask is built row by row and merged
// with two logic operations, the groups are counted with popcount.  No LDS, no scratch, no atomics but the two counters, ordinary
// vector stores.  The counters: one integer atomic per wave and counter with something to count, spread over SCW_SLOTS slots of
// 64 bytes by the wave's number (the host adds the slots up) -- at 4096^2 a quarter of a million waves adding to ONE address took
// 3.2 ms of a 3.4 ms call, whatever the shapes (profiles/scene.md).
//
// The shortcuts (S >= 4, knob scene_shortcuts).  For a group and a shape, the tests below are evaluated at the four corner
// samples of the group, (a, b) in {0, S-1} x {b0, b0 + rows - 1}; where they decide, the group's mask is all ones or zero without
// sampling.  What they rest on: a correctly rounded sum, difference or product is monotone in each operand (non-decreasing or
// non-increasing, by the sign of the other factor), and so is every composition of them in which an operand enters once.
//   - xs is monotone in a and ys in b, so every sample's xs lies between xs(0) and xs(S-1), its ys between the group's first and last;
//   - px, py and the products px*c, py*s, ... are monotone in xs or ys alone, and lx, ly, the half-plane's sum and a triangle's
//     e_k are a rounded sum or difference of one term in xs and one in ys: each is monotone in xs and in ys separately, so over the
//     samples of the group it stays between the smallest and the largest of its four corner values;
//   - a NaN inside the group (inf - inf, 0 * inf) implies one at a corner: an infinite term in xs is infinite at one end of xs,
//     one in ys at one end of ys, and the corner that has both ends has the NaN.  Every test below is a comparison, false on a NaN:
//     a corner NaN decides nothing and the group is sampled.
//   BOX        all in if |lx| <= hx and |ly| <= hy at the four corners; all out if lx > hx at all four, or lx < -hx, ly > hy, ly < -hy
//              at all four (a sample outside in one coordinate is outside).  For an axis-aligned box (c = 1, s = 0: lx = px, ly = py)
//              that is the comparison of the first and the last sample coordinate with the box's edges
//   HALFPLANE  all in if the sum is <= 0 at the four corners, all out if it is > 0 at the four
//   TRIANGLE   all in if every e_k >= 0 at the four corners, or every e_k <= 0; all out if one e_k is < 0 at the four corners (no
//              sample has all three >= 0) and one is > 0 at the four (none has all three <= 0)
//   ELLIPSE    the left side is not monotone in xs, but it is in |lx| and |ly|: t1*t1 is a rounded square of a rounded product with
//              hy >= 0.  With no NaN among the corner values, |lx| <= L1 = the largest corner |lx| and |lx| >= L0 = the smallest corner
//              |lx|, or 0 if the corner values straddle 0; M1, M0 likewise from ly.  Q(L, M), the left side evaluated with the same
//              roundings at |lx| = L, |ly| = M, bounds it: all in if Q(L1, M1) <= t3*t3, all out if Q(L0, M0) > t3*t3
// Lanes that decide wait for the lanes of their wave that sample; whole waves inside or outside a shape -- most of them -- skip it.
#pragma once
#include "cells.h"

namespace vof {

// = VOF_SHAPE_*, VOF_SCENE_* of include/vof2d.h: the kinds, the phases, the fields of a record, the flag, the counter words
enum : int { SHK_BOX = 0, SHK_ELLIPSE, SHK_HALFPLANE, SHK_TRIANGLE, SHK_N };
enum : int { SHP_GAS = 0, SHP_LIQUID = 1 };
enum : int { SHR_KIND = 0, SHR_PHASE, SHR_A0, SHR_N = 8 };
enum : int { SCF_CLEAR = 1 };
enum : int { SCW_PAINTED = 0, SCW_MIXED, SCW_STRIDE = 8, SCW_SLOTS = 256 };   // 64-bit words: a slot is SCW_STRIDE of them

// the groups of S x S samples: RPG whole sample rows of S bits each in one 64-bit mask, NG groups a cell
template <int S>
struct SceneGroups {
  static_assert(S == 1 || S == 2 || S == 4 || S == 8 || S == 16, "samples per axis");
  static constexpr int RPG = S * S >= 64 ? 64 / S : S, NG = S / RPG, BITS = RPG * S;
  static constexpr unsigned long long ALL = BITS == 64 ? ~0ull : (1ull << BITS) - 1ull;
};

// the coordinate of sample `sub` of cell `cell` along an axis of spacing d
template <int S>
__device__ __forceinline__ double scene_coord(int cell, int sub, double d) {
  return mul_rounded((double)(cell - 1) + ((double)sub + 0.5) * (1.0 / S), d);
}

// ------------------------------------------------------------------ the shapes: in(), and decide() over the corners (x0 | x1, y0 | y1)
// decide: 1 every sample between the corners is inside, -1 every one is outside, 0 not known (the argument: the head of this file)
struct ScBox {
  double cx, cy, hx, hy, c, s;
  __device__ __forceinline__ void local(double xs, double ys, double& lx, double& ly) const {
    const double px = xs - cx, py = ys - cy;
    lx = mul_rounded(px, c) + mul_rounded(py, s);
    ly = mul_rounded(py, c) - mul_rounded(px, s);
  }
  __device__ __forceinline__ bool in(double xs, double ys) const {
    double lx, ly;
    local(xs, ys, lx, ly);
    return __builtin_fabs(lx) <= hx && __builtin_fabs(ly) <= hy;
  }
  __device__ __forceinline__ void corners(double x0, double x1, double y0, double y1, double (&lx)[4], double (&ly)[4]) const {
    local(x0, y0, lx[0], ly[0]);
    local(x1, y0, lx[1], ly[1]);
    local(x0, y1, lx[2], ly[2]);
    local(x1, y1, lx[3], ly[3]);
  }
  __device__ __forceinline__ int decide(double x0, double x1, double y0, double y1) const {
    double lx[4], ly[4];
    corners(x0, x1, y0, y1, lx, ly);
    bool all_in = true, xhi = true, xlo = true, yhi = true, ylo = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      all_in = all_in && __builtin_fabs(lx[q]) <= hx && __builtin_fabs(ly[q]) <= hy;
      xhi = xhi && lx[q] > hx;
      xlo = xlo && lx[q] < -hx;
      yhi = yhi && ly[q] > hy;
      ylo = ylo && ly[q] < -hy;
    }
    return all_in ? 1 : ((xhi || xlo || yhi || ylo) ? -1 : 0);
  }
};

struct ScEllipse {
  ScBox f;      // the frame: cx, cy, hx, hy, c, s
  double rhs;   // t3*t3
  __device__ __forceinline__ explicit ScEllipse(const ScBox& b) : f(b) {
    const double t3 = mul_rounded(b.hx, b.hy);
    rhs = mul_rounded(t3, t3);
  }
  __device__ __forceinline__ double lhs(double lx, double ly) const {
    const double t1 = mul_rounded(lx, f.hy), t2 = mul_rounded(ly, f.hx);
    return mul_rounded(t1, t1) + mul_rounded(t2, t2);
  }
  __device__ __forceinline__ bool in(double xs, double ys) const {
    double lx, ly;
    f.local(xs, ys, lx, ly);
    return lhs(lx, ly) <= rhs;
  }
  __device__ __forceinline__ int decide(double x0, double x1, double y0, double y1) const {
    double lx[4], ly[4];
    f.corners(x0, x1, y0, y1, lx, ly);
    bool ok = true;
    double xmin = lx[0], xmax = lx[0], ymin = ly[0], ymax = ly[0];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      ok = ok && lx[q] == lx[q] && ly[q] == ly[q];
      xmin = lx[q] < xmin ? lx[q] : xmin;
      xmax = lx[q] > xmax ? lx[q] : xmax;
      ymin = ly[q] < ymin ? ly[q] : ymin;
      ymax = ly[q] > ymax ? ly[q] : ymax;
    }
    if (!ok) return 0;
    const double ax0 = __builtin_fabs(xmin), ax1 = __builtin_fabs(xmax), ay0 = __builtin_fabs(ymin), ay1 = __builtin_fabs(ymax);
    const double L1 = ax0 > ax1 ? ax0 : ax1, M1 = ay0 > ay1 ? ay0 : ay1;
    const double L0 = (xmin <= 0.0 && xmax >= 0.0) ? 0.0 : (ax0 < ax1 ? ax0 : ax1);
    const double M0 = (ymin <= 0.0 && ymax >= 0.0) ? 0.0 : (ay0 < ay1 ? ay0 : ay1);
    if (lhs(L1, M1) <= rhs) return 1;
    return lhs(L0, M0) > rhs ? -1 : 0;
  }
};

struct ScHalfplane {
  double px0, py0, nx, ny;
  __device__ __forceinline__ double side(double xs, double ys) const { return mul_rounded(xs - px0, nx) + mul_rounded(ys - py0, ny); }
  __device__ __forceinline__ bool in(double xs, double ys) const { return side(xs, ys) <= 0.0; }
  __device__ __forceinline__ int decide(double x0, double x1, double y0, double y1) const {
    const double v[4] = {side(x0, y0), side(x1, y0), side(x0, y1), side(x1, y1)};
    bool all_in = true, all_out = true;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      all_in = all_in && v[q] <= 0.0;
      all_out = all_out && v[q] > 0.0;
    }
    return all_in ? 1 : (all_out ? -1 : 0);
  }
};

struct ScTriangle {
  double x0, y0, x1, y1, x2, y2;
  __device__ __forceinline__ void edges(double xs, double ys, double (&e)[3]) const {
    e[0] = mul_rounded(x1 - x0, ys - y0) - mul_rounded(y1 - y0, xs - x0);
    e[1] = mul_rounded(x2 - x1, ys - y1) - mul_rounded(y2 - y1, xs - x1);
    e[2] = mul_rounded(x0 - x2, ys - y2) - mul_rounded(y0 - y2, xs - x2);
  }
  __device__ __forceinline__ bool in(double xs, double ys) const {
    double e[3];
    edges(xs, ys, e);
    return (e[0] >= 0.0 && e[1] >= 0.0 && e[2] >= 0.0) || (e[0] <= 0.0 && e[1] <= 0.0 && e[2] <= 0.0);
  }
  __device__ __forceinline__ int decide(double xa, double xb, double ya, double yb) const {
    double e[4][3];
    edges(xa, ya, e[0]);
    edges(xb, ya, e[1]);
    edges(xa, yb, e[2]);
    edges(xb, yb, e[3]);
    bool all_ge = true, all_le = true, some_lt = false, some_gt = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      bool lt = true, gt = true;   // edge k at the four corners
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        all_ge = all_ge && e[q][k] >= 0.0;
        all_le = all_le && e[q][k] <= 0.0;
        lt = lt && e[q][k] < 0.0;
        gt = gt && e[q][k] > 0.0;
      }
      some_lt = some_lt || lt;
      some_gt = some_gt || gt;
    }
    return (all_ge || all_le) ? 1 : ((some_lt && some_gt) ? -1 : 0);
  }
};

// the inside mask of one group (sample rows b0 .. b0 + RPG - 1 of cell column j; bit bb S + a is sample (a, b0 + bb))
template <int S, class Shape>
__device__ __forceinline__ unsigned long long scene_group_mask(const Shape& sh, const double (&xs)[S], int j, int b0, double y0, double y1, double dy, bool shortcuts) {
  using SG = SceneGroups<S>;
  if (S >= 4 && shortcuts) {
    const int d = sh.decide(xs[0], xs[S - 1], y0, y1);
    if (d > 0) return SG::ALL;
    if (d < 0) return 0ull;
  }
  unsigned long long m = 0ull;
#pragma unroll 1
  for (int bb = 0; bb < SG::RPG; ++bb) {
    const double ys = scene_coord<S>(j, b0 + bb, dy);
    unsigned r = 0u;
#pragma unroll
    for (int a = 0; a < S; ++a) r |= (unsigned)sh.in(xs[a], ys) << a;
    m |= (unsigned long long)r << (bb * S);
  }
  return m;
}

// ------------------------------------------------------------------ the pass
// Grid: x over the columns 0 .. ny + 1 in blocks of 256, y over the stored rows (k_init_F's).  shapes: n records of SHR_N doubles,
// validated by the host (runtime/scene.h).  words: SCW_SLOTS slots of SCW_STRIDE words, zeroed in front of the launch.
template <typename T, int S>
__global__ __launch_bounds__(256) void k_scene(Geom g, T* __restrict__ F, T* __restrict__ F2, const double* __restrict__ shapes, int n, int clear, int shortcuts,
                                                double dx, double dy, int rep_lo, int rep_hi, unsigned long long* __restrict__ words) {
  using SG = SceneGroups<S>;
  constexpr int TOTAL = S * S;
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const int i = g.row_lo + (int)blockIdx.y;
  const bool live = j <= g.ny + 1 && i <= g.row_hi;
  bool painted = false, mixed = false;
  if (live) {
    double xs[S];
#pragma unroll
    for (int a = 0; a < S; ++a) xs[a] = scene_coord<S>(i, a, dx);
    int n_liq = 0, n_gas = 0;
#pragma unroll 1
    for (int gq = 0; gq < SG::NG; ++gq) {
      const int b0 = gq * SG::RPG;
      const double y0 = scene_coord<S>(j, b0, dy), y1 = scene_coord<S>(j, b0 + SG::RPG - 1, dy);
      unsigned long long liq = 0ull, gas = 0ull;
      for (int k = 0; k < n; ++k) {   // (k and the record are wave-uniform)
        const double* const r = shapes + (size_t)k * SHR_N;
        const int kind = (int)r[SHR_KIND];
        unsigned long long m;
        if (kind == SHK_BOX) {
          m = scene_group_mask<S>(ScBox{r[2], r[3], r[4], r[5], r[6], r[7]}, xs, j, b0, y0, y1, dy, shortcuts != 0);
        } else if (kind == SHK_ELLIPSE) {
          m = scene_group_mask<S>(ScEllipse(ScBox{r[2], r[3], r[4], r[5], r[6], r[7]}), xs, j, b0, y0, y1, dy, shortcuts != 0);
        } else if (kind == SHK_HALFPLANE) {
          m = scene_group_mask<S>(ScHalfplane{r[2], r[3], r[4], r[5]}, xs, j, b0, y0, y1, dy, shortcuts != 0);
        } else {
          m = scene_group_mask<S>(ScTriangle{r[2], r[3], r[4], r[5], r[6], r[7]}, xs, j, b0, y0, y1, dy, shortcuts != 0);
        }
        if ((int)r[SHR_PHASE] == SHP_LIQUID) { liq |= m; gas &= ~m; }
        else { gas |= m; liq &= ~m; }
      }
      n_liq += __popcll(liq);
      n_gas += __popcll(gas);
    }
    if (clear) n_gas = TOTAL - n_liq;
    const int n_keep = TOTAL - n_liq - n_gas;
    painted = n_keep < TOTAL;
    mixed = n_liq != TOTAL && n_gas != TOTAL && n_keep != TOTAL;
    if (painted) {
      const size_t o = at(g, i, j);
      double acc = (double)n_liq;
      if (n_keep) acc += mul_rounded((double)n_keep, (double)F[o]);
      const T val = (T)mul_rounded(acc, 1.0 / TOTAL);
      F[o] = val;
      F2[o] = val;
    }
  }
  // the counters: the interior cells of the reported rows; one integer atomic per wave with something to count
  const bool counted = live && i >= rep_lo && i <= rep_hi && j >= 1 && j <= g.ny;
  const unsigned long long np = __popcll(__ballot(counted && painted)), nm = __popcll(__ballot(counted && mixed));
  if ((threadIdx.x & 63) == 0) {
    const unsigned wave = (blockIdx.y * gridDim.x + blockIdx.x) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    unsigned long long* const slot = words + (size_t)(wave & (SCW_SLOTS - 1)) * SCW_STRIDE;
    if (np) atomicAdd(slot + SCW_PAINTED, np);
    if (nm) atomicAdd(slot + SCW_MIXED, nm);
  }
}

}  // namespace vof
