// kernels/tracers.h -- passive tracer particles moved with the flow on the device (k_tracer_advance, k_tracer_sample, k_tracer_finish)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order).  Unlike the stencil kernels these do not march a tile: ONE TRACER PER LANE,
// a gather of 2 x 2 cells of u, v (and F) around each position.
//
// Extension, not part of the reference (include/vof2d.h, vof_tracers_*).  All arithmetic is in double,
// whatever the fields' type: every field operand is converted to double on load.  dxi, dyi, Lx, Ly, dt are the
// Python-double values vof_get_param returns.  In this order (a NumPy restatement follows it term for term,
// tests/_tracers_np.py), every sum and product as written, `c ? x : y` a select on exactly that comparison:
//
//   where the fields sit   u[i,j] at ((i - 1) dx, (j - 0.5) dy)    v[i,j] at ((i - 0.5) dx, (j - 1) dy)    F[i,j] at ((i - 0.5) dx, (j - 0.5) dy)
//   offsets (ox, oy)       u: (0, 0.5)    v: (0.5, 0)    F: (0.5, 0.5)
//   sample of f at (x, y)  s = x * dxi + ox                          t = y * dyi + oy
//                          ib = floor(s) + (ox == 0 ? 1 : 0)         clamped to [1, nx] for u, to [0, nx] for v and F
//                          jb = floor(t) + (oy == 0 ? 1 : 0)         clamped to [1, ny] for v, to [0, ny] for u and F
//                          a = s - (ib - (ox == 0 ? 1 : 0))          b = t - (jb - (oy == 0 ? 1 : 0))       (of the clamped ib, jb)
//                          lo = f[ib,jb] + a * (f[ib+1,jb] - f[ib,jb])
//                          hi = f[ib,jb+1] + a * (f[ib+1,jb+1] - f[ib,jb+1])
//                          value = lo + b * (hi - lo)
//     With these clamps the four loads lie inside the stored (nx + 2, ny + 2) array for every position of the closed domain.
//   clamp(c, L)            c < 0 ? 0 : (c > L ? L : c)               (keeps a NaN)
//   one advance by h       k1 = (u, v)(x, y)
//                          xm = x + (0.5 * h) * k1.u                 ym = y + (0.5 * h) * k1.v
//                          xm or ym not finite: LOST; else xm = clamp(xm, Lx), ym = clamp(ym, Ly)
//                          k2 = (u, v)(xm, ym)
//                          x' = x + h * k2.u                         y' = y + h * k2.v
//                          x' or y' not finite: LOST; else x' = clamp(x', Lx), y' = clamp(y', Ly)
//   LOST                   x = y = NaN, for good: a lost tracer is recognised by x != x in front of every load; it is not moved
//                          or sampled again, its U, V, F read NaN
//   a row                  TR_N doubles: X, Y, then U, V, F sampled at (X, Y); the unused slots read 0
// No contraction (-ffp-contract=off): each term is the bits of the line above.  The eight (advance) or twelve (sample) loads
// of a stage do not depend on each other: they are issued in front of the arithmetic.  No LDS, no scratch.
//
// The counts LOST and IN_LIQUID (sampled F >= 0.5; a lost tracer is in neither phase) are 32-bit integer atomic adds on two
// words zeroed in front of the launch -- integers: whatever the arrival order, the same state gives the same bytes -- and
// k_tracer_finish turns them into the summary.  No floating-point atomics.
#pragma once
#include "common.h"

namespace vof {

// slots of a row and of the summary (= VOF_TRACER_* of include/vof2d.h)
enum : int { TR_X = 0, TR_Y, TR_U, TR_V, TR_F, TR_N = 8 };
enum : int { TRS_COUNT = 0, TRS_LOST, TRS_IN_LIQUID, TRS_ISTEP, TRS_TIME, TRS_N = 8 };
enum : int { TRC_LOST = 0, TRC_IN_LIQUID, TRC_N };   // the integer counters behind the summary

struct TracerConsts { double dxi, dyi, Lx, Ly; };

// the 2 x 2 cells of a sample: the offset of f[ib, jb] and the two weights
struct TrCell { size_t o; double a, b; };
template <typename T> struct TrQuad { T f00, f10, f01, f11; };   // f[ib,jb], f[ib+1,jb], f[ib,jb+1], f[ib+1,jb+1]

// OX0: ox == 0 (u), else 0.5; OY0: oy == 0 (v), else 0.5
template <bool OX0, bool OY0>
__device__ __forceinline__ TrCell tr_cell(const Geom& g, const TracerConsts& c, double x, double y) {
  const double s = x * c.dxi + (OX0 ? 0.0 : 0.5), t = y * c.dyi + (OY0 ? 0.0 : 0.5);
  constexpr int i0 = OX0 ? 1 : 0, j0 = OY0 ? 1 : 0;
  int ib = (int)__builtin_floor(s) + i0, jb = (int)__builtin_floor(t) + j0;
  ib = ib < i0 ? i0 : (ib > g.nx ? g.nx : ib);
  jb = jb < j0 ? j0 : (jb > g.ny ? g.ny : jb);
  return {at(g, ib, jb), s - (double)(ib - i0), t - (double)(jb - j0)};
}
template <typename T>
__device__ __forceinline__ TrQuad<T> tr_load(const T* __restrict__ f, size_t o, int64_t pitch) {
  return {f[o], f[o + pitch], f[o + 1], f[o + pitch + 1]};
}
template <typename T>
__device__ __forceinline__ double tr_value(const TrQuad<T>& q, const TrCell& c) {
  const double f00 = (double)q.f00, f10 = (double)q.f10, f01 = (double)q.f01, f11 = (double)q.f11;
  const double lo = f00 + c.a * (f10 - f00);
  const double hi = f01 + c.a * (f11 - f01);
  return lo + c.b * (hi - lo);
}
__device__ __forceinline__ bool tr_finite(double x) { return __builtin_fabs(x) < __builtin_huge_val(); }   // (false for a NaN)
__device__ __forceinline__ double tr_clamp(double c, double L) { return c < 0.0 ? 0.0 : (c > L ? L : c); }

// ------------------------------------------------------------------ one midpoint step of every tracer on the frozen u, v
// xy: n x 2 doubles, updated in place.
template <typename T>
__global__ __launch_bounds__(256) void k_tracer_advance(Geom g, TracerConsts c, const T* __restrict__ u, const T* __restrict__ v, double h, long long n,
                                                         double* __restrict__ xy) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double2* const slot = reinterpret_cast<double2*>(xy) + k;
  const double2 p = *slot;
  const double x = p.x, y = p.y;
  if (x != x) return;   // lost
  const double nan = __builtin_nan("");
  double xn = nan, yn = nan;
  const TrCell cu1 = tr_cell<true, false>(g, c, x, y), cv1 = tr_cell<false, true>(g, c, x, y);
  const TrQuad<T> qu1 = tr_load(u, cu1.o, g.pitch), qv1 = tr_load(v, cv1.o, g.pitch);
  const double hh = 0.5 * h;
  double xm = x + hh * tr_value(qu1, cu1), ym = y + hh * tr_value(qv1, cv1);
  if (tr_finite(xm) && tr_finite(ym)) {
    xm = tr_clamp(xm, c.Lx); ym = tr_clamp(ym, c.Ly);
    const TrCell cu2 = tr_cell<true, false>(g, c, xm, ym), cv2 = tr_cell<false, true>(g, c, xm, ym);
    const TrQuad<T> qu2 = tr_load(u, cu2.o, g.pitch), qv2 = tr_load(v, cv2.o, g.pitch);
    const double x2 = x + h * tr_value(qu2, cu2), y2 = y + h * tr_value(qv2, cv2);
    if (tr_finite(x2) && tr_finite(y2)) { xn = tr_clamp(x2, c.Lx); yn = tr_clamp(y2, c.Ly); }
  }
  *slot = make_double2(xn, yn);
}

// ------------------------------------------------------------------ the rows: X, Y and U, V, F sampled there
// rows: n x TR_N doubles (64 bytes a row, 16-byte aligned).  counts: the TRC_N words (zeroed in front of the launch), or
// nullptr for a snapshot, which has no summary.
template <typename T>
__global__ __launch_bounds__(256) void k_tracer_sample(Geom g, TracerConsts c, const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v, long long n,
                                                        const double* __restrict__ xy, double* __restrict__ rows, unsigned* __restrict__ counts) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double2 p = reinterpret_cast<const double2*>(xy)[k];
  const double x = p.x, y = p.y;
  const bool lost = x != x;
  double U = x, V = x, Fv = x;   // (NaN if lost)
  if (!lost) {
    const TrCell cu = tr_cell<true, false>(g, c, x, y), cv = tr_cell<false, true>(g, c, x, y), cf = tr_cell<false, false>(g, c, x, y);
    const TrQuad<T> qu = tr_load(u, cu.o, g.pitch), qv = tr_load(v, cv.o, g.pitch), qf = tr_load(F, cf.o, g.pitch);
    U = tr_value(qu, cu); V = tr_value(qv, cv); Fv = tr_value(qf, cf);
  }
  double2* const row = reinterpret_cast<double2*>(rows + (size_t)k * TR_N);
  row[0] = make_double2(x, y);
  row[1] = make_double2(U, V);
  row[2] = make_double2(Fv, 0.0);
  row[3] = make_double2(0.0, 0.0);
  if (counts) {
    if (lost) atomicAdd(counts + TRC_LOST, 1u);
    else if (Fv >= 0.5) atomicAdd(counts + TRC_IN_LIQUID, 1u);
  }
}

// ------------------------------------------------------------------ the counters -> the summary
// One wave; threads 0 .. TRS_N - 1 store one slot each (unused slots read 0).  The launch boundary in front of it is what
// makes the atomics of k_tracer_sample visible.
__global__ __launch_bounds__(64) void k_tracer_finish(const unsigned* __restrict__ counts, double* __restrict__ summary, double count, double istep, double time) {
  const int t = threadIdx.x;
  if (t >= TRS_N) return;
  double x = 0.0;
  if (t == TRS_COUNT) x = count;
  else if (t == TRS_LOST) x = (double)counts[TRC_LOST];
  else if (t == TRS_IN_LIQUID) x = (double)counts[TRC_IN_LIQUID];
  else if (t == TRS_ISTEP) x = istep;
  else if (t == TRS_TIME) x = time;
  summary[t] = x;
}

}  // namespace vof
