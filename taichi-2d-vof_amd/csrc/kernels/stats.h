// kernels/stats.h -- per-cell statistics over a run (k_stats, k_stats_fill, k_stats_summary, kStatsRow): running sums of F, u, v and their products, envelopes, wet time, arrival step
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_stats_*).  The accumulators are planes of doubles for
// both field types, one value per interior cell: element (i, j) of a plane at [(i - 1) * pitch + (j - 1)], the pitch a whole number of
// wave tiles (runtime/carve.h, stats_pitch), so that the V columns of a lane are one aligned vector of V doubles in every plane and
// no lane's vector leaves its row.  One sample is one pass of k_stats over F, u, v on the cells i in [g.ilo, g.ihi], j in [1, ny]:
// every operand converted to double on load; then, per cell, in this order (tests/_stats_np.py restates it term for term):
//   f  = F[i,j]    Fc = fmin(fmax(f, 0), 1)    uc = (u[i,j] + u[i+1,j]) * 0.5    vc = (v[i,j] + v[i,j+1]) * 0.5     (clamp01, face_mean of kernels/cells.h)
//   SUM_F += Fc   SUM_F2 += Fc * Fc   SUM_U += uc   SUM_V += vc   SUM_UU += uc * uc   SUM_VV += vc * vc   SUM_UV += uc * vc
//   SUM_FU += Fc * uc   SUM_FV += Fc * vc                                                                      (group MOMENTS)
//   s2 = uc * uc + vc * vc    MAX_SPEED2 = diag_max(MAX_SPEED2, s2)    MAX_F = diag_max(MAX_F, Fc)
//   wet = (Fc >= level)    WET += wet ? 1.0 : 0.0    if (wet && ARRIVAL < 0) ARRIVAL = (double)istep                   (group ENVELOPE)
// The plain clamp takes a NaN F to Fc = 0 (fmax returns its other operand), as in k_diag: such a cell is dry and its F sums stay finite; a
// NaN u or v makes the sums it enters NaN and, by diag_max (a NaN operand counts as +inf), MAX_SPEED2 = +inf.  Every product is rounded
// on its own in either build: it passes through mul_rounded of kernels/cells.h, which no contraction reaches.
//
// Each cell's accumulation is a sequential chain over the samples: no order of lanes, waves or blocks enters a plane, so the bits
// depend on the samples alone.  Traffic per sample and cell: F, v once and u once (row i + 1 of one iteration is row i of the next),
// every plane of the chosen groups read once and written once as vectors of V doubles.  No LDS, no atomics, no scratch.  MASK is a
// template argument: a group that is off has no load, no store and no register.  Two choices settled by measurement at 4096^2 fp64,
// both groups (profiles/stats.md): the plane loads and stores carry the non-temporal hint (650 us a sample against 729 without: the
// planes of a sample are many times the last-level cache), and the field and plane loads of TWO rows are issued before the first of
// them is computed (650 us against 687 with one row, at 251 VGPRs against 127).
#pragma once
#include "cells.h"

namespace vof {

// the planes (= VOF_STATS_* of include/vof2d.h), the groups and the slots of the summary
enum : int { ST_SUM_F = 0, ST_SUM_F2, ST_SUM_U, ST_SUM_V, ST_SUM_UU, ST_SUM_VV, ST_SUM_UV, ST_SUM_FU, ST_SUM_FV, ST_MAX_F, ST_MAX_SPEED2, ST_WET, ST_ARRIVAL, ST_PLANES };
enum : int { STM_MOMENTS = 1, STM_ENVELOPE = 2 };
enum : int { STS_SAMPLES = 0, STS_ISTEP_FIRST, STS_ISTEP_LAST, STS_MASK, STS_LEVEL, STS_CELLS, STS_EVER_WET, STS_MAX_SPEED2, STS_N = 16 };
constexpr int kStatsMoments = ST_MAX_F, kStatsEnvelope = ST_PLANES - ST_MAX_F;
constexpr int kStatsPart = 2;   // doubles per block in the partials buffer of the summary: one sum (EVER_WET), one maximum (MAX_SPEED2)

// what a launch gets of the planes: the base of each (nullptr: its group is off) and their common pitch in doubles
struct StatsPlanes { double* p[ST_PLANES]; long long pitch; };

// the V doubles of a lane in a plane, stored whole (load_s of kernels/common.h is the load that goes with it)
template <int V>
__device__ __forceinline__ void st_store(double* __restrict__ p, const double (&c)[V]) {
  typedef double vec_t __attribute__((ext_vector_type(V)));
  vec_t k;
#pragma unroll
  for (int q = 0; q < V; ++q) k[q] = c[q];
  __builtin_nontemporal_store(k, reinterpret_cast<vec_t*>(p));
}
constexpr int kStatsRowsInFlight = 2;

// N consecutive rows from row offsets o (fields) and po (planes): every load of the N rows first, then the cells, then the stores.
// uw: row i of u on entry, row i + N on return.
template <typename T, int V, int MASK, int N>
__device__ __forceinline__ void st_rows(const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v, const StatsPlanes& pl, size_t o, size_t po,
                                        int64_t pitch, T (&uw)[V], double level, double istep) {
  T f[N][V], ue[N][V];
  Row<T, V> vr[N];
  double m[N][kStatsMoments][V], ev[N][kStatsEnvelope][V];
#pragma unroll
  for (int n = 0; n < N; ++n) {
    load_s<T, V>(f[n], F + o + n * pitch);
    load_c<T, V>(ue[n], u + o + (n + 1) * pitch);
    load_row<T, V>(vr[n], v + o + n * pitch);
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const size_t pn = po + (size_t)n * (size_t)pl.pitch;
    if constexpr ((MASK & STM_MOMENTS) != 0) {
#pragma unroll
      for (int k = 0; k < kStatsMoments; ++k) load_s<double, V>(m[n][k], pl.p[k] + pn);
    }
    if constexpr ((MASK & STM_ENVELOPE) != 0) {
#pragma unroll
      for (int k = 0; k < kStatsEnvelope; ++k) load_s<double, V>(ev[n][k], pl.p[ST_MAX_F + k] + pn);
    }
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const Cell c = cell_at<T, V>(q, f[n], n == 0 ? uw : ue[n > 0 ? n - 1 : 0], ue[n], vr[n]);
      const double Fc = clamp01(c.f);
      const double uc = face_mean(c.w, c.e), vc = face_mean(c.s, c.n);
      const double uu = mul_rounded(uc, uc), vv = mul_rounded(vc, vc);
      if constexpr ((MASK & STM_MOMENTS) != 0) {
        m[n][ST_SUM_F][q] += Fc;
        m[n][ST_SUM_F2][q] += mul_rounded(Fc, Fc);
        m[n][ST_SUM_U][q] += uc;
        m[n][ST_SUM_V][q] += vc;
        m[n][ST_SUM_UU][q] += uu;
        m[n][ST_SUM_VV][q] += vv;
        m[n][ST_SUM_UV][q] += mul_rounded(uc, vc);
        m[n][ST_SUM_FU][q] += mul_rounded(Fc, uc);
        m[n][ST_SUM_FV][q] += mul_rounded(Fc, vc);
      }
      if constexpr ((MASK & STM_ENVELOPE) != 0) {
        const double s2 = uu + vv;
        ev[n][ST_MAX_SPEED2 - ST_MAX_F][q] = diag_max(ev[n][ST_MAX_SPEED2 - ST_MAX_F][q], s2);
        ev[n][0][q] = diag_max(ev[n][0][q], Fc);
        const bool wet = Fc >= level;
        ev[n][ST_WET - ST_MAX_F][q] += wet ? 1.0 : 0.0;
        if (wet && ev[n][ST_ARRIVAL - ST_MAX_F][q] < 0.0) ev[n][ST_ARRIVAL - ST_MAX_F][q] = istep;
      }
    }
  }
#pragma unroll
  for (int n = 0; n < N; ++n) {
    const size_t pn = po + (size_t)n * (size_t)pl.pitch;
    if constexpr ((MASK & STM_MOMENTS) != 0) {
#pragma unroll
      for (int k = 0; k < kStatsMoments; ++k) st_store<V>(pl.p[k] + pn, m[n][k]);
    }
    if constexpr ((MASK & STM_ENVELOPE) != 0) {
#pragma unroll
      for (int k = 0; k < kStatsEnvelope; ++k) st_store<V>(pl.p[ST_MAX_F + k] + pn, ev[n][k]);
    }
  }
#pragma unroll
  for (int q = 0; q < V; ++q) uw[q] = ue[N - 1][q];
}

// ------------------------------------------------------------------ one sample
// The march of k_diag (cell_tile: chunks of R rows of [g.ilo, g.ihi]); nothing crosses lanes here, so a lane whose first column lies
// right of ny leaves.  A lane that holds column ny alone (ny odd) carries column ny + 1 along: the pad of the planes' rows.
template <typename T, int V, int MASK>
__global__ __launch_bounds__(256) void k_stats(Geom g, const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v, int R, StatsPlanes pl,
                                                double level, double istep) {
  static_assert((V * sizeof(double)) % 16 == 0, "a lane moves whole 16-byte vectors of every plane");
  static_assert(MASK >= 1 && MASK <= 3, "at least one group");
  constexpr int U = kStatsRowsInFlight;
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb) || j0 > g.ny) return;
  const int64_t pitch = g.pitch;
  size_t o = at(g, ra, j0);
  size_t po = (size_t)(ra - 1) * (size_t)pl.pitch + (size_t)(j0 - 1);
  T uw[V];
  load_c<T, V>(uw, u + o);
  int i = ra;
  for (; i + U - 1 <= rb; i += U) {
    st_rows<T, V, MASK, U>(F, u, v, pl, o, po, pitch, uw, level, istep);
    o += (size_t)U * pitch;
    po += (size_t)U * (size_t)pl.pitch;
  }
  for (; i <= rb; ++i) {
    st_rows<T, V, MASK, 1>(F, u, v, pl, o, po, pitch, uw, level, istep);
    o += pitch;
    po += (size_t)pl.pitch;
  }
}

// ------------------------------------------------------------------ a plane set to one value (vof_stats_begin: ARRIVAL = -1)
__global__ __launch_bounds__(256) void k_stats_fill(double* __restrict__ p, long long n, double value) {
  for (long long k = (long long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long long)gridDim.x * 256) p[k] = value;
}

// ------------------------------------------------------------------ the summary: EVER_WET, MAX_SPEED2 over the cells
// One pass over the planes ARRIVAL and MAX_SPEED2 in the shape of k_cg_sum, then the reduction of kernels/reduce.h: the count of
// the cells with ARRIVAL >= 0 (a sum of ones: exact) and the maximum of MAX_SPEED2 (never NaN: diag_max formed it).
template <int V>
__global__ __launch_bounds__(256) void k_stats_summary(Geom g, const double* __restrict__ arrival, const double* __restrict__ speed2, long long ppitch, int R,
                                                        double* __restrict__ part) {
  int j0, ra, rb;
  const bool active = cell_tile<V>(g, R, j0, ra, rb);
  double acc[kStatsPart] = {0.0, 0.0};
  if (active) {
    size_t po = (size_t)(ra - 1) * (size_t)ppitch + (size_t)(j0 - 1);
    for (int i = ra; i <= rb; ++i) {
      double a[V], s[V];
      load_c<double, V>(a, arrival + po);
      load_c<double, V>(s, speed2 + po);
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (j0 + q <= g.ny) {
          acc[0] += a[q] >= 0.0 ? 1.0 : 0.0;
          acc[1] = __builtin_fmax(acc[1], s[q]);
        }
      po += (size_t)ppitch;
    }
  }
  block_publish<1, 1>(acc, part);
}
constexpr RowMap<1, 1> kStatsRow = {kStatsPart, {{ROW_VALUE, 0}, {ROW_VALUE, 1}}, {0.0, 0.0}};   // k_row_finish (kernels/cells.h) folds them into two doubles: EVER_WET, MAX_SPEED2

}  // namespace vof
