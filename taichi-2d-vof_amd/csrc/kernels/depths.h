// kernels/depths.h -- both marginals of F, the top of the liquid per row and the front on the floor in one pass (k_depths, k_depths_fold, k_depths_finish), and the fixed sensors that read them (k_gauge_sample)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_depths, vof_gauges_*).  One pass over F on the
// cells i in [g.ilo, g.ihi] (the caller passes the handle's owned interior rows there), j in [1, ny]; every F is
// converted to double on load.  With f = (double)F[i,j], in this order (a NumPy restatement follows it term for term,
// tests/_depths_np.py):
//
//   depth_i[i]  1. a lane holds the V = 2 columns j0, j0 + 1 of the row:  l = 0.0;  l += f[i,j0];  l += f[i,j0+1]   (a column > ny adds nothing)
//               2. lanes -> wave by __shfl_down with s = 32, 16, ... 1 (wave_fold of kernels/reduce.h): one partial per (row, tile of 128 columns)
//               3. k_depths_fold, one lane per row:  d = partial of tile 0;  d += partial of tile 1;  ...  in ascending tile order
//   depth_j[j]  1. a lane owns its columns over the R rows of its chunk:  c = 0.0;  c += f[i,j] for i ascending: one partial per (chunk, column)
//               2. k_depths_fold, one lane per column:  d = 0.0;  d += partial of chunk 0;  d += partial of chunk 1;  ...  in ascending chunk order
//   top[i]      the largest j with f[i,j] >= 0.5, 0 if there is none (a NaN fails the comparison: not a member)
//   FRONT_LO    the smallest, FRONT_HI the largest i with f[i,1] >= 0.5; 0 if there is none
//   TOP_J       the maximum of top
//   SUM         s = 0.0;  s += depth_i[i] for i ascending, one row after the other
// The chunk length R is the launch's (depths_chunk of runtime/depths.h: the cells-per-wave rule with 2 and 32); chunk c
// holds the rows g.ilo + c R .. g.ilo + c R + R - 1.  The sums take the raw F, not a clamp of it: a NaN reaches depth_i
// of its row, depth_j of its column and SUM, nothing else.  No contraction is possible: there are only additions.
//
// top and the fronts are integers: the wave finds its largest member column (ballot, the highest lane), then one 32-bit
// integer atomicMax per (row, tile) with a member on words zeroed in front of the launch (FRONT_LO as the maximum of
// kFrontLoBase - i) -- integers: whatever the arrival order, the same state gives the same bytes.  No floating-point
// atomics, no LDS, no scratch, plain vector stores.  Traffic: F once, the partials once each way.
//
// A gauge (k_gauge_sample, one per lane) is a fixed position (X, Y): U, V, F are the bilinear samples of kernels/tracers.h
// (tr_cell / tr_load / tr_value, with their offsets and clamps), P is p sampled with F's offsets (0.5, 0.5) and clamps;
//   ig = (int)floor(X * dxi) + 1  clamped to [1, nx]      DEPTH = depth_i[ig] * dy      TOP = (double)top[ig]
// with depth_i and top of the k_depths pass in front of it.
#pragma once
#include "cells.h"
#include "tracers.h"

namespace vof {

// slots of the summary of vof_depths, of a gauge's row and of the gauges' summary (= VOF_DEPTH_SUM_*, VOF_GAUGE_* of include/vof2d.h)
enum : int { DPS_ROWS = 0, DPS_ISTEP, DPS_FRONT_LO, DPS_FRONT_HI, DPS_TOP_J, DPS_SUM, DPS_N = 8 };
enum : int { GA_X = 0, GA_Y, GA_U, GA_V, GA_F, GA_P, GA_DEPTH, GA_TOP, GA_N = 8 };
enum : int { GAS_COUNT = 0, GAS_ISTEP, GAS_RECORDS, GAS_N = 8 };
// the integer words behind top[rows], zeroed with it: max i, max (kFrontLoBase - i) over the rows with liquid on the floor
enum : int { DPW_FRONT_HI = 0, DPW_FRONT_LO, DPW_N };
constexpr int kFrontLoBase = 0x7fffffff;

// ------------------------------------------------------------------ the pass over F
// rowpart: (rows, ntj) doubles; colpart: (chunks, ny) doubles, every one of them stored by exactly one lane; top: rows ints, then the
// DPW_N words, zeroed in front of the launch.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_depths(Geom g, const T* __restrict__ F, int R, double* __restrict__ rowpart, double* __restrict__ colpart,
                                                 int* __restrict__ top) {
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb)) return;
  const int ny = g.ny, ntj = g.ntj, lane = (int)(threadIdx.x & 63);
  const int tj = (j0 - 1) / (64 * V);
  int* const words = top + (g.ihi - g.ilo + 1);
  double col[V];
#pragma unroll
  for (int q = 0; q < V; ++q) col[q] = 0.0;
  size_t o = at(g, ra, j0);
  T f[V];
  load_s<T, V>(f, F + o);
  for (int i = ra; i <= rb; ++i) {
    T fn[V];
    load_s<T, V>(fn, F + o + g.pitch);   // the next row in flight under this one's folds (row rb + 1 <= row_hi is stored: not used)
    double w[1] = {0.0};
    int m = 0;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (j0 + q <= ny) {
        const double fd = (double)f[q];
        w[0] += fd;
        col[q] += fd;
        if (fd >= 0.5) m = j0 + q;
      }
    }
    wave_fold<1, 0>(w);
    // the largest member column of the wave: the lanes' columns ascend with the lane
    const unsigned long long has = __ballot(m != 0);
    const int r = i - g.ilo;
    if (has) {
      const int hi = 63 - __builtin_clzll(has);
      const int mj = __shfl(m, hi, 64);
      if (lane == 0) atomicMax(top + r, mj);
    }
    if (lane == 0) {
      rowpart[(size_t)r * ntj + tj] = w[0];
      if (j0 == 1 && (double)f[0] >= 0.5) {
        atomicMax(words + DPW_FRONT_HI, i);
        atomicMax(words + DPW_FRONT_LO, kFrontLoBase - i);
      }
    }
#pragma unroll
    for (int q = 0; q < V; ++q) f[q] = fn[q];
    o += g.pitch;
  }
  const int ch = (ra - g.ilo) / R;
#pragma unroll
  for (int q = 0; q < V; ++q)
    if (j0 + q <= ny) colpart[(size_t)ch * ny + (j0 + q - 1)] = col[q];
}

// ------------------------------------------------------------------ the partials -> depth_i, depth_j
// One lane per row (blocks 0 .. row_blocks - 1), then one lane per column (the blocks behind): the loads of a column lane
// are coalesced across the wave, chunk after chunk.  The launch boundary in front of it makes the partials visible.
__global__ __launch_bounds__(256) void k_depths_fold(const double* __restrict__ rowpart, const double* __restrict__ colpart, int rows, int ntj, int chunks, int ny,
                                                      int row_blocks, double* __restrict__ depth_i, double* __restrict__ depth_j) {
  if ((int)blockIdx.x < row_blocks) {
    const int r = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (r >= rows) return;
    const double* const p = rowpart + (size_t)r * ntj;
    double d = p[0];
    for (int t = 1; t < ntj; ++t) d += p[t];
    depth_i[r] = d;
  } else {
    const int c = ((int)blockIdx.x - row_blocks) * 256 + (int)threadIdx.x;
    if (c >= ny) return;
    double d = 0.0;
    int ch = 0;
    for (; ch + 16 <= chunks; ch += 16) {   // sixteen loads in flight, added in ascending order
      double v[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) v[k] = colpart[(size_t)(ch + k) * ny + c];
#pragma unroll
      for (int k = 0; k < 16; ++k) d += v[k];
    }
    for (; ch < chunks; ++ch) d += colpart[(size_t)ch * ny + c];
    depth_j[c] = d;
  }
}

// ------------------------------------------------------------------ depth_i, top, the words -> the summary
// ONE wave.  SUM is depth_i added one row after the other: the lanes load 64 rows at a time (coalesced, the next 64 in flight),
// the additions run through them in lane order -- a row past the last adds 0.0, which changes no bit of a sum that started
// from 0.0.  TOP_J: the lanes' maxima of top, then the wave's (integers).
__global__ __launch_bounds__(64) void k_depths_finish(const double* __restrict__ depth_i, const int* __restrict__ top, int rows, double* __restrict__ summary,
                                                       double istep) {
  const int lane = (int)threadIdx.x;
  const int* const words = top + rows;
  double s = 0.0;
  int tmax = 0;
  double x = lane < rows ? depth_i[lane] : 0.0;
  int t = lane < rows ? top[lane] : 0;
  for (int r0 = 0; r0 < rows; r0 += 64) {
    const int rn = r0 + 64 + lane;
    const double xn = rn < rows ? depth_i[rn] : 0.0;
    const int tn = rn < rows ? top[rn] : 0;
    tmax = t > tmax ? t : tmax;
    const int xlo = __double2loint(x), xhi = __double2hiint(x);
#pragma unroll
    for (int l = 0; l < 64; ++l) s += __hiloint2double(__builtin_amdgcn_readlane(xhi, l), __builtin_amdgcn_readlane(xlo, l));   // (lane l's row, in lane order)
    x = xn; t = tn;
  }
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    const int other = __shfl_down(tmax, sft, 64);
    tmax = other > tmax ? other : tmax;
  }
  tmax = __shfl(tmax, 0, 64);
  if (lane >= DPS_N) return;
  double out = 0.0;
  if (lane == DPS_ROWS) out = (double)rows;
  else if (lane == DPS_ISTEP) out = istep;
  else if (lane == DPS_FRONT_LO) out = words[DPW_FRONT_LO] ? (double)(kFrontLoBase - words[DPW_FRONT_LO]) : 0.0;
  else if (lane == DPS_FRONT_HI) out = (double)words[DPW_FRONT_HI];
  else if (lane == DPS_TOP_J) out = (double)tmax;
  else if (lane == DPS_SUM) out = s;
  summary[lane] = out;
}

// ------------------------------------------------------------------ the gauges' rows: X, Y, then U, V, F, P sampled there, DEPTH and TOP of the row above X
// xy: n x 2 doubles; rows: n x GA_N doubles (64 bytes a row, 16-byte aligned).  depth_i, top: of the k_depths pass on this
// state, indexed by i - first (the handle is a whole domain: first = 1).
template <typename T>
__global__ __launch_bounds__(256) void k_gauge_sample(Geom g, TracerConsts c, const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v,
                                                       const T* __restrict__ p, long long n, const double* __restrict__ xy, const double* __restrict__ depth_i,
                                                       const int* __restrict__ top, int first, double dy, double* __restrict__ rows) {
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double2 pos = reinterpret_cast<const double2*>(xy)[k];
  const double x = pos.x, y = pos.y;
  const TrCell cu = tr_cell<true, false>(g, c, x, y), cv = tr_cell<false, true>(g, c, x, y), cf = tr_cell<false, false>(g, c, x, y);
  const TrQuad<T> qu = tr_load(u, cu.o, g.pitch), qv = tr_load(v, cv.o, g.pitch), qf = tr_load(F, cf.o, g.pitch), qp = tr_load(p, cf.o, g.pitch);
  int ig = (int)__builtin_floor(x * c.dxi) + 1;
  ig = ig < 1 ? 1 : (ig > g.nx ? g.nx : ig);
  const double depth = depth_i[ig - first] * dy, tp = (double)top[ig - first];
  double2* const row = reinterpret_cast<double2*>(rows + (size_t)k * GA_N);
  row[0] = make_double2(x, y);
  row[1] = make_double2(tr_value(qu, cu), tr_value(qv, cv));
  row[2] = make_double2(tr_value(qf, cf), tr_value(qp, cf));
  row[3] = make_double2(depth, tp);
}

}  // namespace vof
