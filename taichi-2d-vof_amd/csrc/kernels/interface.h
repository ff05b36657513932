// kernels/interface.h -- PLIC interface segments extracted on the device (k_iface, k_iface_scan; scan_counts): Youngs' normal, the line in the cell, an ordered compaction
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
// Order of the rows: ascending (i, j), i first.  Three launches, no atomics:
//   k_iface<EMIT = false>  a wave marches its 64 * V columns over its chunk of rows with the rows i - 1, i, i + 1 of F in
//                          registers (each row of F is loaded once per chunk, plus two lead-in rows) and writes the number of
//                          segments of every (row, column tile) into cnt[(i - g.ilo) * ntj + tile]; the lengths and the
//                          degenerate count go through the reduction of kernels/reduce.h into one partial per block
//   k_iface_scan           one block: cnt -> exclusive offsets in place (thread t owns a run of consecutive entries; the
//                          runs' totals are scanned through LDS), and the summary
//   k_iface<EMIT = true>   recomputes the cells and stores segment k of a (row, tile) at row offset[(row, tile)] + k of
//                          the output, k being the segment's rank within the wave in column order (ballot + mbcnt over
//                          the lanes' V cells); rows from `cap` on are not stored
// Order of the LENGTH sum, fixed: a lane adds the lengths of its cells row by row, column by column; from there the
// reduction of kernels/reduce.h, two sums wide: one partial of kIfacePart doubles per block, folded by k_iface_scan (one
// block of 1024 threads).  The degenerate count travels the same way as a double (exact).
#pragma once
#include "cells.h"

namespace vof {

// slots of a row and of the summary (= VOF_IFACE_* of include/vof2d.h)
enum : int { IF_I = 0, IF_J, IF_X0, IF_Y0, IF_X1, IF_Y1, IF_NX, IF_NY, IF_N = 8 };
enum : int { IFS_SEGMENTS = 0, IFS_DEGENERATE, IFS_LENGTH, IFS_ISTEP, IFS_N = 4 };
constexpr int kIfaceScanThreads = 1024;
constexpr int kIfacePart = 2;   // doubles per block in the partials buffer: the length, the degenerate cells

struct IfaceConsts { double eps, one_m_eps, cx, cy, dx, dy; };

// The line of a mixed cell in the frame of a, b >= 0: the liquid is a xi + b eta < alpha; flip_x, flip_y: the mirrors that take the
// frame back to the cell's (mxsum < 0, mysum < 0).  What k_iface cuts into a segment and k_regrid_refine (kernels/regrid.h) into
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

// ------------------------------------------------------------------ the pass over F: count (+ length), or emit
// cnt: EMIT = false, written: segments per (row, tile); EMIT = true, read: the exclusive offsets k_iface_scan left there.
// part: kIfacePart doubles per block (slot 0: length, slot 1: degenerate cells) -- EMIT = false only.
// rows: the output, `cap` rows of IF_N doubles -- EMIT = true only.
template <typename T, int V, bool EMIT>
__global__ __launch_bounds__(256) void k_iface(Geom g, const T* __restrict__ F, int R, IfaceConsts c, int* __restrict__ cnt, double* __restrict__ part,
                                                double* __restrict__ rows, long long cap) {
  int j0, ra, rb;
  const bool active = cell_tile<V>(g, R, j0, ra, rb);
  double acc[kIfacePart] = {0.0, 0.0};
  int ndeg = 0;   // the lane's degenerate cells (an integer until the lanes are folded: one register, the same value)
  if (active) {
    const int ny = g.ny;
    const int64_t pitch = g.pitch;
    const int lane = threadIdx.x & 63;
    const int tile = (j0 - 1) / (64 * V);   // (wave-uniform)
    size_t o = at(g, ra, j0);
    Row<T, V> wm, w0, wp;
    load_row<T, V>(wm, F + o - pitch);
    load_row<T, V>(w0, F + o);
    for (int i = ra; i <= rb; ++i) {
      load_row<T, V>(wp, F + o + pitch);
      // which of the lane's cells are candidates (wave-uniform skip: most waves see no interface at all)
      bool cand[V];
      bool any = false;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const double f = (double)w0.c[q];
        cand[q] = j0 + q <= ny && c.eps < f && f < c.one_m_eps;
        any = any || cand[q];
      }
      int total = 0;
      if (__builtin_amdgcn_ballot_w64(any) != 0ull) {
        const long long base = EMIT ? (long long)cnt[(size_t)(i - g.ilo) * g.ntj + tile] : 0ll;
        int before = 0;   // segments of this row in the lanes below this one
        int kind[V];
        double seg[V][IF_N];
#pragma unroll
        for (int q = 0; q < V; ++q) {
          kind[q] = 0;
          if (cand[q]) {
            const double fm[3] = {(double)left_of(wm, q), (double)wm.c[q], (double)right_of(wm, q)};
            const double f0[3] = {(double)left_of(w0, q), (double)w0.c[q], (double)right_of(w0, q)};
            const double fp[3] = {(double)left_of(wp, q), (double)wp.c[q], (double)right_of(wp, q)};
            kind[q] = iface_cell(c, fm, f0, fp, i, j0 + q, seg[q]);
          }
          const unsigned long long b = __builtin_amdgcn_ballot_w64(kind[q] == 2);
          before += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
          total += __builtin_popcountll(b);
        }
        int rank = before;   // of the lane's first segment within the row's tile, in column order
#pragma unroll
        for (int q = 0; q < V; ++q) {
          if (kind[q] == 2) {
            if constexpr (EMIT) {
              const long long k = base + rank;
              if (k < cap) {
                Pack<double, 2>* dst = reinterpret_cast<Pack<double, 2>*>(rows + (size_t)k * IF_N);
#pragma unroll
                for (int m = 0; m < IF_N / 2; ++m) dst[m] = Pack<double, 2>{{seg[q][2 * m], seg[q][2 * m + 1]}};
              }
            } else {
              const double ddx = seg[q][IF_X1] - seg[q][IF_X0], ddy = seg[q][IF_Y1] - seg[q][IF_Y0];
              acc[0] += __builtin_sqrt(ddx * ddx + ddy * ddy);
            }
            ++rank;
          } else if (!EMIT && kind[q] == 1) {
            ++ndeg;
          }
        }
      }
      if (!EMIT && lane == 0) cnt[(size_t)(i - g.ilo) * g.ntj + tile] = total;
      wm = w0;
      w0 = wp;
      o += pitch;
    }
  }
  if constexpr (!EMIT) {
    acc[1] = (double)ndeg;
    block_publish<kIfacePart, 0>(acc, part);
  }
}

// ------------------------------------------------------------------ counts -> exclusive offsets, block partials -> summary
// Every thread of a ONE-block kernel of NT threads calls it (k_iface_scan, k_curv_scan of kernels/curvature.h).  Thread t owns the entries
// [t * run, (t + 1) * run) of cnt (run = ceil(n / threads)): it adds them up, the block scans the threads' totals (waves by __shfl_up,
// the NT / 64 wave totals by thread 0 through LDS), and the thread writes its entries' exclusive offsets back.  Returns the total of all
// entries to every thread.  wsum: NT / 64 + 1 words of LDS.
template <int NT>
__device__ __forceinline__ long long scan_counts(int* __restrict__ cnt, long long n, long long* wsum) {
  constexpr int NW = NT / 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long long run = (n + NT - 1) / NT;
  const long long e0 = (long long)t * run, e1 = e0 + run < n ? e0 + run : n;
  long long mine = 0;
  for (long long e = e0; e < e1; ++e) mine += cnt[e];
  long long incl = mine;   // inclusive scan over the wave's lanes
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const long long up = __shfl_up(incl, s, 64);
    if (lane >= s) incl += up;
  }
  if (lane == 63) wsum[wave + 1] = incl;
  __syncthreads();
  if (t == 0) {
    wsum[0] = 0;
    for (int w = 1; w <= NW; ++w) wsum[w] += wsum[w - 1];
  }
  __syncthreads();
  long long off = wsum[wave] + incl - mine;
  for (long long e = e0; e < e1; ++e) {
    const int k = cnt[e];
    cnt[e] = (int)off;
    off += k;
  }
  return wsum[NW];
}

// ONE block of kIfaceScanThreads threads: scan_counts, then the partials (fold_partials of kernels/reduce.h), and threads
// 0 .. IFS_N - 1 store one slot of the summary each.  The launch boundary in front of it is what makes the counts and partials of
// every block visible.
__global__ __launch_bounds__(kIfaceScanThreads) void k_iface_scan(int* __restrict__ cnt, long long n, const double* __restrict__ part, int nblocks,
                                                                   double* __restrict__ summary, double istep) {
  constexpr int NT = kIfaceScanThreads;
  __shared__ long long wsum[NT / 64 + 1];
  __shared__ double red[NT][kIfacePart];
  const int t = threadIdx.x;
  const double segments = (double)scan_counts<NT>(cnt, n, wsum);
  const double zero[kIfacePart] = {0.0, 0.0};
  fold_partials<NT, kIfacePart, 0>(part, nblocks, zero, red);
  if (t >= IFS_N) return;
  summary[t] = t == IFS_SEGMENTS ? segments : t == IFS_DEGENERATE ? red[0][1] : t == IFS_LENGTH ? red[0][0] : istep;
}

}  // namespace vof
