// kernels/cell_rows.h -- one row per interface cell, in order: the count, scan and emit passes that vof_interface and vof_curvature share (k_cell_rows, k_cell_rows_scan; scan_counts)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions).  Nothing here belongs to one verb:
// a verb keeps its per-cell operations, their order and what a row adds to its reduced values (kernels/interface.h, kernels/curvature.h).
//
// Order of the rows: ascending (i, j), i first.  Three launches, no atomics:
//   k_cell_rows<EMIT = false>  a wave marches its 64 * V columns over its chunk of rows with the rows i - 1, i, i + 1 of F in
//                              registers (each row of F is loaded once per chunk, plus two lead-in rows), skips, wave-uniformly,
//                              a row of its tile without a mixed cell, and writes the number of rows of every (grid row, column
//                              tile) into cnt[(i - g.ilo) * ntj + tile]; the verb's reduced values go through the reduction of
//                              kernels/reduce.h into one partial per block
//   k_cell_rows_scan           one block: cnt -> exclusive offsets in place (thread t owns a run of consecutive entries; the
//                              runs' totals are scanned through LDS), and the summary
//   k_cell_rows<EMIT = true>   recomputes the cells and stores row k of a (grid row, tile) at row offset[(grid row, tile)] + k of
//                              the output, k being the row's rank within the wave in column order (ballot + mbcnt over the
//                              lanes' V cells); rows from `cap` on are not stored
// Order of the reduced values, fixed: a lane takes its cells row by row, column by column; from there the reduction of
// kernels/reduce.h, one partial of NS + NM doubles per block, folded by k_cell_rows_scan (one block of kScanThreads threads).
//
// A verb is a type with
//   ROW_N, SUM_N         doubles of a row (even) and of the summary
//   NS, NM               its reduced values: NS sums, then NM maxima
//   Consts               what its cell function reads; has eps and one_m_eps
//   cell<T>(c, g, F, fm, f0, fp, i, j, row)   the cell (i, j) from its 3 x 3 neighbourhood fm = row i - 1, f0 = row i, fp = row i + 1,
//                        each [j - 1, j, j + 1] (and whatever else it gathers from F): 0 not mixed, 1 degenerate, 2 a row (filled)
//   Tally                the lane's reduced values in the count pass: acc[NS + NM] as a new Tally holds them is also what the fold
//                        starts from; row(r) takes a row, degenerate() a degenerate cell, publish(part) ends in block_publish<NS, NM>.
//                        Counts stay integers until publish (one register each, the same values)
//   summary(t, total, red, istep)   slot t of the summary from the number of rows and the folded values
#pragma once
#include "cells.h"

namespace vof {

constexpr int kScanThreads = 1024;

// ------------------------------------------------------------------ the pass over F: count (+ the reduced values), or emit
// cnt: EMIT = false, written: rows per (grid row, tile); EMIT = true, read: the exclusive offsets k_cell_rows_scan left there.
// part: NS + NM doubles per block -- EMIT = false only.  rows: the output, `cap` rows of ROW_N doubles -- EMIT = true only.
template <typename Verb, typename T, int V, bool EMIT>
__global__ __launch_bounds__(256) void k_cell_rows(Geom g, const T* __restrict__ F, int R, typename Verb::Consts c, int* __restrict__ cnt,
                                                    double* __restrict__ part, double* __restrict__ rows, long long cap) {
  constexpr int N = Verb::ROW_N;
  int j0, ra, rb;
  const bool active = cell_tile<V>(g, R, j0, ra, rb);
  typename Verb::Tally tally;
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
      // which of the lane's cells are candidates (wave-uniform skip: most rows of most tiles hold no mixed cell)
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
        int before = 0;   // rows of this grid row in the lanes below this one
        int kind[V];
        double row[V][N];
#pragma unroll
        for (int q = 0; q < V; ++q) {
          kind[q] = 0;
          if (cand[q]) {
            const double fm[3] = {(double)left_of(wm, q), (double)wm.c[q], (double)right_of(wm, q)};
            const double f0[3] = {(double)left_of(w0, q), (double)w0.c[q], (double)right_of(w0, q)};
            const double fp[3] = {(double)left_of(wp, q), (double)wp.c[q], (double)right_of(wp, q)};
            kind[q] = Verb::template cell<T>(c, g, F, fm, f0, fp, i, j0 + q, row[q]);
          }
          const unsigned long long b = __builtin_amdgcn_ballot_w64(kind[q] == 2);
          before += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
          total += __builtin_popcountll(b);
        }
        int rank = before;   // of the lane's first row within the grid row's tile, in column order
#pragma unroll
        for (int q = 0; q < V; ++q) {
          if (kind[q] == 2) {
            if constexpr (EMIT) {
              const long long k = base + rank;
              if (k < cap) {
                Pack<double, 2>* dst = reinterpret_cast<Pack<double, 2>*>(rows + (size_t)k * N);
#pragma unroll
                for (int m = 0; m < N / 2; ++m) dst[m] = Pack<double, 2>{{row[q][2 * m], row[q][2 * m + 1]}};
              }
            } else {
              tally.row(row[q]);
            }
            ++rank;
          } else if (!EMIT && kind[q] == 1) {
            tally.degenerate();
          }
        }
      }
      if (!EMIT && lane == 0) cnt[(size_t)(i - g.ilo) * g.ntj + tile] = total;
      wm = w0;
      w0 = wp;
      o += pitch;
    }
  }
  if constexpr (!EMIT) tally.publish(part);
}

// ------------------------------------------------------------------ counts -> exclusive offsets, block partials -> summary
// Every thread of a ONE-block kernel of NT threads calls it.  Thread t owns the entries [t * run, (t + 1) * run) of cnt
// (run = ceil(n / threads)): it adds them up, the block scans the threads' totals (waves by __shfl_up, the NT / 64 wave totals by
// thread 0 through LDS), and the thread writes its entries' exclusive offsets back.  Returns the total of all entries to every
// thread.  wsum: NT / 64 + 1 words of LDS.
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

// ONE block of kScanThreads threads: scan_counts, then the partials (fold_partials of kernels/reduce.h), and threads
// 0 .. SUM_N - 1 store one slot of the summary each.  The launch boundary in front of it is what makes the counts and partials of
// every block visible.
template <typename Verb>
__global__ __launch_bounds__(kScanThreads) void k_cell_rows_scan(int* __restrict__ cnt, long long n, const double* __restrict__ part, int nblocks,
                                                                  double* __restrict__ summary, double istep) {
  constexpr int NT = kScanThreads;
  __shared__ long long wsum[NT / 64 + 1];
  __shared__ double red[NT][Verb::NS + Verb::NM];
  const int t = threadIdx.x;
  const double total = (double)scan_counts<NT>(cnt, n, wsum);
  const typename Verb::Tally init;
  fold_partials<NT, Verb::NS, Verb::NM>(part, nblocks, init.acc, red);
  if (t >= Verb::SUM_N) return;
  summary[t] = Verb::summary(t, total, red[0], istep);
}

}  // namespace vof
