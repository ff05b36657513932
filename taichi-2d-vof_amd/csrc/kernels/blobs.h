// kernels/blobs.h -- droplets and bubbles labelled and measured on the device (k_blob_init, k_blob_merge, k_blob_flatten, k_blob_number, k_blob_label, k_blob_stats, k_blob_summary, k_blob_plan, k_blob_sums, k_blob_rows)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_blobs).  The cells are i in [g.ilo, g.ihi]
// (the caller passes the handle's owned interior rows there), j in [1, ny]; the KEY of a cell is its rank in ascending
// (i, j) order, key = (i - g.ilo) * ny + (j - 1).  Every operand is converted to double first.  A cell is a member of
// the liquid if F >= threshold, of the gas if F < threshold (a NaN F of neither); a blob is a maximal set of members
// joined through shared faces; blobs are numbered in ascending order of their first (smallest-key) cell.
//
// LABELLING: union-find on the int32 array `parent` over the keys (non-members hold -1).
//   k_blob_init     parent[cell] = the key of the start of the cell's horizontal run inside its wave tile (one ballot and one
//                   shuffle per row: the nearest lane to the left that holds a non-member, and that lane's last non-member)
//   k_blob_merge    unite(cell, cell - ny) for the FIRST cell of every stretch in which rows i and i - 1 are both members
//                   (the other cells of the stretch hang on it through their runs), and unite(cell, cell - 1) where a run
//                   crosses the boundary between two column tiles
//   k_blob_flatten  a launch of its own: parent[cell] = root(cell); roots counted per (row, tile)
// Invariant: parent[x] <= x, and parents only ever decrease (the only writes of the merge are atomicMin), so a set's
// root -- the one cell with parent == key -- is its smallest key: the blob's first cell.  Every walk up a chain visits
// strictly smaller keys and ends; unite() repeats with a strictly smaller pair (max(a, b) decreases) each time its
// atomicMin finds that the larger root had already been given a parent, so every loop makes progress on its own: no
// locks, no spinning, no thread ever waits for another.
// Coherence: in the merge launch `parent` is read with relaxed agent-scope atomic loads only, and even a stale value
// would still name an ancestor in the same set (parents are only replaced by smaller members of the set or of the set
// united with it).  unite() stops on just two grounds: both walks ended in the same cell (then the two cells share an
// ancestor: one set), or the VALUE RETURNED by the agent-scope atomicMin shows that the target still was a root when it
// was linked.  Nothing is flattened in the merge launch; k_blob_flatten starts behind the launch boundary that makes
// every link visible, and its own stores replace a parent by the root, again an ancestor.
//
// NUMBERING: k_cell_rows_scan (kernels/cell_rows.h, one block) turns the root counts into exclusive offsets; a root's rank
// within its (row, tile) in column order (ballot + mbcnt) plus the offset is its blob index (k_blob_number, which also
// starts the blob's integer record); k_blob_label writes index[root(cell)] over parent: the labels.
// INTEGER RECORD per blob (kBlobRec ints: first key, cells, imin, imax, jmin, jmax) by 32-bit integer atomics, whose
// result does not depend on the order of arrival.  k_blob_label folds first: while the members a wave sees row after
// row all carry one label (the pool, the gas) it keeps one wave-uniform record and issues its atomics when the label
// changes or the chunk ends; only a row in which the wave sees two labels goes cell by cell.
//
// THE FIVE SUMS of blob b (no floating-point atomics), for the first min(BLOBS, cap_rows) blobs.  With f = F[i,j]:
//   Fc = fmin(fmax(f, 0), 1)      w = Fc (liquid) | 1 - Fc (gas)
//   uc = (u[i,j] + u[i+1,j]) * 0.5      vc = (v[i,j] + v[i,j+1]) * 0.5                      (clamp01, face_mean of kernels/cells.h)
//   SUM_W += w    SUM_WI += w * i    SUM_WJ += w * j    SUM_WU += w * uc    SUM_WV += w * vc    (i, j global indices as doubles)
// Order, fixed by the geometry and the blob's own box [imin, imax] x [jmin, jmax] alone:
//   1. the box is cut into row chunks of kBlobRows rows counted from imin and into the column tiles of the grid
//      (64 * V columns, tile t starts at j = 1 + t * 64 * V) that it touches; one wave per (chunk, tile), chunk-major;
//   2. a lane starts from 0 and adds the cells of ITS blob (label == b, every other cell is skipped, not added as 0 times
//      something) row by row, column by column;
//   3. lanes -> wave by wave_fold of kernels/reduce.h; one partial of kBlobSums doubles per wave (k_blob_sums);
//   4. one wave per blob folds the blob's partials: lane l starts from 0 and takes partials l, l + 64, ... in that
//      order, then wave_fold again (k_blob_rows, which also writes the row).
// Cost of the sum pass: the sum of the box areas (in waves: k_blob_plan, scanned by k_cell_rows_scan); a blob whose box is
// most of the domain is spread over (rows / kBlobRows) x tiles waves like any pass over the grid.
// No contraction (-ffp-contract=off): each term is the bits of the line above.
#pragma once
#include "cells.h"

namespace vof {

// slots of a row and of the summary (= VOF_BLOB_* of include/vof2d.h)
enum : int { BL_I0 = 0, BL_J0, BL_CELLS, BL_IMIN, BL_IMAX, BL_JMIN, BL_JMAX, BL_SUM_W, BL_SUM_WI, BL_SUM_WJ, BL_SUM_WU, BL_SUM_WV, BL_N = 16 };
enum : int { BLS_BLOBS = 0, BLS_MEMBER_CELLS, BLS_MAX_CELLS, BLS_ISTEP, BLS_N = 4 };
enum : int { BR_FIRST = 0, BR_CELLS, BR_IMIN, BR_IMAX, BR_JMIN, BR_JMAX, kBlobRec = 6 };   // the integer record of a blob
constexpr int kBlobSums = 5;
constexpr int kBlobRows = 32;           // rows of a chunk of the sum pass
constexpr int kBlobStatPer = 8;        // records per thread of k_blob_stats

__device__ __forceinline__ bool blob_member(double f, int phase, double thr) { return phase == 0 ? f >= thr : f < thr; }

__device__ __forceinline__ int blob_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// the end of the chain above x (parents decrease strictly until the root, parent == key)
__device__ __forceinline__ int blob_find(const int* parent, int x) {
  int y = blob_load(parent + x);
  while (y != x) {
    x = y;
    y = blob_load(parent + x);
  }
  return x;
}
__device__ __forceinline__ void blob_unite(int* parent, int a, int b) {
  for (;;) {
    a = blob_find(parent, a);
    b = blob_find(parent, b);
    if (a == b) return;
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(parent + a, b);   // (agent scope)
    if (old == a) return;                       // a still was a root: it hangs on b now
    a = old;                                    // a had a parent `old` < a, which the minimum may have replaced: unite that one with b
  }
}

// ------------------------------------------------------------------ parent = start of the horizontal run within the tile
template <typename T, int V>
__global__ __launch_bounds__(256) void k_blob_init(Geom g, const T* __restrict__ F, int R, int phase, double thr, int* __restrict__ parent) {
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb)) return;
  const int ny = g.ny, lane = threadIdx.x & 63;
  const int col0 = j0 - 1 - lane * V;   // (0-based column of the tile's first cell, wave-uniform)
  const unsigned long long below = lane ? ~0ull >> (64 - lane) : 0ull;
  size_t o = at(g, ra, j0);
  for (int i = ra; i <= rb; ++i) {
    T f[V];
    load_c<T, V>(f, F + o);
    bool m[V];
    int lastnm = -1;   // the lane's last non-member
#pragma unroll
    for (int q = 0; q < V; ++q) {
      m[q] = j0 + q <= ny && blob_member((double)f[q], phase, thr);
      if (!m[q]) lastnm = q;
    }
    const unsigned long long open = __builtin_amdgcn_ballot_w64(lastnm >= 0) & below;   // lanes to the left that break a run
    const int src = open ? 63 - __builtin_clzll(open) : lane;
    const int theirs = __shfl(lastnm, src, 64);
    int start = open ? src * V + theirs + 1 : 0;   // (tile-relative column) of the run that reaches this lane from the left
    const int rowkey = (i - g.ilo) * ny;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (!m[q]) start = lane * V + q + 1;
      if (j0 + q <= ny) parent[rowkey + j0 - 1 + q] = m[q] ? rowkey + col0 + start : -1;
    }
    o += g.pitch;
  }
}

// ------------------------------------------------------------------ runs -> sets
template <typename T, int V>
__global__ __launch_bounds__(256) void k_blob_merge(Geom g, const T* __restrict__ F, int R, int phase, double thr, int* __restrict__ parent) {
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb)) return;
  const int ny = g.ny, lane = threadIdx.x & 63;
  size_t o = at(g, ra, j0);
  bool up[V], upl[V];   // membership of (i - 1, j) and of (i - 1, j - 1)
#pragma unroll
  for (int q = 0; q < V; ++q) up[q] = upl[q] = false;
  if (ra > g.ilo) {
    Row<T, V> w;
    load_row<T, V>(w, F + o - g.pitch);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      up[q] = j0 + q <= ny && blob_member((double)w.c[q], phase, thr);
      upl[q] = j0 + q - 1 >= 1 && j0 + q - 1 <= ny && blob_member((double)left_of(w, q), phase, thr);
    }
  }
  for (int i = ra; i <= rb; ++i) {
    Row<T, V> w;
    load_row<T, V>(w, F + o);
    const int rowkey = (i - g.ilo) * ny;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const int j = j0 + q;
      const bool m = j <= ny && blob_member((double)w.c[q], phase, thr);
      const bool ml = j - 1 >= 1 && j - 1 <= ny && blob_member((double)left_of(w, q), phase, thr);
      const int key = rowkey + j - 1;
      if (m && up[q] && !(ml && upl[q])) blob_unite(parent, key, key - ny);
      if (m && ml && q == 0 && lane == 0) blob_unite(parent, key, key - 1);   // (the run crosses into this tile)
      up[q] = m;
      upl[q] = ml;
    }
    o += g.pitch;
  }
}

// ------------------------------------------------------------------ every cell -> its root; roots per (row, tile)
template <int V>
__global__ __launch_bounds__(256) void k_blob_flatten(Geom g, int R, int* __restrict__ parent, int* __restrict__ cnt) {
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb)) return;
  const int ny = g.ny, lane = threadIdx.x & 63;
  const int tile = (j0 - 1) / (64 * V);
  for (int i = ra; i <= rb; ++i) {
    const int rowkey = (i - g.ilo) * ny;
    int total = 0;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      bool root = false;
      if (j0 + q <= ny) {
        const int key = rowkey + j0 - 1 + q;
        const int p = blob_load(parent + key);
        if (p >= 0) {
          const int r = blob_find(parent, p);
          if (r != p) __hip_atomic_store(parent + key, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          root = r == key;
        }
      }
      total += __builtin_popcountll(__builtin_amdgcn_ballot_w64(root));
    }
    if (lane == 0) cnt[(size_t)(i - g.ilo) * g.ntj + tile] = total;
  }
}

// ------------------------------------------------------------------ roots -> blob indices, the start of the records
// cnt: the exclusive offsets k_cell_rows_scan left there.  index[key of a root] = its blob index.
template <int V>
__global__ __launch_bounds__(256) void k_blob_number(Geom g, int R, const int* __restrict__ parent, const int* __restrict__ cnt, int* __restrict__ index,
                                                      int* __restrict__ rec) {
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb)) return;
  const int ny = g.ny;
  const int tile = (j0 - 1) / (64 * V);
  for (int i = ra; i <= rb; ++i) {
    const int rowkey = (i - g.ilo) * ny;
    int k = cnt[(size_t)(i - g.ilo) * g.ntj + tile];
    bool root[V];
    int before = 0;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      root[q] = j0 + q <= ny && parent[rowkey + j0 - 1 + q] == rowkey + j0 - 1 + q;
      const unsigned long long b = __builtin_amdgcn_ballot_w64(root[q]);
      before += (int)__builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    }
    k += before;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if (root[q]) {
        const int key = rowkey + j0 - 1 + q;
        index[key] = k;
        int* r = rec + (size_t)k * kBlobRec;
        r[BR_FIRST] = key; r[BR_CELLS] = 0;
        r[BR_IMIN] = 0x7fffffff; r[BR_IMAX] = -1; r[BR_JMIN] = 0x7fffffff; r[BR_JMAX] = -1;
        ++k;
      }
    }
  }
}

__device__ __forceinline__ void blob_record(int* __restrict__ rec, int label, int cells, int i0, int i1, int jlo, int jhi) {
  int* r = rec + (size_t)label * kBlobRec;
  atomicAdd(r + BR_CELLS, cells);
  atomicMin(r + BR_IMIN, i0);
  atomicMax(r + BR_IMAX, i1);
  atomicMin(r + BR_JMIN, jlo);
  atomicMax(r + BR_JMAX, jhi);
}

// ------------------------------------------------------------------ roots -> labels (over parent), cells and extent of every blob
template <int V>
__global__ __launch_bounds__(256) void k_blob_label(Geom g, int R, int* __restrict__ parent, const int* __restrict__ index, int* __restrict__ rec) {
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb)) return;
  const int ny = g.ny, lane = threadIdx.x & 63;
  const int tj0 = j0 - lane * V;   // (the tile's first column, wave-uniform)
  int wl = -1, wc = 0, wi0 = 0, wi1 = 0, wj0 = 0, wj1 = 0;   // the wave's record while it sees one label
  for (int i = ra; i <= rb; ++i) {
    const int rowkey = (i - g.ilo) * ny;
    int lab[V];
    int mine = -1;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      lab[q] = -1;
      if (j0 + q <= ny) {
        const int key = rowkey + j0 - 1 + q;
        const int p = parent[key];
        if (p >= 0) lab[q] = index[p];
        parent[key] = lab[q];
      }
      if (mine < 0) mine = lab[q];
    }
    const unsigned long long have = __builtin_amdgcn_ballot_w64(mine >= 0);
    if (have == 0ull) continue;
    const int ref = __shfl(mine, __builtin_ctzll(have), 64);
    bool other = false;
#pragma unroll
    for (int q = 0; q < V; ++q) other = other || (lab[q] >= 0 && lab[q] != ref);
    if (__builtin_amdgcn_ballot_w64(other) == 0ull) {
      if (ref != wl) {
        if (wl >= 0 && lane == 0) blob_record(rec, wl, wc, wi0, wi1, wj0, wj1);
        wl = ref; wc = 0; wi0 = i; wj0 = 0x7fffffff; wj1 = -1;
      }
      wi1 = i;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const unsigned long long b = __builtin_amdgcn_ballot_w64(lab[q] >= 0);
        if (b) {
          wc += __builtin_popcountll(b);
          const int lo = tj0 + __builtin_ctzll(b) * V + q, hi = tj0 + (63 - __builtin_clzll(b)) * V + q;
          wj0 = lo < wj0 ? lo : wj0;
          wj1 = hi > wj1 ? hi : wj1;
        }
      }
    } else {
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (lab[q] >= 0) blob_record(rec, lab[q], 1, i, i, j0 + q, j0 + q);
    }
  }
  if (wl >= 0 && lane == 0) blob_record(rec, wl, wc, wi0, wi1, wj0, wj1);
}

// ------------------------------------------------------------------ the summary
// The largest blob and the number of member cells: a thread takes kBlobStatPer records, the wave folds them, lane 0 issues
// one atomicAdd and one atomicMax on the two ints of `stat` (zeroed before the launch; at most 2^31 - 1 cells: no overflow).
__global__ __launch_bounds__(256) void k_blob_stats(const int* __restrict__ rec, long long nblobs, int* __restrict__ stat) {
  const long long b0 = ((long long)blockIdx.x * 256 + threadIdx.x) * kBlobStatPer;
  int s = 0, m = 0;
  for (int k = 0; k < kBlobStatPer; ++k) {
    if (b0 + k < nblobs) {
      const int c = rec[(size_t)(b0 + k) * kBlobRec + BR_CELLS];
      s += c;
      m = c > m ? c : m;
    }
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    s += __shfl_down(s, d, 64);
    const int o = __shfl_down(m, d, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63) == 0 && s > 0) {
    atomicAdd(stat, s);
    atomicMax(stat + 1, m);
  }
}
__global__ __launch_bounds__(64) void k_blob_summary(const int* __restrict__ stat, long long nblobs, double* __restrict__ summary, double istep) {
  const int t = threadIdx.x;
  if (t >= BLS_N) return;
  summary[t] = t == BLS_BLOBS ? (double)nblobs : t == BLS_MEMBER_CELLS ? (double)stat[0] : t == BLS_MAX_CELLS ? (double)stat[1] : istep;
}

// the box of blob b in global indices, and the waves of its sum pass
struct BlobBox { int imin, imax, t0, ntiles, nchunks; };
template <int V>
__device__ __forceinline__ BlobBox blob_box(const int* __restrict__ rec, int b) {
  const int* r = rec + (size_t)b * kBlobRec;
  BlobBox x;
  x.imin = r[BR_IMIN]; x.imax = r[BR_IMAX];
  x.t0 = (r[BR_JMIN] - 1) / (64 * V);
  x.ntiles = (r[BR_JMAX] - 1) / (64 * V) - x.t0 + 1;
  x.nchunks = (x.imax - x.imin + kBlobRows) / kBlobRows;
  return x;
}
// waves[b] = the waves blob b takes in k_blob_sums, b < nsel; waves[nsel] = 0 (the scan leaves the total there)
template <int V>
__global__ __launch_bounds__(256) void k_blob_plan(const int* __restrict__ rec, int nsel, int* __restrict__ waves) {
  const int b = blockIdx.x * 256 + threadIdx.x;
  if (b > nsel) return;
  int n = 0;
  if (b < nsel) {
    const BlobBox x = blob_box<V>(rec, b);
    n = x.ntiles * x.nchunks;
  }
  waves[b] = n;
}

// ------------------------------------------------------------------ the five sums: one partial per (blob, chunk, tile)
// off: nsel + 1 exclusive offsets of the blobs' waves (off[nsel] = total).  labels: the array k_blob_label left.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_blob_sums(Geom g, const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v,
                                                    const int* __restrict__ labels, const int* __restrict__ rec, const int* __restrict__ off, int nsel,
                                                    int phase, double* __restrict__ part) {
  const long long wave = (long long)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave >= (long long)off[nsel]) return;   // (wave-uniform; nothing below synchronises the block)
  int lo = 0, hi = nsel - 1;   // the blob: the last b with off[b] <= wave (every blob has at least one wave)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((long long)off[mid] <= wave) lo = mid; else hi = mid - 1;
  }
  const int b = lo;
  const BlobBox x = blob_box<V>(rec, b);
  const int local = (int)(wave - off[b]);
  const int ch = local / x.ntiles, tile = x.t0 + local % x.ntiles;
  const int lane = threadIdx.x & 63, ny = g.ny;
  const int j0 = 1 + tile * 64 * V + lane * V;
  const int ra = x.imin + ch * kBlobRows, rb = ra + kBlobRows - 1 < x.imax ? ra + kBlobRows - 1 : x.imax;
  double acc[kBlobSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = ra; i <= rb; ++i) {
    const int rowkey = (i - g.ilo) * ny;
    const double di = (double)i;
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const int j = j0 + q;
      if (j <= ny && labels[rowkey + j - 1] == b) {
        const size_t o = at(g, i, j);
        const Cell c = {di, (double)j, (double)F[o], (double)u[o], (double)u[o + g.pitch], (double)v[o], (double)v[o + 1]};
        const double Fc = clamp01(c.f);
        const double w = phase == 0 ? Fc : 1.0 - Fc;
        const double uc = face_mean(c.w, c.e), vc = face_mean(c.s, c.n);
        acc[0] += w;
        acc[1] += w * c.i;
        acc[2] += w * c.j;
        acc[3] += w * uc;
        acc[4] += w * vc;
      }
    }
  }
  wave_fold<kBlobSums, 0>(acc);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kBlobSums; ++k) part[(size_t)wave * kBlobSums + k] = acc[k];
  }
}

// ------------------------------------------------------------------ a blob's partials -> its row
// One wave per blob.  ilo: the first owned row (key -> global indices).
__global__ __launch_bounds__(256) void k_blob_rows(const int* __restrict__ rec, const int* __restrict__ off, int nsel, const double* __restrict__ part,
                                                    int ilo, int ny, double* __restrict__ rows) {
  const int b = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (b >= nsel) return;
  const int lane = threadIdx.x & 63;
  const int p0 = off[b], n = off[b + 1] - p0;
  double acc[kBlobSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = lane; k < n; k += 64) {
    const double* o = part + (size_t)(p0 + k) * kBlobSums;
#pragma unroll
    for (int s = 0; s < kBlobSums; ++s) acc[s] += o[s];
  }
  wave_fold<kBlobSums, 0>(acc);
  const int* r = rec + (size_t)b * kBlobRec;
  if (lane < BL_N && (lane < BL_SUM_W || lane > BL_SUM_WV)) {
    double x = 0.0;   // (unused slots read 0)
    if (lane == BL_I0) x = (double)(ilo + r[BR_FIRST] / ny);
    else if (lane == BL_J0) x = (double)(1 + r[BR_FIRST] % ny);
    else if (lane >= BL_CELLS && lane <= BL_JMAX) x = (double)r[BR_CELLS + (lane - BL_CELLS)];
    rows[(size_t)b * BL_N + lane] = x;
  }
  if (lane == 0) {
#pragma unroll
    for (int s = 0; s < kBlobSums; ++s) rows[(size_t)b * BL_N + BL_SUM_W + s] = acc[s];
  }
}

}  // namespace vof
