// kernels/cells.h -- what the extension kernels share: the tile of the reported cells (cell_tile), the product no contraction reaches (mul_rounded), a cell's operands as doubles (Cell), the pass that ends in a reduced row (reduced_rows, k_row_finish)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions).  Nothing here belongs to one verb: a kernel
// keeps its own operations, their order and which of its products are rounded on their own -- its contract with its NumPy restatement.
#pragma once
#include "reduce.h"

namespace vof {

// ------------------------------------------------------------------ the tile
// wave -> (first column of the lane, rows [ra, rb]) of the cells i in [g.ilo, g.ihi], j in [1, ny], cut into column tiles of 64 * V and
// row chunks of R; false (wave-uniform) for a wave past the last chunk.  Unlike wave_tile no LANE leaves: lanes right of ny load in-row padding,
// contribute nothing and store nothing, so that the cross-lane moves and the block reduction of the caller always see 64 live lanes.
template <int V>
__device__ __forceinline__ bool cell_tile(const Geom& g, int R, int& j0, int& ra, int& rb) {
  const int wave = blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tj = wave % g.ntj, ch = wave / g.ntj;
  j0 = 1 + tj * 64 * V + (int)(threadIdx.x & 63) * V;
  ra = g.ilo + ch * R;
  rb = ra + R - 1 < g.ihi ? ra + R - 1 : g.ihi;
  return ra <= g.ihi;
}

// ------------------------------------------------------------------ the rounded product
// a * b rounded on its own in either build: the product passes through an empty asm statement, so the compiler cannot fuse it
// with the addition or subtraction that takes it (-ffp-contract=fast fuses in the backend, whatever a pragma in the source says;
// the parity build has nothing to fuse).  No instruction is emitted for it.
__device__ __forceinline__ double mul_rounded(double a, double b) {
  double p = a * b;
  asm("" : "+v"(p));
  return p;
}

// ------------------------------------------------------------------ the operands of a cell
// Every operand converted to double first: f = F[i,j], w = u[i,j], e = u[i+1,j], s = v[i,j], n = v[i,j+1]; i, j the global
// indices as doubles.  A kernel that does not read a member pays nothing for it.
struct Cell { double i, j, f, w, e, s, n; };
// column q of a lane that marches along i: uw, ue rows i, i + 1 of u, vr row i of v; di, j0 from a kernel that reads i, j
template <typename T, int V>
__device__ __forceinline__ Cell cell_at(int q, const T (&f)[V], const T (&uw)[V], const T (&ue)[V], const Row<T, V>& vr, double di = 0.0, int j0 = 0) {
  return {di, (double)(j0 + q), (double)f[q], (double)uw[q], (double)ue[q], (double)vr.c[q], (double)right_of(vr, q)};
}
// Fc = fmin(fmax(f, 0), 1): the order of 2dvof.py:202, a plain clamp (a NaN f gives 0: fmax returns its other operand)
__device__ __forceinline__ double clamp01(double f) { return __builtin_fmin(__builtin_fmax(f, 0.0), 1.0); }
// uc = face_mean(w, e), vc = face_mean(s, n) (interp_velocity, 2dvof.py:492); kernels/frames.h rounds the product on its own
__device__ __forceinline__ double face_mean(double a, double b) { return (a + b) * 0.5; }

// ------------------------------------------------------------------ a pass over the reported cells that ends in one partial per block
// F and v rows are loaded once, the u row i + 1 of one iteration is the row i of the next (3 array passes), one more field X in the layout of F
// where EXTRA (nullptr otherwise).  cell(c, x) accumulates one cell, x = X[i,j] as a double (0 without X), row by row, column by column.  acc: the
// lane's NS sums and NM maxima, started by the caller, which the cell lambda captures by reference (handed to it as an argument they are kept
// twice, as a vector and as scalars: k_dye_stats at 68 VGPRs against 62, 7 waves a SIMD against 8).  Every thread of the block calls it.
template <int NS, int NM, bool EXTRA, typename T, int V, typename Body>
__device__ __forceinline__ void reduced_rows(const Geom& g, const T* __restrict__ X, const T* __restrict__ F, const T* __restrict__ u,
                                             const T* __restrict__ v, int R, const double (&acc)[NS + NM], double* __restrict__ part, Body cell) {
  int j0, ra, rb;
  if (cell_tile<V>(g, R, j0, ra, rb)) {
    const int ny = g.ny;
    const int64_t pitch = g.pitch;
    size_t o = at(g, ra, j0);
    T uw[V];
    load_c<T, V>(uw, u + o);
    for (int i = ra; i <= rb; ++i) {
      T x[V], f[V], ue[V];
      Row<T, V> vr;
      if constexpr (EXTRA) load_s<T, V>(x, X + o);
      load_s<T, V>(f, F + o);
      load_c<T, V>(ue, u + o + pitch);
      load_row<T, V>(vr, v + o);
      const double di = (double)i;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        if (j0 + q <= ny) {
          if constexpr (EXTRA) cell(cell_at<T, V>(q, f, uw, ue, vr, di, j0), (double)x[q]);
          else cell(cell_at<T, V>(q, f, uw, ue, vr, di, j0), 0.0);
        }
      }
#pragma unroll
      for (int q = 0; q < V; ++q) uw[q] = ue[q];
      o += pitch;
    }
  }
  block_publish<NS, NM>(acc, part);
}

// ------------------------------------------------------------------ the block partials -> one row
// What slot t of a row is: nothing (0), the step, the count of the reported cells, reduced value k or its negative
enum : signed char { ROW_ZERO = 0, ROW_ISTEP, ROW_CELLS, ROW_VALUE, ROW_MINUS };
struct RowSlot { signed char what, k; };
// n <= 16 slots, and what a sum or a maximum starts from: what a launch without blocks reports (fold_partials of kernels/reduce.h)
template <int NS, int NM>
struct RowMap { int n; RowSlot slot[16]; double init[NS + NM]; };

// ONE block of 256 threads, the shape of k_cg_finish: fold_partials, then threads 0 .. map.n - 1 store one slot each of the
// row.  The launch boundary in front of it is what makes the partials of every other block visible.
template <int NS, int NM>
__global__ __launch_bounds__(256) void k_row_finish(const double* __restrict__ part, int nblocks, double* __restrict__ row, double istep, double cells,
                                                     RowMap<NS, NM> map) {
  __shared__ double red[256][NS + NM];
  const int t = threadIdx.x;
  fold_partials<256, NS, NM>(part, nblocks, map.init, red);
  if (t >= map.n) return;
  const RowSlot s = map.slot[t];
  double x = 0.0;
  if (s.what == ROW_ISTEP) x = istep;
  else if (s.what == ROW_CELLS) x = cells;
  else if (s.what == ROW_VALUE) x = red[0][s.k];
  else if (s.what == ROW_MINUS) x = -red[0][s.k];
  row[t] = x;
}

}  // namespace vof
