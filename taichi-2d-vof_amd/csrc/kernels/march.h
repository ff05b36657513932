// kernels/march.h -- what the marching kernels share: the overlapped tile's decode, the clamped row pointer, the Courant count, the store of a corrected u, v row, the reference's per-cell formulas used by more than one header
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// The arithmetic of a row has one source per pipeline (MomentumWindow::step, TransportWindow::step, FctXPipe::push, fct_y_row);
// this header is the code around it.  Everything here is inlined into its caller and results leave through references.  A call
// site is on a helper only where its kernel kept the instruction stream it had with the lines written out (or the same
// instructions in another order); the sites that did not are left as they were and name the helper they mirror
// (profiles/march_helpers_refactor.md has the list and the reasons).  IN forms: an interior pair of k_tm, whose rows and
// columns need no wall test.
#pragma once
#include "common.h"

namespace vof {

// ------------------------------------------------------------------ the overlapped tile (TG: the kernel's TileGeom of vof2d_device.h)
// The wave (or pair) index of a launch whose first `skip_blocks` blocks do something else (the planner block).  SGPR: rows are wave-uniform.
__device__ __forceinline__ int wave_index(int skip_blocks = 0) {
  return ((int)blockIdx.x - skip_blocks) * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
}
// Tile column tj covers columns c0 .. c0 + W - 1, of which the H on either side are loaded and computed but not stored.
template <typename TG>
__device__ __forceinline__ int tile_c0(int tj) { return 1 - TG::H + tj * TG::STRIDE; }
// A lane's first column j0 and the columns [jlo, jhi] the tile stores (IN: every one of them inside [1, ny]) ...
// ... for a march that is handed c0 (the pair kernels)
template <typename TG, int V, bool IN = false>
__device__ __forceinline__ void tile_columns(int c0, int lane, int ny, int& j0, int& jlo, int& jhi) {
  j0 = c0 + lane * V;
  jlo = IN ? c0 + TG::H : (c0 + TG::H > 1 ? c0 + TG::H : 1);
  jhi = IN ? c0 + TG::W - TG::H - 1 : (c0 + TG::W - TG::H - 1 < ny ? c0 + TG::W - TG::H - 1 : ny);
}
// ... from the index of a wave in a launch with `ntiles` tile columns, which also gives the row chunk ch.  Written out, not a
// call of the two above, and c0 stays inside: the compiler simplifies a helper before it inlines it, and what it makes of these
// lines depends on seeing c0's definition and all of its uses together (profiles/march_helpers_refactor.md).
template <typename TG, int V>
__device__ __forceinline__ void tile_decode(int index, int ntiles, int lane, int ny, int& tj, int& ch, int& j0, int& jlo, int& jhi) {
  tj = index % ntiles;
  ch = index / ntiles;
  const int c0 = 1 - TG::H + tj * TG::STRIDE;
  j0 = c0 + lane * V;
  jlo = c0 + TG::H > 1 ? c0 + TG::H : 1;
  jhi = c0 + TG::W - TG::H - 1 < ny ? c0 + TG::W - TG::H - 1 : ny;
}

// ------------------------------------------------------------------ the clamped row pointer
// column j0 of row r of a field; rows outside the stored rows read the nearest stored row (IN: r is a stored row)
template <bool IN = false, typename T>
__device__ __forceinline__ const T* row_ptr(const Geom& g, const T* base, int r, int j0) {
  const int rc = IN ? r : (r < g.row_lo ? g.row_lo : (r > g.row_hi ? g.row_hi : r));
  return base + at(g, rc, j0);
}

// ------------------------------------------------------------------ small loops
template <typename T, int V>
__device__ __forceinline__ void zero_fill(T (&row)[V]) {
#pragma unroll
  for (int q = 0; q < V; ++q) row[q] = (T)0;
}
// every lane of the wave holds an exact zero in all its V cells (wave-uniform)
template <typename T, int V>
__device__ __forceinline__ bool wave_all_zero(const T (&row)[V]) {
  bool rz = true;
#pragma unroll
  for (int q = 0; q < V; ++q) rz = rz && row[q] == (T)0;
  return __all(rz);
}
// the sum of a count over the wave, in lane 0
__device__ __forceinline__ unsigned int wave_sum(unsigned int n) {
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) n += __shfl_down(n, sft, 64);
  return n;
}

// ------------------------------------------------------------------ Courant count (the reference's prints, 2dvof.py:276-279, as a counter)
// One row: cells of columns [jlo, jhi] whose corrected u (on rows that have one: urow) or v (on j >= 2) moves more than the
// limit in a step.  Which rows count -- the chunk's own, the handle's owned -- is the caller's condition around the call.
template <bool IN = false, typename T, int V>
__device__ __forceinline__ void courant_count(const Consts<T>& c, const T (&ur)[V], const T (&vr)[V], bool urow, int j0, int jlo, int jhi,
                                              unsigned int& viol) {
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const int j = j0 + q;
    if (j >= jlo && j <= jhi) {
      if (urow && ur[q] * c.dt > c.cfl_x) viol++;
      if ((IN || j >= 2) && vr[q] * c.dt > c.cfl_y) viol++;
    }
  }
}
// ... and a wave's count into the handle's counter: one atomic per wave that counted anything
__device__ __forceinline__ void courant_publish(unsigned int viol, unsigned long long* __restrict__ courant) {
  if (__any(viol != 0)) {
    const unsigned int tot = wave_sum(viol);
    if ((threadIdx.x & 63) == 0) atomicAdd(courant, (unsigned long long)tot);
  }
}

// ------------------------------------------------------------------ store of a corrected u, v row
// Columns [jlo, jhi] of u and v to urow / vrow (the lane's pointers into row r of Uo, Vo), wall faces included (set_BC's zeros,
// :525): v's wall column ny + 1 goes with the tile that ends at ny, and behind the last row (`last`: r == nx) the zeros of
// u[nx + 1] (unext), which the x sweep reads before the u, v boundary kernel runs on a full domain.
template <typename T, int V>
__device__ __forceinline__ void store_uv_row(T* __restrict__ urow, T* __restrict__ vrow, T* __restrict__ unext, bool last, const T (&ur)[V],
                                             const T (&vr)[V], int j0, int jlo, int jhi, int ny) {
  store_s<T, V>(urow, ur, j0, jlo, jhi);
  store_s<T, V>(vrow, vr, j0, jlo, jhi == ny ? ny + 1 : jhi);
  if (last) {
    T zero[V];
    zero_fill(zero);
    store_c<T, V>(unext, zero, j0, jlo, jhi);
  }
}

// ------------------------------------------------------------------ the reference's formulas that more than one header states
// get_normal_young, loop 1 (2dvof.py:285-306), for one cell from its 3 x 3 neighbourhood of F (m / 0 / p: i-1 / i / i+1, then j)
template <typename T>
__device__ __forceinline__ void normals_cell(const Consts<T>& c, T Fmm, T Fm0, T Fmp, T F0m, T F00, T F0p, T Fpm,
                                             T Fp0, T Fpp, T& ox, T& oy) {
  const T cxn = c.nrm_x, cyn = c.nrm_y;
  T mx1 = cxn * (Fpp + Fp0 - F0p - F00);
  T my1 = cyn * (Fpp - Fp0 + F0p - F00);
  T mx2 = cxn * (Fp0 + Fpm - F00 - F0m);
  T my2 = cyn * (Fp0 - Fpm + F00 - F0m);
  T mx3 = cxn * (F00 + F0m - Fm0 - Fmm);
  T my3 = cyn * (F00 - F0m + Fm0 - Fmm);
  T mx4 = cxn * (F0p + F00 - Fmp - Fm0);
  T my4 = cyn * (F0p - F00 + Fmp - Fm0);
  T mxsum = (mx1 + mx2 + mx3 + mx4) / (T)4;
  T mysum = (my1 + my2 + my3 + my4) / (T)4;
  if (dabs<T>(mxsum) < c.tiny && dabs<T>(mysum) < c.tiny) {
    ox = mxsum;
    oy = mysum;
  } else {
    T magnitude = dsqrt<T>(mxsum * mxsum + mysum * mysum);
    ox = mxsum / magnitude;
    oy = mysum / magnitude;
  }
}
// update_uv (2dvof.py:269-280) for one cell and one component: the same expressions in the same order.  rho_c / rho_m: density
// of the cell and of its lower neighbour in the component's direction; pc / pm likewise for p.
template <typename T>
__device__ __forceinline__ T corrected_velocity(const Consts<T>& c, T star, T rho_c, T rho_m, T pc, T pm, T di) {
  const T r = (rho_c + rho_m) * (T)0.5;
  return star - c.dt / r * (pc - pm) * di;
}

}  // namespace vof
