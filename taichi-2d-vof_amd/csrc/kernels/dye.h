// kernels/dye.h -- a marker field carried by the reference's FCT transport (k_dye), and its statistics (k_dye_stats, kDyeRow)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_dye_*).  The dye C is a second colour
// function in the layout of F, moved by solve_VOF_rudman (2dvof.py:312-318) + post_process_f (:452-455) with C in the
// place of F on the FINAL u, v of a step: the operator is transport.h's, cell function by cell function.
#pragma once
#include "march.h"
#include "transport.h"
#include "cells.h"

namespace vof {

// ------------------------------------------------------------------ k_dye: both FCT sweeps of the dye in one pass
// k_transport (transport.h) without its update_uv half: one march along i that reads C, u, v and writes the twin Cn
// (4 array passes; the two launches k_fct_x<CORR = false> + k_fct_y move 8 and write the intermediate dye to memory).
// The x sweep is FctXPipe -- the pipeline of k_fct_x --, the y sweep is fct_y_row -- the row function of k_fct_y -- as a
// per-row stage in front of the pipeline (YFIRST, even istep: y then x) or behind it (odd istep: x then y); the sweep
// that runs second carries post_process_f as the fused POST form.  Per-cell functions, operands and order are those
// of k_fct_x<CORR = false> and k_fct_y<CORR = false>:
//   * u and v come from memory as those kernels read them (rows clamped to the stored rows; set_BC's zeros on the
//     wall faces u[1], u[nx+1], v[:,1], v[:,ny+1] are there: the host settles the ghost cells first);
//   * zero-ghost semantics (S5): F~, rp, rm outside [ilo, ihi] x [1, ny] and the limiter of the first face read as 0;
//   * nothing between the sweeps touches the ghost cells (S6): rows outside [ilo, ihi] enter the x pipeline unswept
//     (YFIRST), and C' in the ghost columns (x first) only ever meets the zero wall velocity v[:,1] = v[:,ny+1] = 0 --
//     so does the twin's ghost column in the two-launch form: both products are the same +0;
// so Cn is what the two launches leave in the interior, bit for bit.  The data-dependent shortcuts are the two
// DESIGN 3.3 proves for F, inside FctXPipe::push and fct_y_row (all anti-diffusive fluxes of the wave zero) and the
// all-zero row segment (C == 0 on every lane of the wave's row: the y stage passes it through, the pipeline bypasses
// itself after seven such rows); the operator is the same, so the proofs carry over.  No Courant count: the
// velocities are the step's, counted there.
// Tiles and chunks: TransportGeom<V> (vof2d_device.h) and the chunk length of k_transport (L::transport_rows).
// No LDS, no scratch, no atomics.  The ghost ring of Cn is the host's next launch (k_set_bc<BC_F> on the dye pair).
template <typename T, int V, bool YFIRST>
__global__ __launch_bounds__(256) void k_dye(Geom g, Consts<T> c, const T* __restrict__ C, T* __restrict__ Cn, int nty,
                                              const T* __restrict__ u, const T* __restrict__ v, int R) {
  typedef TransportGeom<V> TG;
  static_assert(TG::H >= 4 && TG::H % V == 0, "the y sweep's +-3 dependency is resolved across lanes");
  const int ilo = g.ilo, ihi = g.ihi, ny = g.ny;
  int tj, ch, j0, jlo, jhi;
  tile_decode<TG, V>(wave_index(), nty, threadIdx.x & 63, ny, tj, ch, j0, jlo, jhi);
  const int ra = ilo + ch * R;
  if (ra > ihi) return;  // padding waves of the last block (wave-uniform)
  const int rb = ra + R - 1 < ihi ? ra + R - 1 : ihi;
  auto swept_row = [&](int r) { return r >= ilo && r <= ihi; };   // rows the y sweep produces; the others keep C
  FctXPipe<T, V> pipe;
  {  // the pipeline's first donor row: C[ra - 3], y-swept where the y sweep runs first and produces that row
    T f1[V];
    load_c<T, V>(f1, row_ptr(g, C, ra - 3, j0));
    if (YFIRST && swept_row(ra - 3)) {
      T fs[V];
      zero_fill(fs);   // (what k_fct_y stores for an all-zero segment)
      if (!wave_all_zero(f1)) {
        T v0[V];
        load_s<T, V>(v0, row_ptr(g, v, ra - 3, j0));
        fct_y_row<T, V, false>(c, j0, ny, f1, v0, fs);
      }
      pipe.init(fs);
    } else {
      pipe.init(f1);
    }
  }
  // YFIRST: v of the row that enters the pipeline; x first: v of the row that leaves it (the y sweep trails by 3 rows
  // and only touches the chunk's own rows).  One row of C, u and v is prefetched an iteration ahead.
  auto v_row = [&](int r) { return YFIRST ? r : r - 3; };
  auto v_wanted = [&](int r) { const int rv = v_row(r); return YFIRST ? swept_row(rv) : (rv >= ra && rv <= rb); };
  T Cnx[V], unx[V], vnx[V];
  load_c<T, V>(Cnx, row_ptr(g, C, ra - 2, j0));
  load_s<T, V>(unx, row_ptr(g, u, ra - 2, j0));
#pragma unroll
  for (int q = 0; q < V; ++q) vnx[q] = (T)0;   // (mirrors zero_fill of march.h)
  if (v_wanted(ra - 2)) load_s<T, V>(vnx, row_ptr(g, v, v_row(ra - 2), j0));
  for (int r = ra - 2; r <= rb + 3; ++r) {
    T Cr[V], ur[V], vr[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      Cr[q] = Cnx[q]; ur[q] = unx[q]; vr[q] = vnx[q];
    }
    if (r < rb + 3) {
      load_c<T, V>(Cnx, row_ptr(g, C, r + 1, j0));
      load_s<T, V>(unx, row_ptr(g, u, r + 1, j0));
      if (v_wanted(r + 1)) load_s<T, V>(vnx, row_ptr(g, v, v_row(r + 1), j0));
    }
    T out[V];
    const int io = r - 3;
    const bool zr = wave_all_zero(Cr);
    if (YFIRST) {
      T Cp[V];
      if (!swept_row(r) || zr) {
#pragma unroll
        for (int q = 0; q < V; ++q) Cp[q] = swept_row(r) ? (T)0 : Cr[q];   // (a swept all-zero segment: the zeros k_fct_y stores)
      } else {
        fct_y_row<T, V, false>(c, j0, ny, Cr, vr, Cp);
      }
      pipe.template push<true>(c, r, ilo, ihi, Cp, ur, out, zr);
    } else {
      T Cp[V];
      pipe.template push<false>(c, r, ilo, ihi, Cr, ur, Cp, zr);   // C'[r - 3]
      zero_fill(out);
      if (io >= ra && io <= rb && !wave_all_zero(Cp)) fct_y_row<T, V, true>(c, j0, ny, Cp, vr, out);
    }
    if (io >= ra && io <= rb) store_s<T, V>(Cn + at(g, io, j0), out, j0, jlo, jhi);
  }
}

// ------------------------------------------------------------------ k_dye_stats: one row of statistics of the dye
// slots of a row (= VOF_DYE_* of include/vof2d.h)
enum : int { DY_ISTEP = 0, DY_CELLS, DY_SUM_C, DY_SUM_CI, DY_SUM_CJ, DY_SUM_C2, DY_SUM_CF, DY_SUM_CU, DY_SUM_CV, DY_MIN_C, DY_MAX_C, DY_MAX_EXCESS, DY_N = 16 };
constexpr int kDyeSums = 7, kDyePart = 10;   // doubles per block in the partials buffer: seven sums, then three maxima (-C, C, C - F)
constexpr RowMap<kDyeSums, kDyePart - kDyeSums> kDyeRow = {DY_N, {{ROW_ISTEP, 0}, {ROW_CELLS, 0}, {ROW_VALUE, 0}, {ROW_VALUE, 1}, {ROW_VALUE, 2}, {ROW_VALUE, 3}, {ROW_VALUE, 4},
    {ROW_VALUE, 5}, {ROW_VALUE, 6}, {ROW_MINUS, 7}, {ROW_VALUE, 8}, {ROW_VALUE, 9}},
    {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -__builtin_huge_val(), -__builtin_huge_val(), -__builtin_huge_val()}};
static_assert(DY_CELLS == 1 && DY_SUM_C == 2 && DY_SUM_CV == 8 && DY_MIN_C == 9 && DY_MAX_C == 10 && DY_MAX_EXCESS == 11, "kDyeRow lists the slots in this order");

// One pass over C, F, u, v on the cells i in [g.ilo, g.ihi], j in [1, ny], the march of k_diag (reduced_rows of kernels/cells.h) with C as the extra field.  Every
// operand is converted to double first; then, per cell, in this order (tests/_dye_np.py restates it term for term):
//   c  = C[i,j]     f = F[i,j]       uw = u[i,j]    ue = u[i+1,j]    vs = v[i,j]    vn = v[i,j+1]
//   SUM_C  += c
//   SUM_CI += c * i                  (global integer index as a double)
//   SUM_CJ += c * j
//   SUM_C2 += c * c
//   Fc = fmin(fmax(f, 0), 1)         SUM_CF += c * Fc                                (the plain clamp of vof_diagnostics)
//   uc = (uw + ue) * 0.5             vc = (vs + vn) * 0.5                            (interp_velocity, 2dvof.py:492)
//   SUM_CU += c * uc                 SUM_CV += c * vc
//   MIN_C = -max(-c)                 MAX_C = max(c)                  MAX_EXCESS = max(c - f)
// A NaN operand of a maximum counts as +inf (diag_max of kernels/reduce.h: a NaN C reads MAX_C = +inf, MIN_C = -inf); the
// sums propagate it.  No contraction (-ffp-contract=off).
// Order of the sums, fixed: that of k_diag; seven sums and three maxima wide, folded by k_row_finish into the row kDyeRow describes.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_dye_stats(Geom g, const T* __restrict__ C, const T* __restrict__ F, const T* __restrict__ u,
                                                    const T* __restrict__ v, int R, double* __restrict__ part) {
  const double ninf = -__builtin_huge_val();
  double acc[kDyePart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, ninf, ninf, ninf};
  reduced_rows<kDyeSums, kDyePart - kDyeSums, true, T, V>(g, C, F, u, v, R, acc, part, [&](const Cell& c, double cd) {
    acc[0] += cd;
    acc[1] += cd * c.i;
    acc[2] += cd * c.j;
    acc[3] += cd * cd;
    acc[4] += cd * clamp01(c.f);
    acc[5] += cd * face_mean(c.w, c.e);
    acc[6] += cd * face_mean(c.s, c.n);
    acc[7] = diag_max(acc[7], -cd);
    acc[8] = diag_max(acc[8], cd);
    acc[9] = diag_max(acc[9], cd - c.f);
  });
}

}  // namespace vof
