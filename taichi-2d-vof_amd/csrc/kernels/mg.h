// kernels/mg.h -- geometric multigrid on the pressure equation (k_mg_smooth, k_mg_restrict, k_mg_prolong), and the stop rule of its coarsest-level solve
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (DESIGN.md "multigrid pressure solve").  The equation is the one of kernels/cg.h,
//   L p = b - c ap,   c = sum(b) / sum(ap),   L p = ae (pE - p) + aw (pW - p) + an (pN - p) + a_s (pS - p),
// whose coefficients (2dvof.py:258-262) are constants: dxi2 / dyi2, or zero at a wall.  Level l of the hierarchy is the same
// stencil on nx / 2^l x ny / 2^l cells with dxi2 / 4^l, dyi2 / 4^l (the launch wrapper passes them in Consts<T>), cell
// centred: coarse cell (I, J) covers the fine cells (2I - 1 .. 2I, 2J - 1 .. 2J).  Every level keeps a correction e and a
// right-hand side f in the fields' pitched layout (its own Geom) with zeros outside the interior; on the finest level e
// is p itself and f is b - c ap, formed on the fly from rhs and the device scalar CG_C (sc != nullptr).
//
// Expression order (tests/_mg_np.py restates it):
//   smoothing      e_new = e + w * (((f - c ap) - L e) / ap),  w = 0.8, L e as the four differences above in that order
//   restriction    f_coarse = 0.25 * ((r[2I-1][2J-1] + r[2I-1][2J]) + (r[2I][2J-1] + r[2I][2J])),  r = (f - c ap) - L e
//   prolongation   along j first:  lo = 0.75 * x[J] + 0.25 * x[J-1],  hi = 0.75 * x[J] + 0.25 * x[J+1]   (fine columns 2J-1, 2J)
//                  then along i:   e[2I-1] += 0.75 * row[I] + 0.25 * row[I-1],  e[2I] += 0.75 * row[I] + 0.25 * row[I+1]
//                  (together the bilinear weights 9/16, 3/16, 3/16, 1/16); beyond a wall the coarse value is repeated.
// No LDS, no atomics, no cross-lane traffic: a lane's j -+ 1 neighbours are two more loads of lines its neighbours load
// anyway (load_row, as k_jacobi and k_cg_residual).  Lanes whose first column lies right of the level's ny leave.
#pragma once
#include "cg.h"

namespace vof {

// device scalar next to those of kernels/cg.h: max|z| at the start of the coarsest-level solve
enum : int { MG_Z0 = CG_STOP + 1 };
static_assert(MG_Z0 < CG_NSCAL, "the scalars of a solve");

// r = (f - cc ap) - L e for V cells of row i: w / x the centre columns of rows i - 1 / i + 1
template <typename T, int V>
__device__ __forceinline__ void mg_residual_row(const Consts<T>& c, int i, int nx, T cc, const T (&an)[V], const T (&as_)[V],
                                                const T (&w)[V], const Row<T, V>& cur, const T (&x)[V], const T (&ff)[V],
                                                T (&r)[V], T (&apo)[V]) {
  const T ae = i != nx ? c.dxi2 : (T)0.0;
  const T aw = i != 1 ? c.dxi2 : (T)0.0;
#pragma unroll
  for (int q = 0; q < V; ++q) {
    const T pc = cur.c[q];
    const T ap = (T)-1.0 * (ae + aw + an[q] + as_[q]);
    const T Le = ae * (x[q] - pc) + aw * (w[q] - pc) + an[q] * (right_of(cur, q) - pc) + as_[q] * (left_of(cur, q) - pc);
    r[q] = (ff[q] - cc * ap) - Le;
    apo[q] = ap;
  }
}

// ------------------------------------------------------------------ one damped Jacobi sweep e -> en
// Rows of e march through registers as in k_cg_residual: 3 arrays per cell.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_mg_smooth(Geom g, Consts<T> c, const T* __restrict__ e, const T* __restrict__ f,
                                                    T* __restrict__ en, int R, const double* __restrict__ sc) {
  int j0, ra, rb;
  if (!wave_tile<V>(g, g.ilo, g.ihi, R, j0, ra, rb)) return;
  const int nx = g.nx, ny = g.ny;
  const T cc = sc ? (T)sc[CG_C] : (T)0.0;
  const T om = (T)0.8;
  T an[V], as_[V];
#pragma unroll
  for (int q = 0; q < V; ++q) {
    an[q] = (j0 + q) != ny ? c.dyi2 : (T)0.0;
    as_[q] = (j0 + q) != 1 ? c.dyi2 : (T)0.0;
  }
  const int64_t pitch = g.pitch;
  size_t o = at(g, ra, j0);
  T w[V];
  Row<T, V> cur, x;
  load_c<T, V>(w, e + o - pitch);
  load_row<T, V>(cur, e + o);
  for (int i = ra; i <= rb; ++i) {
    load_row<T, V>(x, e + o + pitch);
    T ff[V], r[V], ap[V], out[V];
    load_c<T, V>(ff, f + o);
    mg_residual_row<T, V>(c, i, nx, cc, an, as_, w, cur, x.c, ff, r, ap);
#pragma unroll
    for (int q = 0; q < V; ++q) out[q] = cur.c[q] + om * (r[q] / ap[q]);
    store_c<T, V>(en + o, out, j0, 1, ny);
#pragma unroll
    for (int q = 0; q < V; ++q) w[q] = cur.c[q];
    cur = x;
    o += pitch;
  }
}

// ------------------------------------------------------------------ f_coarse = mean of the four fine residuals, e_coarse = 0
// A wave works on a tile of the COARSE level (gc): a lane's V coarse columns are 2 V fine ones, a coarse row two fine rows.
// The fine residual lives in registers only: 2 fine arrays read, 2 coarse arrays written.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_mg_restrict(Geom gf, Geom gc, Consts<T> c /* of the fine level */, const T* __restrict__ e,
                                                      const T* __restrict__ f, T* __restrict__ fc, T* __restrict__ ec, int R,
                                                      const double* __restrict__ sc) {
  int j0, ra, rb;
  if (!wave_tile<V>(gc, gc.ilo, gc.ihi, R, j0, ra, rb)) return;
  constexpr int V2 = 2 * V;
  const int jf = 2 * j0 - 1;
  const int nx = gf.nx, ny = gf.ny;
  const T cc = sc ? (T)sc[CG_C] : (T)0.0;
  T an[V2], as_[V2];
#pragma unroll
  for (int q = 0; q < V2; ++q) {
    an[q] = (jf + q) != ny ? c.dyi2 : (T)0.0;
    as_[q] = (jf + q) != 1 ? c.dyi2 : (T)0.0;
  }
  const int64_t pitch = gf.pitch;
  size_t o = at(gf, 2 * ra - 1, jf), oc = at(gc, ra, j0);
  T w[V2];
  Row<T, V2> a, b, n;
  load_c<T, V2>(w, e + o - pitch);
  load_row<T, V2>(a, e + o);
  for (int ic = ra; ic <= rb; ++ic) {
    const int i = 2 * ic - 1;
    load_row<T, V2>(b, e + o + pitch);
    load_row<T, V2>(n, e + o + 2 * pitch);
    T fa[V2], fb[V2], r0[V2], r1[V2], ap[V2];
    load_c<T, V2>(fa, f + o);
    load_c<T, V2>(fb, f + o + pitch);
    mg_residual_row<T, V2>(c, i, nx, cc, an, as_, w, a, b.c, fa, r0, ap);
    mg_residual_row<T, V2>(c, i + 1, nx, cc, an, as_, a.c, b, n.c, fb, r1, ap);
    T out[V], zero[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      out[q] = (T)0.25 * ((r0[2 * q] + r0[2 * q + 1]) + (r1[2 * q] + r1[2 * q + 1]));
      zero[q] = (T)0.0;
    }
    store_c<T, V>(fc + oc, out, j0, 1, gc.ny);
    store_c<T, V>(ec + oc, zero, j0, 1, gc.ny);
#pragma unroll
    for (int q = 0; q < V2; ++q) w[q] = b.c[q];
    a = n;
    o += 2 * pitch;
    oc += gc.pitch;
  }
}

// ------------------------------------------------------------------ e_fine += bilinear(e_coarse)
// Coarse tiles again.  Three coarse rows, already interpolated along j, march through registers; each coarse row gives
// two fine rows, updated in place (a cell is read and written by the same lane): 1/4 array read, one read and written.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_mg_prolong(Geom gf, Geom gc, const T* __restrict__ ec, T* __restrict__ e, int R) {
  int j0, ra, rb;
  if (!wave_tile<V>(gc, gc.ilo, gc.ihi, R, j0, ra, rb)) return;
  constexpr int V2 = 2 * V;
  const int jf = 2 * j0 - 1;
  const int nxc = gc.nx, nyc = gc.ny;
  // row i of e_coarse (the nearest interior row beyond a wall) along j: fine columns 2 J - 1 (even slots) and 2 J (odd slots)
  auto jrow = [&](int i, T (&t)[V2]) {
    const int ii = i < 1 ? 1 : (i > nxc ? nxc : i);
    Row<T, V> x;
    load_row<T, V>(x, ec + at(gc, ii, j0));
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const T l = (j0 + q) == 1 ? x.c[q] : left_of(x, q);
      const T r = (j0 + q) >= nyc ? x.c[q] : right_of(x, q);
      t[2 * q] = (T)0.75 * x.c[q] + (T)0.25 * l;
      t[2 * q + 1] = (T)0.75 * x.c[q] + (T)0.25 * r;
    }
  };
  const int64_t pitch = gf.pitch;
  size_t o = at(gf, 2 * ra - 1, jf);
  T prev[V2], cur[V2], nxt[V2];
  jrow(ra - 1, prev);
  jrow(ra, cur);
  for (int ic = ra; ic <= rb; ++ic) {
    jrow(ic + 1, nxt);
    T ea[V2], eb[V2];
    load_c<T, V2>(ea, e + o);
    load_c<T, V2>(eb, e + o + pitch);
#pragma unroll
    for (int q = 0; q < V2; ++q) {
      ea[q] = ea[q] + ((T)0.75 * cur[q] + (T)0.25 * prev[q]);
      eb[q] = eb[q] + ((T)0.75 * cur[q] + (T)0.25 * nxt[q]);
    }
    store_c<T, V2>(e + o, ea, jf, 1, gf.ny);
    store_c<T, V2>(e + o + pitch, eb, jf, 1, gf.ny);
#pragma unroll
    for (int q = 0; q < V2; ++q) { prev[q] = cur[q]; cur[q] = nxt[q]; }
    o += 2 * pitch;
  }
}

// ------------------------------------------------------------------ the coarsest-level solve ends on a reduction of max|z|
// The conjugate-gradient kernels of kernels/cg.h run on the coarsest level's Geom; a captured cycle cannot ask the host
// when to stop, so one thread does: start = 1 records the starting max|z| (k_cg_finish has just formed it), later calls set
// the stop word once the recurrence's max|z| is down to `reduction` of it, and every later launch of the solve returns at
// once (kernels/cg.h).
__global__ void k_mg_coarse_stop(double* __restrict__ sc, int start, double reduction) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double z = sc[CG_MAXZ];
  if (start) {
    sc[MG_Z0] = z;
    if (!(z > 0.0)) sc[CG_STOP] = 1.0;
  } else if (z <= reduction * sc[MG_Z0]) {
    sc[CG_STOP] = 1.0;
  }
}

}  // namespace vof
