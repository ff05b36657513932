// kernels/cg.h -- preconditioned conjugate gradients on the pressure equation (k_cg_apply, k_cg_update, k_cg_residual), with their fixed-order reductions
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (DESIGN.md "conjugate-gradient pressure solve").  With the coefficients of
// 2dvof.py:258-262 -- ae, aw, an, a_s = dxi2 / dyi2 or zero at the walls, ap = -(ae + aw + an + a_s) -- and
//   L p = ae (pE - p) + aw (pW - p) + an (pN - p) + a_s (pS - p)          ( = ae pE + aw pW + an pN + a_s pS + ap p )
// the Jacobi sweep of :263 is p_new = p + (b - L p) / ap.  Its right-hand side b does not sum to zero, so the sweeps
// have no fixed point: what they tend to is the p for which one more sweep adds the same constant c = sum(b) / sum(ap)
// to every cell.  That p solves the compatible problem  L p = b - c ap,  and this file solves it by conjugate
// gradients on -L preconditioned with -ap (the diagonal):
//   r = (b - c ap) - L p,   z = r / ap      ("what a sweep would still change, beyond the drift")
//   s <- z + beta s,  q = L s,  alpha = dot(r, z) / dot(s, q),  p += alpha s,  r -= alpha q,  beta = dot(r, z)_new / dot(r, z)
// (both dot products are <= 0; only their quotients are used).
//
// Reductions are reproducible: every lane accumulates in double (both field types) and publishes through the fixed-order
// reduction of kernels/reduce.h (one sum, two maxima per block); k_cg_finish (one block) folds the partials and forms
// alpha / beta ON THE DEVICE -- the host reads nothing between iterations.  No floating-point atomics.  A zero or
// non-finite denominator sets the stop word instead of dividing; every later launch of the batch then returns at once
// and the host's check decides.
//
// tests/_solver_bits_np.py restates every kernel here operation for operation (and the scalar logic of k_cg_finish mode by
// mode); tests/test_solver_bits_gpu.py holds the kernels to it bit for bit.  tests/_cg_np.py restates the METHOD, from the
// textbook: the independent judge of what a solve converges to, not of these bits.
#pragma once
#include "cells.h"

namespace vof {

// device scalars of a solve (doubles)
enum : int { CG_SUMB = 0, CG_C, CG_RZ, CG_RZ_OLD, CG_SQ, CG_ALPHA, CG_BETA, CG_MAXZ, CG_MAXP, CG_STOP, CG_NSCAL = 16 };
// what k_cg_finish does with the sums it has formed
enum : int { CG_FIN_SUMB = 0, CG_FIN_RESID, CG_FIN_APPLY, CG_FIN_UPDATE };
constexpr int kCgPart = 3;   // doubles per block in the partials buffer: one sum, two maxima

// ------------------------------------------------------------------ the block partials -> scalars, alpha, beta
// ONE block of 256 threads folds the partials (fold_partials of kernels/reduce.h); thread 0 acts on the result.  The launch
// boundary in front of it is what makes the partials of every other block visible.
__global__ __launch_bounds__(256) void k_cg_finish(const double* __restrict__ part, int nblocks, double* __restrict__ sc,
                                                    int mode, double sum_ap, int restart) {
  __shared__ double red[256][kCgPart];
  const double zero[kCgPart] = {0.0, 0.0, 0.0};
  fold_partials<256, 1, 2>(part, nblocks, zero, red);
  if (threadIdx.x != 0) return;
  const double sum = red[0][0], m1 = red[0][1], m2 = red[0][2];
  if (mode == CG_FIN_SUMB) {          // c = sum(b) / sum(ap)
    sc[CG_SUMB] = sum;
    sc[CG_C] = sum / sum_ap;
  } else if (mode == CG_FIN_RESID) {  // the recomputed residual replaces the recurrence's; the direction s is kept
    const double old = sc[CG_RZ_OLD];
    double beta = 0.0;
    if (restart) sc[CG_STOP] = 0.0;
    else if (old != 0.0 && __builtin_isfinite(old) && __builtin_isfinite(sum)) beta = sum / old;
    if (!__builtin_isfinite(beta)) beta = 0.0;
    sc[CG_BETA] = beta;
    sc[CG_RZ] = sum; sc[CG_MAXZ] = m1; sc[CG_MAXP] = m2;
  } else if (mode == CG_FIN_APPLY) {  // alpha = dot(r, z) / dot(s, q)
    if (sc[CG_STOP] != 0.0) return;
    const double rz = sc[CG_RZ];
    double alpha = 0.0;
    if (sum != 0.0 && __builtin_isfinite(sum) && __builtin_isfinite(rz)) alpha = rz / sum;
    if (!__builtin_isfinite(alpha)) alpha = 0.0;
    if (alpha == 0.0) sc[CG_STOP] = 1.0;   // nothing to divide by (or nothing left to do): the check decides
    sc[CG_SQ] = sum; sc[CG_ALPHA] = alpha;
  } else {                            // CG_FIN_UPDATE: beta = dot(r, z)_new / dot(r, z)
    if (sc[CG_STOP] != 0.0) return;
    const double rz = sc[CG_RZ];
    double beta = 0.0;
    if (rz != 0.0 && __builtin_isfinite(sum)) beta = sum / rz;
    if (!__builtin_isfinite(sum) || !__builtin_isfinite(beta)) { beta = 0.0; sc[CG_STOP] = 1.0; }
    sc[CG_RZ_OLD] = rz; sc[CG_RZ] = sum; sc[CG_BETA] = beta; sc[CG_MAXZ] = m1; sc[CG_MAXP] = m2;
  }
}

// ------------------------------------------------------------------ sum(b) over the interior (once per solve)
template <typename T, int V>
__global__ __launch_bounds__(256) void k_cg_sum(Geom g, const T* __restrict__ b, int R, double* __restrict__ part) {
  int j0, ra, rb;
  const bool active = cell_tile<V>(g, R, j0, ra, rb);
  double acc[kCgPart] = {0.0, 0.0, 0.0};
  if (active) {
    size_t o = at(g, ra, j0);
    for (int i = ra; i <= rb; ++i) {
      T v[V];
      load_c<T, V>(v, b + o);
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (j0 + q <= g.ny) acc[0] += (double)v[q];
      o += g.pitch;
    }
  }
  block_publish<1, 2>(acc, part);
}

// ------------------------------------------------------------------ r = (b - c ap) - L p, recomputed from p
// Start of a solve and every check: the true residual (which also keeps the recurrence of k_cg_update from drifting),
// dot(r, z), max|z| and max|p| over the interior.  Rows of p march through registers as in k_jacobi: 3 arrays per cell.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_cg_residual(Geom g, Consts<T> c, const T* __restrict__ p, const T* __restrict__ b,
                                                      T* __restrict__ r, int R, const double* __restrict__ sc,
                                                      double* __restrict__ part) {
  int j0, ra, rb;
  const bool active = cell_tile<V>(g, R, j0, ra, rb);
  double acc[kCgPart] = {0.0, 0.0, 0.0};
  if (active) {
    const int nx = g.nx, ny = g.ny;
    const T cc = (T)sc[CG_C];
    T an[V], as_[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      an[q] = (j0 + q) != ny ? c.dyi2 : (T)0.0;
      as_[q] = (j0 + q) != 1 ? c.dyi2 : (T)0.0;
    }
    const int64_t pitch = g.pitch;
    size_t o = at(g, ra, j0);
    T w[V];
    Row<T, V> cur, e;
    load_c<T, V>(w, p + o - pitch);
    load_row<T, V>(cur, p + o);
    for (int i = ra; i <= rb; ++i) {
      load_row<T, V>(e, p + o + pitch);
      T bb[V], out[V];
      load_c<T, V>(bb, b + o);
      const T ae = i != nx ? c.dxi2 : (T)0.0;
      const T aw = i != 1 ? c.dxi2 : (T)0.0;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const T pc = cur.c[q];
        const T ap = (T)-1.0 * (ae + aw + an[q] + as_[q]);
        const T Lp = ae * (e.c[q] - pc) + aw * (w[q] - pc) + an[q] * (right_of(cur, q) - pc) + as_[q] * (left_of(cur, q) - pc);
        const T rr = (bb[q] - cc * ap) - Lp;
        out[q] = rr;
        if (j0 + q <= ny) {
          const T z = rr / ap;
          acc[0] += (double)rr * (double)z;
          acc[1] = cg_amax(acc[1], (double)z);
          acc[2] = cg_amax(acc[2], (double)pc);
        }
      }
      store_c<T, V>(r + o, out, j0, 1, ny);
#pragma unroll
      for (int q = 0; q < V; ++q) w[q] = cur.c[q];
      cur = e;
      o += pitch;
    }
  }
  block_publish<1, 2>(acc, part);
}

// ------------------------------------------------------------------ s <- z + beta s,  q = L s,  dot(s, q)
// Reads r and the old direction with a one-cell halo (the new direction of the rows above and below the chunk and of
// the columns beside the tile is formed here as well: z = r / ap in registers, ap from the position, never stored),
// writes the new direction into the OTHER direction array (a vertical neighbour may still be reading the old one) and
// q.  4 arrays per cell.  The lanes' j -+ 1 neighbours come by DPP; the tile's edge lanes load theirs.  Cells outside
// the interior hold r = s = 0 in every work array, so their direction is 0 and the walls need no special case beyond
// the zero coefficients.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_cg_apply(Geom g, Consts<T> c, const T* __restrict__ r, const T* __restrict__ s_in,
                                                   T* __restrict__ s_out, T* __restrict__ qo, int R,
                                                   const double* __restrict__ sc, double* __restrict__ part) {
  int j0, ra, rb;
  bool active = cell_tile<V>(g, R, j0, ra, rb);
  if (sc[CG_STOP] != 0.0) active = false;
  double acc[kCgPart] = {0.0, 0.0, 0.0};
  if (active) {
    const int nx = g.nx, ny = g.ny;
    const int lane = threadIdx.x & 63;
    const T beta = (T)sc[CG_BETA];
    T an[V], as_[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      an[q] = (j0 + q) != ny ? c.dyi2 : (T)0.0;
      as_[q] = (j0 + q) != 1 ? c.dyi2 : (T)0.0;
    }
    // the column beside the tile that this lane forms itself if it is an edge lane
    const int jx = lane == 0 ? j0 - 1 : j0 + V;
    const T anx = jx != ny ? c.dyi2 : (T)0.0, asx = jx != 1 ? c.dyi2 : (T)0.0;
    const int64_t pitch = g.pitch;
    auto direction = [&](int i, size_t o, Row<T, V>& d) {
      T rr[V], ss[V];
      load_c<T, V>(rr, r + o);
      load_c<T, V>(ss, s_in + o);
      const T ax = (i != nx ? c.dxi2 : (T)0.0) + (i != 1 ? c.dxi2 : (T)0.0);
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const T ap = (T)-1.0 * (ax + an[q] + as_[q]);
        d.c[q] = rr[q] / ap + beta * ss[q];
      }
      d.l = lane_up(d.c[V - 1]);
      d.r = lane_dn(d.c[0]);
      if (lane == 0 || lane == 63) {
        const size_t ox = lane == 0 ? o - 1 : o + V;
        const T x = r[ox] / ((T)-1.0 * (ax + anx + asx)) + beta * s_in[ox];
        if (lane == 0) d.l = x; else d.r = x;
      }
    };
    size_t o = at(g, ra, j0);
    Row<T, V> w, cur, e;
    direction(ra - 1, o - pitch, w);
    direction(ra, o, cur);
    for (int i = ra; i <= rb; ++i) {
      direction(i + 1, o + pitch, e);
      const T ae = i != nx ? c.dxi2 : (T)0.0;
      const T aw = i != 1 ? c.dxi2 : (T)0.0;
      T out[V];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const T sc_ = cur.c[q];
        out[q] = ae * (e.c[q] - sc_) + aw * (w.c[q] - sc_) + an[q] * (right_of(cur, q) - sc_) + as_[q] * (left_of(cur, q) - sc_);
        if (j0 + q <= ny) acc[0] += (double)sc_ * (double)out[q];
      }
      store_c<T, V>(s_out + o, cur.c, j0, 1, ny);
      store_c<T, V>(qo + o, out, j0, 1, ny);
      w = cur;
      cur = e;
      o += pitch;
    }
  }
  block_publish<1, 2>(acc, part);
}

// ------------------------------------------------------------------ p += alpha s,  r -= alpha q,  dot(r, z), max|z|, max|p|
// Pointwise, in place: 6 arrays per cell.
template <typename T, int V>
__global__ __launch_bounds__(256) void k_cg_update(Geom g, Consts<T> c, T* __restrict__ p, const T* __restrict__ s,
                                                    T* __restrict__ r, const T* __restrict__ qi, int R,
                                                    const double* __restrict__ sc, double* __restrict__ part) {
  int j0, ra, rb;
  bool active = cell_tile<V>(g, R, j0, ra, rb);
  if (sc[CG_STOP] != 0.0) active = false;
  double acc[kCgPart] = {0.0, 0.0, 0.0};
  if (active) {
    const int nx = g.nx, ny = g.ny;
    const T alpha = (T)sc[CG_ALPHA];
    T an[V], as_[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      an[q] = (j0 + q) != ny ? c.dyi2 : (T)0.0;
      as_[q] = (j0 + q) != 1 ? c.dyi2 : (T)0.0;
    }
    size_t o = at(g, ra, j0);
    for (int i = ra; i <= rb; ++i) {
      T pp[V], ss[V], rr[V], qq[V];
      load_c<T, V>(pp, p + o);
      load_c<T, V>(ss, s + o);
      load_c<T, V>(rr, r + o);
      load_c<T, V>(qq, qi + o);
      const T ax = (i != nx ? c.dxi2 : (T)0.0) + (i != 1 ? c.dxi2 : (T)0.0);
#pragma unroll
      for (int q = 0; q < V; ++q) {
        pp[q] = pp[q] + alpha * ss[q];
        rr[q] = rr[q] - alpha * qq[q];
        if (j0 + q <= ny) {
          const T z = rr[q] / ((T)-1.0 * (ax + an[q] + as_[q]));
          acc[0] += (double)rr[q] * (double)z;
          acc[1] = cg_amax(acc[1], (double)z);
          acc[2] = cg_amax(acc[2], (double)pp[q]);
        }
      }
      store_c<T, V>(p + o, pp, j0, 1, ny);
      store_c<T, V>(r + o, rr, j0, 1, ny);
      o += g.pitch;
    }
  }
  block_publish<1, 2>(acc, part);
}

}  // namespace vof
