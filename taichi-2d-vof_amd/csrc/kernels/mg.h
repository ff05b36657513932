// kernels/mg.h -- geometric multigrid on the pressure equation (k_mg_smooth, k_mg_restrict, k_mg_prolong), the stop rule of its
// coarsest-level solve, that solve as one workgroup (k_mg_coarse_block), and the per-step residual record of vof_step_mg (k_mg_step_record)
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
// Expression order (tests/_solver_bits_np.py restates it operation for operation and tests/test_solver_bits_gpu.py holds the
// kernels to it bit for bit; tests/_mg_np.py restates the METHOD from the textbook, not this order):
//   smoothing      e_new = e + w * (((f - c ap) - L e) / ap),  w = 0.8, L e as the four differences above in that order
//   restriction    f_coarse = 0.25 * ((r[2I-1][2J-1] + r[2I-1][2J]) + (r[2I][2J-1] + r[2I][2J])),  r = (f - c ap) - L e
//   prolongation   along j first:  lo = 0.75 * x[J] + 0.25 * x[J-1],  hi = 0.75 * x[J] + 0.25 * x[J+1]   (fine columns 2J-1, 2J)
//                  then along i:   e[2I-1] += 0.75 * row[I] + 0.25 * row[I-1],  e[2I] += 0.75 * row[I] + 0.25 * row[I+1]
//                  (together the bilinear weights 9/16, 3/16, 3/16, 1/16); beyond a wall the coarse value is repeated.
// No LDS, no atomics, no cross-lane traffic: a lane's j -+ 1 neighbours are two more loads of lines its neighbours load
// anyway (load_row, as k_jacobi and k_cg_residual).  Lanes whose first column lies right of the level's ny leave.
#pragma once
#include "cg.h"
#include "residual_rule.h"

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

// ------------------------------------------------------------------ the coarsest-level solve as ONE workgroup (knob "mg_coarse_block")
// What L<T>::mg_coarse_solve enqueues as 3 + 5 x cap launches -- L e = f - c' ap from the e it finds, diagonally preconditioned
// conjugate gradients until max|z| is down to `reduction` of its start or `cap` iterations -- for a level of at most
// kMgBlockCells cells counting its ghost ring.  e, r, s, q live in LDS for the whole solve (4 x 1024 x 8 bytes in fp64);
// cell (i, j) is element i (ny + 2) + j, its ghost ring stays 0 as in the level's arrays in memory.  A thread owns the
// interior cells t, t + 256, ... in every phase, so only s -- whose neighbours the stencil reads -- needs a barrier
// between its writer and its readers; the reductions carry the others.  Sums in double for both field types: a thread's
// cells in order, lanes -> wave by wave_fold of kernels/reduce.h, waves -> block through LDS in wave order, every thread adding the four
// wave values itself -- so alpha, beta and the stop decision are formed by every thread from the same bits and the
// control flow stays uniform.  A zero or non-finite denominator ends the solve instead of dividing (kernels/cg.h).
// Another order of sums than the launches': other bits, same solver -- hence a knob.
constexpr int kMgBlockCells = 1024;

__device__ __forceinline__ void mg_block_reduce(double& sum, double& mx, double (*red)[2]) {
  double w[2] = {sum, mx};
  wave_fold<1, 1>(w);   // (kernels/reduce.h)
  __syncthreads();   // (everybody is through reading the previous reduction)
  if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = w[0]; red[threadIdx.x >> 6][1] = w[1]; }
  __syncthreads();
  sum = red[0][0]; mx = red[0][1];
  for (int k = 1; k < 4; ++k) { sum += red[k][0]; mx = __builtin_fmax(mx, red[k][1]); }
}

// sc_c: the scalars holding the solve's own c (a one-level cycle: the level is the grid), nullptr below the grid, where
// c' = sum(f) / sum_ap of this level is formed first
template <typename T>
__global__ __launch_bounds__(256) void k_mg_coarse_block(Geom g, Consts<T> c, T* __restrict__ e, const T* __restrict__ f,
                                                          const double* __restrict__ sc_c, double sum_ap, int cap, double reduction) {
  __shared__ T le[kMgBlockCells], lr[kMgBlockCells], ls[kMgBlockCells], lq[kMgBlockCells];
  __shared__ double red[4][2];
  const int t = threadIdx.x, nx = g.nx, ny = g.ny, w = ny + 2, ncell = nx * ny;
  for (int k = t; k < (nx + 2) * w; k += 256) { ls[k] = (T)0.0; le[k] = (T)0.0; }
  __syncthreads();
  double sum = 0.0, mx = 0.0;
  for (int n = t; n < ncell; n += 256) {
    const int i = 1 + n / ny, j = 1 + n % ny;
    const T ff = f[at(g, i, j)];
    lq[i * w + j] = ff;   // (parked: q is not formed before the first iteration)
    le[i * w + j] = e[at(g, i, j)];
    sum += (double)ff;
  }
  double cc_d;
  if (sc_c) cc_d = sc_c[CG_C];
  else { mg_block_reduce(sum, mx, red); cc_d = sum / sum_ap; }
  const T cc = (T)cc_d;
  __syncthreads();   // e of the neighbours
  auto coef = [&](int i, int j, T& ae, T& aw, T& an, T& as_) {
    ae = i != nx ? c.dxi2 : (T)0.0; aw = i != 1 ? c.dxi2 : (T)0.0;
    an = j != ny ? c.dyi2 : (T)0.0; as_ = j != 1 ? c.dyi2 : (T)0.0;
  };
  // r = (f - c ap) - L e,  dot(r, z),  max|z|
  sum = 0.0; mx = 0.0;
  for (int n = t; n < ncell; n += 256) {
    const int i = 1 + n / ny, j = 1 + n % ny, k = i * w + j;
    T ae, aw, an, as_;
    coef(i, j, ae, aw, an, as_);
    const T ap = (T)-1.0 * (ae + aw + an + as_), pc = le[k];
    const T Le = ae * (le[k + w] - pc) + aw * (le[k - w] - pc) + an * (le[k + 1] - pc) + as_ * (le[k - 1] - pc);
    const T rr = (lq[k] - cc * ap) - Le, z = rr / ap;
    lr[k] = rr;
    sum += (double)rr * (double)z;
    mx = cg_amax(mx, (double)z);
  }
  mg_block_reduce(sum, mx, red);
  double rz = sum, beta = 0.0;
  const double z0 = mx;
  bool stop = !(z0 > 0.0);
  for (int it = 0; it < cap && !stop; ++it) {
    // s <- z + beta s
    const T bt = (T)beta;
    for (int n = t; n < ncell; n += 256) {
      const int i = 1 + n / ny, j = 1 + n % ny, k = i * w + j;
      T ae, aw, an, as_;
      coef(i, j, ae, aw, an, as_);
      ls[k] = lr[k] / ((T)-1.0 * (ae + aw + an + as_)) + bt * ls[k];
    }
    __syncthreads();
    // q = L s,  dot(s, q)
    sum = 0.0; mx = 0.0;
    for (int n = t; n < ncell; n += 256) {
      const int i = 1 + n / ny, j = 1 + n % ny, k = i * w + j;
      T ae, aw, an, as_;
      coef(i, j, ae, aw, an, as_);
      const T sc_ = ls[k];
      const T q = ae * (ls[k + w] - sc_) + aw * (ls[k - w] - sc_) + an * (ls[k + 1] - sc_) + as_ * (ls[k - 1] - sc_);
      lq[k] = q;
      sum += (double)sc_ * (double)q;
    }
    mg_block_reduce(sum, mx, red);
    double alpha = 0.0;
    if (sum != 0.0 && __builtin_isfinite(sum) && __builtin_isfinite(rz)) alpha = rz / sum;
    if (!__builtin_isfinite(alpha)) alpha = 0.0;
    if (alpha == 0.0) break;   // nothing to divide by (or nothing left to do)
    // e += alpha s,  r -= alpha q,  dot(r, z),  max|z|
    const T al = (T)alpha;
    sum = 0.0; mx = 0.0;
    for (int n = t; n < ncell; n += 256) {
      const int i = 1 + n / ny, j = 1 + n % ny, k = i * w + j;
      T ae, aw, an, as_;
      coef(i, j, ae, aw, an, as_);
      le[k] = le[k] + al * ls[k];
      const T rr = lr[k] - al * lq[k];
      lr[k] = rr;
      const T z = rr / ((T)-1.0 * (ae + aw + an + as_));
      sum += (double)rr * (double)z;
      mx = cg_amax(mx, (double)z);
    }
    mg_block_reduce(sum, mx, red);
    beta = 0.0;
    if (rz != 0.0 && __builtin_isfinite(sum)) beta = sum / rz;
    if (!__builtin_isfinite(sum) || !__builtin_isfinite(beta)) { beta = 0.0; stop = true; }
    rz = sum;
    if (mx <= reduction * z0) stop = true;
  }
  for (int n = t; n < ncell; n += 256) {
    const int i = 1 + n / ny, j = 1 + n % ny;
    e[at(g, i, j)] = le[i * w + j];
  }
}

// ------------------------------------------------------------------ the residual record of a vof_step_mg call
// One thread, behind k_cg_residual + k_cg_finish at the end of a step's cycles: the step's residual by the rule of
// vof_residual_value (kernels/residual_rule.h) into the handle's record -- last, worst, which recorded step the worst
// belongs to (1-based; the first one on a tie), steps recorded.  The stream is a straight line: no atomics.  The host
// zeroes the record at the start of a call and reads it once, at the end.
enum : int { MGR_LAST = 0, MGR_WORST, MGR_WORST_AT, MGR_COUNT, MGR_N };
__global__ void k_mg_step_record(const double* __restrict__ sc, double* __restrict__ rec, int criterion) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double r = residual_rule(sc[CG_MAXZ], sc[CG_MAXP], criterion);
  const double n = rec[MGR_COUNT] + 1.0;
  rec[MGR_LAST] = r;
  if (n == 1.0 || r > rec[MGR_WORST]) { rec[MGR_WORST] = r; rec[MGR_WORST_AT] = n; }
  rec[MGR_COUNT] = n;
}

}  // namespace vof
