// kernels/regrid.h -- a state carried onto a finer or coarser grid (k_regrid_refine, k_regrid_coarsen, k_regrid_ring, k_regrid_sum, k_regrid_finish): F from the PLIC line of the cell, u, v along the face normal, p between the cell centres
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_regrid).  Two handles: src (nx_s x ny_s cells of type Ts)
// and dst (nx_d x ny_d of type Td) over the same Lx x Ly; rx, ry in [1, 16] the integer factors along i and j.  Every operand is
// converted to double on load, all arithmetic is in double, a result is rounded once, on store (a NumPy restatement follows the
// operators term for term, tests/_regrid_np.py).  `c ? x : y` is a select on exactly that comparison (a NaN takes the `y`
// branch); every product that feeds a sum or a difference is rounded on its own in either build (mul_rounded of kernels/cells.h).
//
// REFINEMENT (nx_d = rx nx_s, ny_d = ry ny_s).  Source cell (I, J), child (k, m), k in [0, rx), m in [0, ry), is the destination cell
// i = (I - 1) rx + 1 + k, j = (J - 1) ry + 1 + m.  With drx = (double)rx, dry = (double)ry:
//   u[i,j]   k == 0 ? u_s[I,J] : u_s[I,J] + ((double)k / drx) * (u_s[I+1,J] - u_s[I,J])            (linear along the face normal, constant
//   v[i,j]   m == 0 ? v_s[I,J] : v_s[I,J] + ((double)m / dry) * (v_s[I,J+1] - v_s[I,J])             across it: every child has its parent's divergence)
//   p[i,j]   si = ((double)k + 0.5) / drx - 0.5;   si < 0 ? (ib = I - 1, wa = si + 1) : (ib = I, wa = si)        (bilinear between the source
//            sj = ((double)m + 0.5) / dry - 0.5;   sj < 0 ? (jb = J - 1, wb = sj + 1) : (jb = J, wb = sj)        cell centres, ghost cells included;
//            lo = p_s[ib,jb] + wa * (p_s[ib+1,jb] - p_s[ib,jb])                                                  the order of the tracer sample,
//            hi = p_s[ib,jb+1] + wa * (p_s[ib+1,jb+1] - p_s[ib,jb+1]);    p = lo + wb * (hi - lo)                kernels/tracers.h)
//   F[i,j]   without PLIC, or where iface_line (kernels/interface.h) at the call's eps gives no line for (I, J) -- not mixed, degenerate,
//            a NaN --: F_s[I,J].  Otherwise, with a, b, alpha, flip_x, flip_y of that line:
//              k' = flip_x ? rx - 1 - k : k        m' = flip_y ? ry - 1 - m : m        a' = a / drx        b' = b / dry
//              al = (alpha - a * ((double)k' / drx)) - b * ((double)m' / dry)          s' = a' + b'
//              n1 = a' < b' ? a' : b'              n2 = a' < b' ? b' : a'              t = s' - al
//              F = al <= 0 ? 0 : al >= s' ? 1 : al < n1 ? (al * al) / ((2 * n1) * n2) : al <= n2 ? (al - n1 * 0.5) / n2
//                                                                                      : 1 - (t * t) / ((2 * n1) * n2)
//            (the area of the child's rectangle under the parent's line, over the rectangle's)
// COARSENING (nx_s = rx nx_d, ny_s = ry ny_d; rx = ry = 1: the copy, which keeps every bit a conversion keeps).  Destination cell
// (i, j), children (k, m) at the source cell io + k, jo + m, io = (i - 1) rx + 1, jo = (j - 1) ry + 1:
//   F[i,j], p[i,j]   the rx ry children, k ascending and m ascending inside it, / (double)(rx * ry)
//   u[i,j]           u_s[io, jo + m], m ascending, / dry                  (the fine faces on the coarse face: the coarse divergence
//   v[i,j]           v_s[io + k, jo], k ascending, / drx                   is the mean of the fine ones)
// A sum of n terms x[0 .. n) in that order is added up in pairs (PairSum): x[0] + x[1], x[2] + x[3], ... then the pairs' sums in
// pairs, and so on -- the blocks of 2^l terms that start at a multiple of 2^l; what is left where n is no power of two, one block
// per set bit of n, is folded from the smallest block up, (older block) + (what the newer ones gave).  One term is the term itself:
// no 0 is added.  So 2^l equal terms add up exactly, and coarsening what a refinement by powers of two made of u, v and (without
// PLIC) F gives the bits back; a running sum x[0] + x[1] + x[2] ... rounds at the third term.
// WRITTEN, either way: F, its twin, u, v, p on i in [1, nx_d], j in [1, ny_d]; k_regrid_ring stores +0 into row 0 of u and column 0
// of v, the cells no kernel reads and set_BC does not write; the host's next launch is k_set_bc<BC_ALL>, which forms every other
// ghost cell and the wall faces u[1,.], u[nx_d+1,.], v[.,1], v[.,ny_d+1].  After it every cell of the four dense arrays is a
// function of the source alone.
//
// The kernels are destination-centred: a wave marches its 64 * V columns of dst along i (cell_tile).  The source reads are gathers at
// column (j - 1) / ry + 1: a lane forms the columns, children and weights of its V cells once, in front of the march; refining, it
// keeps what the source rows I - 1, I, I + 1 give its cells -- the line, the parent's F, six values of p, two of u, two of v -- and
// reloads them only when I changes.  No LDS but the reduction's, no atomics.
// The summary: PLIC_CELLS and DEGENERATE are counted by the child (0, 0) of a source cell, as doubles (exact), through the reduction
// of kernels/reduce.h (one partial of kRegridPart doubles per block of k_regrid_refine).  F_SRC and F_DST: k_regrid_sum on the
// interior of either handle -- a lane adds (double)F of its cells row by row, column by column, from there the same reduction, one
// partial per block --, of the values stored.  k_regrid_finish (one block of 256 threads) folds the three lists.
#pragma once
#include "cells.h"
#include "interface.h"

namespace vof {

// slots of the summary (= VOF_REGRID_SUM_* of include/vof2d.h), the flag, the limit
enum : int { RGS_RX = 0, RGS_RY, RGS_DIR, RGS_PLIC_CELLS, RGS_DEGENERATE, RGS_F_SRC, RGS_F_DST, RGS_ISTEP, RGS_N = 8 };
enum : int { RGF_PLIC = 1 };
constexpr int kRegridMaxFactor = 16;
constexpr int kRegridPart = 2;   // doubles per block of k_regrid_refine in the partials buffer: the cells refined from a line, the degenerate cells
constexpr int kRegridOut = 4;    // what k_regrid_finish stores: PLIC_CELLS, DEGENERATE, F_SRC, F_DST

// the F of child (k, m) of a cell with the line l
__device__ __forceinline__ double regrid_child_F(const IfaceLine& l, int k, int m, int rx, int ry, double drx, double dry) {
  const int k1 = l.flip_x ? rx - 1 - k : k, m1 = l.flip_y ? ry - 1 - m : m;
  const double a1 = l.a / drx, b1 = l.b / dry;
  const double al = (l.alpha - mul_rounded(l.a, (double)k1 / drx)) - mul_rounded(l.b, (double)m1 / dry);
  const double s1 = a1 + b1;
  const double n1 = a1 < b1 ? a1 : b1, n2 = a1 < b1 ? b1 : a1;
  const double t = s1 - al;
  if (al <= 0.0) return 0.0;
  if (al >= s1) return 1.0;
  if (al < n1) return (al * al) / ((2.0 * n1) * n2);
  if (al <= n2) return (al - mul_rounded(n1, 0.5)) / n2;
  return 1.0 - (t * t) / ((2.0 * n1) * n2);
}
__device__ __forceinline__ double regrid_lerp(double x0, double x1, double w) { return x0 + mul_rounded(w, x1 - x0); }

// ------------------------------------------------------------------ refinement
// gd: dst's geometry with [ilo, ihi] = [1, nx_d]; gs: src's.  part: kRegridPart doubles per block.
template <typename Ts, typename Td, int V, bool PLIC>
__global__ __launch_bounds__(256) void k_regrid_refine(Geom gd, Geom gs, const Ts* __restrict__ Fs, const Ts* __restrict__ us, const Ts* __restrict__ vs,
                                                        const Ts* __restrict__ ps, Td* __restrict__ Fd, Td* __restrict__ Fd2, Td* __restrict__ ud,
                                                        Td* __restrict__ vd, Td* __restrict__ pd, int rx, int ry, int R, IfaceConsts c,
                                                        double* __restrict__ part) {
  int j0, ra, rb;
  const bool active = cell_tile<V>(gd, R, j0, ra, rb);
  double acc[kRegridPart] = {0.0, 0.0};
  if (active) {
    const int ny = gd.ny;
    const double drx = (double)rx, dry = (double)ry;
    // the lane's V cells: source column, child, the weights along j (a lane right of ny works on column ny and stores nothing)
    int J[V], m[V], jb[V];
    double wb[V], tv[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const int j = j0 + q <= ny ? j0 + q : ny;
      J[q] = (j - 1) / ry + 1;
      m[q] = (j - 1) - (J[q] - 1) * ry;
      const double sj = ((double)m[q] + 0.5) / dry - 0.5;
      jb[q] = sj < 0.0 ? J[q] - 1 : J[q];
      wb[q] = sj < 0.0 ? sj + 1.0 : sj;
      tv[q] = (double)m[q] / dry;
    }
    // what the source rows I - 1, I, I + 1 give the lane's cells
    int kind[V];
    IfaceLine line[V];
    double f[V], u0[V], u1[V], v0[V], v1[V], pm[V][2], p0[V][2], pp[V][2];
    int Icur = -1;
    size_t o = at(gd, ra, j0);
    for (int i = ra; i <= rb; ++i) {
      const int I = (i - 1) / rx + 1, k = (i - 1) - (I - 1) * rx;   // (wave-uniform)
      if (I != Icur) {
        Icur = I;
#pragma unroll
        for (int q = 0; q < V; ++q) {
          const size_t s0 = at(gs, I, J[q]), sm = s0 - (size_t)gs.pitch, sp = s0 + (size_t)gs.pitch;
          f[q] = (double)Fs[s0];
          kind[q] = 0;
          if constexpr (PLIC) {
            const double fm[3] = {(double)Fs[sm - 1], (double)Fs[sm], (double)Fs[sm + 1]};
            const double f0[3] = {(double)Fs[s0 - 1], f[q], (double)Fs[s0 + 1]};
            const double fp[3] = {(double)Fs[sp - 1], (double)Fs[sp], (double)Fs[sp + 1]};
            kind[q] = iface_line(c, fm, f0, fp, line[q]);
          }
          u0[q] = (double)us[s0]; u1[q] = (double)us[sp];
          v0[q] = (double)vs[s0]; v1[q] = (double)vs[s0 + 1];
          const size_t b0 = at(gs, I, jb[q]);
          pm[q][0] = (double)ps[b0 - (size_t)gs.pitch]; pm[q][1] = (double)ps[b0 - (size_t)gs.pitch + 1];
          p0[q][0] = (double)ps[b0]; p0[q][1] = (double)ps[b0 + 1];
          pp[q][0] = (double)ps[b0 + (size_t)gs.pitch]; pp[q][1] = (double)ps[b0 + (size_t)gs.pitch + 1];
        }
      }
      const double si = ((double)k + 0.5) / drx - 0.5;
      const bool below = si < 0.0;
      const double wa = below ? si + 1.0 : si, tu = (double)k / drx;
      Td oF[V], oU[V], oV[V], oP[V];
#pragma unroll
      for (int q = 0; q < V; ++q) {
        if (k == 0 && m[q] == 0 && j0 + q <= ny) {   // the child that counts its parent
          acc[0] += kind[q] == 2 ? 1.0 : 0.0;
          acc[1] += kind[q] == 1 ? 1.0 : 0.0;
        }
        double F = f[q];
        if constexpr (PLIC) {
          if (kind[q] == 2) F = regrid_child_F(line[q], k, m[q], rx, ry, drx, dry);
        }
        const double u = k == 0 ? u0[q] : regrid_lerp(u0[q], u1[q], tu);
        const double v = m[q] == 0 ? v0[q] : regrid_lerp(v0[q], v1[q], tv[q]);
        const double a00 = below ? pm[q][0] : p0[q][0], a10 = below ? p0[q][0] : pp[q][0];
        const double a01 = below ? pm[q][1] : p0[q][1], a11 = below ? p0[q][1] : pp[q][1];
        const double lo = regrid_lerp(a00, a10, wa), hi = regrid_lerp(a01, a11, wa);
        oF[q] = (Td)F; oU[q] = (Td)u; oV[q] = (Td)v; oP[q] = (Td)regrid_lerp(lo, hi, wb[q]);
      }
      store_c<Td, V>(Fd + o, oF, j0, 1, ny);
      store_c<Td, V>(Fd2 + o, oF, j0, 1, ny);
      store_c<Td, V>(ud + o, oU, j0, 1, ny);
      store_c<Td, V>(vd + o, oV, j0, 1, ny);
      store_c<Td, V>(pd + o, oP, j0, 1, ny);
      o += (size_t)gd.pitch;
    }
  }
  block_publish<kRegridPart, 0>(acc, part);
}

// ------------------------------------------------------------------ coarsening, and the copy (rx = ry = 1)
// The sum in pairs of terms that arrive one by one (at most 2^8 = kRegridMaxFactor^2 of them): s[l] holds the sum of a finished block of
// 2^l terms while bit l of the count is set -- a binary counter whose carries are the additions.  The level loops are unrolled and the
// count is wave-uniform: s stays in registers, the tests are scalar.
struct PairSum {
  static constexpr int kLevels = 9;
  double s[kLevels];
  // term number n (counted from 0)
  __device__ __forceinline__ void push(double x, int n) {
    double carry = x;
    bool placed = false;
#pragma unroll
    for (int l = 0; l < kLevels; ++l) {
      if (!placed) {
        if ((n >> l) & 1) carry = s[l] + carry;
        else { s[l] = carry; placed = true; }
      }
    }
  }
  // of the n >= 1 terms pushed
  __device__ __forceinline__ double total(int n) const {
    double r = 0.0;
    bool has = false;
#pragma unroll
    for (int l = 0; l < kLevels; ++l) {
      if ((n >> l) & 1) { r = has ? s[l] + r : s[l]; has = true; }
    }
    return r;
  }
};
static_assert(kRegridMaxFactor * kRegridMaxFactor < (1 << PairSum::kLevels), "PairSum holds the children of a cell");

template <typename Ts, typename Td, int V>
__global__ __launch_bounds__(256) void k_regrid_coarsen(Geom gd, Geom gs, const Ts* __restrict__ Fs, const Ts* __restrict__ us, const Ts* __restrict__ vs,
                                                         const Ts* __restrict__ ps, Td* __restrict__ Fd, Td* __restrict__ Fd2, Td* __restrict__ ud,
                                                         Td* __restrict__ vd, Td* __restrict__ pd, int rx, int ry, int R) {
  int j0, ra, rb;
  if (!cell_tile<V>(gd, R, j0, ra, rb)) return;
  const int ny = gd.ny;
  const double drx = (double)rx, dry = (double)ry, dn = (double)(rx * ry);
  int jo[V];
#pragma unroll
  for (int q = 0; q < V; ++q) jo[q] = ((j0 + q <= ny ? j0 + q : ny) - 1) * ry + 1;
  size_t o = at(gd, ra, j0);
  for (int i = ra; i <= rb; ++i) {
    const int io = (i - 1) * rx + 1;
    Td oF[V], oU[V], oV[V], oP[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const size_t s0 = at(gs, io, jo[q]);
      PairSum F, p, u, v;
      for (int k = 0; k < rx; ++k) {
        const size_t sk = s0 + (size_t)k * (size_t)gs.pitch;
        v.push((double)vs[sk], k);
        for (int m = 0; m < ry; ++m) {
          F.push((double)Fs[sk + m], k * ry + m);
          p.push((double)ps[sk + m], k * ry + m);
          if (k == 0) u.push((double)us[sk + m], m);
        }
      }
      oF[q] = (Td)(F.total(rx * ry) / dn); oP[q] = (Td)(p.total(rx * ry) / dn); oU[q] = (Td)(u.total(ry) / dry); oV[q] = (Td)(v.total(rx) / drx);
    }
    store_c<Td, V>(Fd + o, oF, j0, 1, ny);
    store_c<Td, V>(Fd2 + o, oF, j0, 1, ny);
    store_c<Td, V>(ud + o, oU, j0, 1, ny);
    store_c<Td, V>(vd + o, oV, j0, 1, ny);
    store_c<Td, V>(pd + o, oP, j0, 1, ny);
    o += (size_t)gd.pitch;
  }
}

// ------------------------------------------------------------------ the cells set_BC leaves alone
// one thread per column of row 0 of u and per row of column 0 of v (a whole domain: both are stored)
template <typename T>
__global__ __launch_bounds__(256) void k_regrid_ring(Geom g, T* __restrict__ u, T* __restrict__ v) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t <= g.ny + 1) u[at(g, 0, t)] = (T)0;
  if (t <= g.nx + 1) v[at(g, t, 0)] = (T)0;
}

// ------------------------------------------------------------------ the sum of F over the interior, one partial per block
template <typename T, int V>
__global__ __launch_bounds__(256) void k_regrid_sum(Geom g, const T* __restrict__ F, int R, double* __restrict__ part) {
  int j0, ra, rb;
  double acc[1] = {0.0};
  if (cell_tile<V>(g, R, j0, ra, rb)) {
    size_t o = at(g, ra, j0);
    for (int i = ra; i <= rb; ++i) {
      T f[V];
      load_c<T, V>(f, F + o);
#pragma unroll
      for (int q = 0; q < V; ++q)
        if (j0 + q <= g.ny) acc[0] += (double)f[q];
      o += (size_t)g.pitch;
    }
  }
  block_publish<1, 0>(acc, part);
}

// ONE block of 256 threads: the counts (ncnt blocks of kRegridPart), the sums of F over src (ns blocks) and dst (nd blocks) -> out[kRegridOut].
// The launch boundary in front of it is what makes the partials of every block visible.
__global__ __launch_bounds__(256) void k_regrid_finish(const double* __restrict__ cnt, int ncnt, const double* __restrict__ sum_s, int ns,
                                                        const double* __restrict__ sum_d, int nd, double* __restrict__ out) {
  __shared__ double red2[256][kRegridPart];
  __shared__ double red1[256][1];
  const double zero2[kRegridPart] = {0.0, 0.0}, zero1[1] = {0.0};
  fold_partials<256, kRegridPart, 0>(cnt, ncnt, zero2, red2);
  if (threadIdx.x < kRegridPart) out[threadIdx.x] = red2[0][threadIdx.x];
  fold_partials<256, 1, 0>(sum_s, ns, zero1, red1);
  if (threadIdx.x == 0) out[2] = red1[0][0];
  __syncthreads();
  fold_partials<256, 1, 0>(sum_d, nd, zero1, red1);
  if (threadIdx.x == 0) out[3] = red1[0][0];
}

}  // namespace vof
