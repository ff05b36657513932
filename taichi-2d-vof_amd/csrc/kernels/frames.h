// kernels/frames.h -- a colour-mapped picture of one quantity: box averages over bx x by cells per pixel in a fixed order (k_frame_cols, k_frame_fold), the range, the colour table, the interface marked on top and the summary (k_frame_paint)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_frame, vof_step_frames).  A whole domain; every
// operand is converted to double on load (one code path for both dtypes); every product, sum, difference, quotient and root
// below is rounded on its own: every product goes through mul_rounded (kernels/cells.h), whose result no contraction reaches, so the FMA build gives the same bytes.
// A NumPy restatement follows it term for term (tests/_frames_np.py).
//
//   the cell value q[i,j], i in [1, nx], j in [1, ny]
//     F, P, DYE   F[i,j], p[i,j], C[i,j], raw
//     U           uc(i,j) = (u[i,j] + u[i+1,j]) * 0.5
//     V           vc(i,j) = (v[i,j] + v[i,j+1]) * 0.5                        (face_mean of kernels/cells.h, the product rounded on its own)
//     SPEED       sqrt(uc * uc + vc * vc)
//     VORT        (vc(i+1,j) - vc(i-1,j)) * hx - (uc(i,j+1) - uc(i,j-1)) * hy     hx = 0.5 dxi, hy = 0.5 dyi, doubles of the host;
//                 vc(i+-1, j), uc(i, j+-1) are the expressions above at the neighbouring cell, a ghost cell at the walls
//   the mean of pixel (a, b): the cells i in [a bx + 1, min((a+1) bx, nx)], j in [b by + 1, min((b+1) by, ny)], cnt of them
//     1. k_frame_cols: for every column j  c = 0.0;  c += q[i,j] for i ascending over the pixel row: one partial per (a, j)
//     2. k_frame_fold: S = 0.0;  S += c_j for j ascending;  m = S / (double)cnt
//   A NaN cell makes exactly its own pixel NaN.  With the contour flag the same two steps give mF, the means of F (for quantity
//   F they are m itself).
//   the range   fixed: lo, hi as given.  Auto: lo the minimum, hi the maximum of the non-NaN means -- as integers: the order-preserving
//     key of a double (its bits with the sign bit flipped if it is clear, all bits flipped if it is set: -0.0 sorts below +0.0), one
//     64-bit integer atomicMax of the key and one of its complement per wave, on words zeroed in front of the pass; no pixel: lo = hi = 0.
//     Auto and symmetric: A = max(|lo|, |hi|), lo = -A, hi = A.
//   the colour  t = (m - lo) / (hi - lo);  idx = 0 if hi == lo or not t > 0 (a NaN t, inf / inf, counts as that);  255 if t >= 1;
//     (int)(t * 255.0 + 0.5) otherwise;  the pixel is lut[idx]
//   the contour s(a,b) = mF(a,b) >= 0.5 (a NaN: false); lut[256] if s(a,b) != s(a+1,b) with a + 1 < pw or s(a,b) != s(a,b+1) with b + 1 < ph
//   NaN         a pixel whose own mean is NaN takes lut[257], whatever else holds
// rgb: (ph, pw, 3) bytes, image row r is pixel row b = ph - 1 - r, image column c is a.  means: (pw, ph) doubles.
//
// k_frame_cols is the pass over the fields: lanes along j, a wave marches K whole pixel rows (frame_geom of runtime/rows.h),
// the next row's loads in flight under this row's additions, and stores its V column partials as one vector every bx rows
// (the columns of a pixel row padded to whole tiles: cpitch).  The j +- 1 neighbours of V, SPEED and VORT are the row loads
// of kernels/common.h (load_row: the lane's columns and the two beside them, cache hits but for the tile's edge lanes).  No LDS,
// no scratch, no floating-point atomics.  Traffic: every field the quantity reads once (u twice at chunk seams), the partials
// (1 / bx of a field in doubles) once each way.
#pragma once
#include "cells.h"

namespace vof {

// = VOF_FRAME_* of include/vof2d.h: the quantities, the flags, the slots of the summary
enum : int { FQ_F = 0, FQ_U, FQ_V, FQ_SPEED, FQ_P, FQ_VORT, FQ_DYE, FQ_N };
enum : int { FRF_CONTOUR = 1, FRF_SYMMETRIC = 2 };
enum : int { FRS_PW = 0, FRS_PH, FRS_ISTEP, FRS_LO, FRS_HI, FRS_NAN_PIXELS, FRS_CONTOUR_PIXELS, FRS_N = 8 };
// the 64-bit words of a pass, zeroed in front of it: the largest key, the largest complement of a key; NaN and contour pixels
// (two 32-bit counters in one word); the blocks of k_frame_paint that are done
enum : int { FRW_MAX = 0, FRW_MIN, FRW_COUNTS, FRW_DONE, FRW_N };
constexpr int kFrameLutRows = 258, kFrameLutContour = 256, kFrameLutNan = 257;

__device__ __forceinline__ unsigned long long frame_key(double x) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(x);
  return (b >> 63) ? ~b : b ^ 0x8000000000000000ull;
}
__device__ __forceinline__ double frame_unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? k ^ 0x8000000000000000ull : ~k));
}

// element k in [-1, V] of a row with its neighbours, as a double
template <typename T, int V>
__device__ __forceinline__ double fr_at(const Row<T, V>& w, int k) { return (double)(k < 0 ? w.l : (k >= V ? w.r : w.c[k])); }
// uc at column offset k from the u rows i and i + 1; vc at column offset q in [0, V) from the v row
template <typename T, int V>
__device__ __forceinline__ double fr_uc(const Row<T, V>& a, const Row<T, V>& b, int k) {
  return mul_rounded(fr_at<T, V>(a, k) + fr_at<T, V>(b, k), 0.5);
}
template <typename T, int V>
__device__ __forceinline__ double fr_vc(const Row<T, V>& a, int q) {
  return mul_rounded(fr_at<T, V>(a, q) + fr_at<T, V>(a, q + 1), 0.5);
}

// ------------------------------------------------------------------ the pass over the fields
// Q: FQ_F (the cell of `s`: F, p or the dye), FQ_U, FQ_V, FQ_SPEED, FQ_VORT.  CONTOUR: the column partials of F too, into colF.
// g: the whole domain (ilo = 1, ihi = nx); R = K bx rows a chunk.  colq, colF: (pw, cpitch) doubles, 16-byte aligned.
template <typename T, int V, int Q, bool CONTOUR>
__global__ __launch_bounds__(256) void k_frame_cols(Geom g, const T* __restrict__ s, const T* __restrict__ u, const T* __restrict__ v, const T* __restrict__ F,
                                                     int R, int bx, int cpitch, double hx, double hy, double* __restrict__ colq, double* __restrict__ colF) {
  constexpr bool NU = Q == FQ_U || Q == FQ_SPEED || Q == FQ_VORT, NV = Q == FQ_V || Q == FQ_SPEED, VORT = Q == FQ_VORT;
  static_assert(Q == FQ_F || NU || NV, "a quantity of the list");
  int j0, ra, rb;
  if (!cell_tile<V>(g, R, j0, ra, rb)) return;
  const size_t pitch = (size_t)g.pitch;
  size_t o = at(g, ra, j0);
  // the windows: x, f rows i of s, F; u0, u1 rows i, i + 1 of u; v0 row i of v (V, SPEED); v1 row i + 1 of v with vcm, vc0 = vc of rows i - 1, i (VORT)
  T x[V], f[V];
  Row<T, V> u0, u1, v0, v1;
  double vcm[V], vc0[V];
  if constexpr (Q == FQ_F) load_s<T, V>(x, s + o);
  if constexpr (CONTOUR) load_s<T, V>(f, F + o);
  if constexpr (NU) { load_row<T, V>(u0, u + o); load_row<T, V>(u1, u + o + pitch); }
  if constexpr (NV) load_row<T, V>(v0, v + o);
  if constexpr (VORT) {
    Row<T, V> vm;
    load_row<T, V>(vm, v + o - pitch);   // row ra - 1 >= 0
    load_row<T, V>(v0, v + o);
    load_row<T, V>(v1, v + o + pitch);
#pragma unroll
    for (int q = 0; q < V; ++q) { vcm[q] = fr_vc<T, V>(vm, q); vc0[q] = fr_vc<T, V>(v0, q); }
  }
  double c[V], cf[V];
#pragma unroll
  for (int q = 0; q < V; ++q) { c[q] = 0.0; cf[q] = 0.0; }
  int a = (ra - 1) / bx, left = bx;
  for (int i = ra; i <= rb; ++i) {
    // the rows of the next step, in flight under this one's additions: i + 1 of s, F, v; i + 2 of u and of VORT's v (the last
    // stored row, nx + 1, again where there is none: loaded, not used)
    const int i2 = i + 2 <= g.nx + 1 ? i + 2 : g.nx + 1;
    const size_t o2 = at(g, i2, j0);
    T xn[V], fn[V];
    Row<T, V> un, vn;
    if constexpr (Q == FQ_F) load_s<T, V>(xn, s + o + pitch);
    if constexpr (CONTOUR) load_s<T, V>(fn, F + o + pitch);
    if constexpr (NU) load_row<T, V>(un, u + o2);
    if constexpr (NV) load_row<T, V>(vn, v + o + pitch);
    if constexpr (VORT) load_row<T, V>(vn, v + o2);
    double vcp[V];
#pragma unroll
    for (int q = 0; q < V; ++q) {
      double val;
      if constexpr (Q == FQ_F) val = (double)x[q];
      else if constexpr (Q == FQ_U) val = fr_uc<T, V>(u0, u1, q);
      else if constexpr (Q == FQ_V) val = fr_vc<T, V>(v0, q);
      else if constexpr (Q == FQ_SPEED) {
        const double uc = fr_uc<T, V>(u0, u1, q), vc = fr_vc<T, V>(v0, q);
        val = __builtin_sqrt(mul_rounded(uc, uc) + mul_rounded(vc, vc));
      } else {
        vcp[q] = fr_vc<T, V>(v1, q);
        val = mul_rounded(vcp[q] - vcm[q], hx) - mul_rounded(fr_uc<T, V>(u0, u1, q + 1) - fr_uc<T, V>(u0, u1, q - 1), hy);
      }
      c[q] += val;
      if constexpr (CONTOUR) cf[q] += (double)f[q];
    }
    if (--left == 0 || i == rb) {   // (wave-uniform) the pixel row ends: its partials out as one vector per lane, padding columns included
      Pack<double, V> k;
#pragma unroll
      for (int q = 0; q < V; ++q) { k.v[q] = c[q]; c[q] = 0.0; }
      *reinterpret_cast<Pack<double, V>*>(colq + (size_t)a * cpitch + (j0 - 1)) = k;
      if constexpr (CONTOUR) {
#pragma unroll
        for (int q = 0; q < V; ++q) { k.v[q] = cf[q]; cf[q] = 0.0; }
        *reinterpret_cast<Pack<double, V>*>(colF + (size_t)a * cpitch + (j0 - 1)) = k;
      }
      ++a;
      left = bx;
    }
#pragma unroll
    for (int q = 0; q < V; ++q) {
      if constexpr (Q == FQ_F) x[q] = xn[q];
      if constexpr (CONTOUR) f[q] = fn[q];
      if constexpr (VORT) { vcm[q] = vc0[q]; vc0[q] = vcp[q]; }
    }
    if constexpr (NU) { u0 = u1; u1 = un; }
    if constexpr (NV) v0 = vn;
    if constexpr (VORT) v1 = vn;
    o += pitch;
  }
}

// ------------------------------------------------------------------ the partials -> the means, the keys of their extrema
// One lane per pixel, pixel = a ph + b (the layout of means), the blocks striding over the pixels (at most kFramePixelBlocks
// of them: a wave keeps the largest key of all its pixels and ends with at most one pair of atomics, none where the words
// already hold as much -- thousands of waves on two addresses would cost more than the sums).  S over the by partials of the
// pixel in ascending j, divided by the cells the pixel really has.  colF / mF: NULL where the contour is off or the quantity
// is F.  The launch boundary in front makes the partials visible.
__global__ __launch_bounds__(256) void k_frame_fold(const double* __restrict__ colq, const double* __restrict__ colF, int nx, int ny, int bx, int by, int pw, int ph,
                                                     int cpitch, double* __restrict__ means, double* __restrict__ mF, unsigned long long* words) {
  const long long total = (long long)pw * ph;
  unsigned long long kmax = 0ull, kmin = 0ull;
  for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
    const long long pix = base + threadIdx.x;
    if (pix >= total) continue;
    const int a = (int)(pix / ph), b = (int)(pix % ph);
    const int jl = b * by, jh = jl + by < ny ? jl + by : ny;              // columns jl + 1 .. jh
    const int il = a * bx, ih = il + bx < nx ? il + bx : nx;
    const double cnt = (double)((long long)(ih - il) * (jh - jl));
    const double* const pq = colq + (size_t)a * cpitch;
    double S = 0.0;
    for (int j = jl; j < jh; ++j) S += pq[j];
    const double m = S / cnt;
    means[pix] = m;
    if (m == m) {
      const unsigned long long k = frame_key(m);
      kmax = k > kmax ? k : kmax;
      kmin = ~k > kmin ? ~k : kmin;
    }
    if (colF) {
      const double* const pf = colF + (size_t)a * cpitch;
      double SF = 0.0;
      for (int j = jl; j < jh; ++j) SF += pf[j];
      mF[pix] = SF / cnt;
    }
  }
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) {
    const unsigned long long o1 = __shfl_down(kmax, sft, 64), o2 = __shfl_down(kmin, sft, 64);
    kmax = o1 > kmax ? o1 : kmax;
    kmin = o2 > kmin ? o2 : kmin;
  }
  if ((threadIdx.x & 63) == 0 && kmax) {   // (a wave without a non-NaN pixel has nothing to say; a word that is read too small costs an atomic, no more)
    volatile unsigned long long* const seen = words;
    if (kmax > seen[FRW_MAX]) atomicMax(words + FRW_MAX, kmax);
    if (kmin > seen[FRW_MIN]) atomicMax(words + FRW_MIN, kmin);
  }
}

// ------------------------------------------------------------------ the means -> the picture and the summary
// One lane per pixel in image order, p = r pw + c, the blocks striding over the pixels like those of k_frame_fold: three byte
// stores at 3 p.  auto_range: lo, hi from the words of k_frame_fold.  mF: NULL without the contour.  The block that finishes
// last (a ticket on FRW_DONE behind a fence) writes the summary.
__global__ __launch_bounds__(256) void k_frame_paint(const double* __restrict__ means, const double* __restrict__ mF, int pw, int ph, int flags, int auto_range,
                                                      double lo, double hi, const unsigned char* __restrict__ lut, unsigned long long* words,
                                                      unsigned char* __restrict__ rgb, double* __restrict__ summary, double istep) {
  if (auto_range) {
    const unsigned long long kmax = words[FRW_MAX], kmin = words[FRW_MIN];
    lo = kmax ? frame_unkey(~kmin) : 0.0;
    hi = kmax ? frame_unkey(kmax) : 0.0;
    if (flags & FRF_SYMMETRIC) {
      const double A = __builtin_fmax(__builtin_fabs(lo), __builtin_fabs(hi));
      lo = -A; hi = A;
    }
  }
  const long long total = (long long)pw * ph;
  unsigned long long nn = 0ull, nc = 0ull;   // NaN and contour pixels of this lane
  for (long long base = (long long)blockIdx.x * 256; base < total; base += (long long)gridDim.x * 256) {
    const long long p = base + threadIdx.x;
    if (p >= total) continue;
    const int r = (int)(p / pw), a = (int)(p % pw), b = ph - 1 - r;
    const size_t at_m = (size_t)a * ph + b;
    const double m = means[at_m];
    int idx;
    if (m != m) {
      ++nn;
      idx = kFrameLutNan;
    } else {
      const double t = (m - lo) / (hi - lo);
      if (hi == lo || !(t > 0.0)) idx = 0;
      else if (t >= 1.0) idx = 255;
      else idx = (int)(mul_rounded(t, 255.0) + 0.5);
      if (mF) {
        const bool s0 = mF[at_m] >= 0.5;
        if ((a + 1 < pw && s0 != (mF[at_m + ph] >= 0.5)) || (b + 1 < ph && s0 != (mF[at_m + 1] >= 0.5))) {
          ++nc;
          idx = kFrameLutContour;
        }
      }
    }
    rgb[3 * p] = lut[3 * idx];
    rgb[3 * p + 1] = lut[3 * idx + 1];
    rgb[3 * p + 2] = lut[3 * idx + 2];
  }
  // the counters: one integer atomic per wave with something to count (NaN pixels in the low half of the word, contour pixels in the high)
  unsigned long long both = nn | (nc << 32);
#pragma unroll
  for (int sft = 32; sft > 0; sft >>= 1) both += __shfl_down(both, sft, 64);
  if ((threadIdx.x & 63) == 0 && both) atomicAdd(words + FRW_COUNTS, both);
  __syncthreads();
  if (threadIdx.x != 0) return;
  __threadfence();
  if (atomicAdd(words + FRW_DONE, 1ull) + 1ull != (unsigned long long)gridDim.x) return;
  __threadfence();
  const unsigned long long counts = atomicAdd(words + FRW_COUNTS, 0ull);
  summary[FRS_PW] = (double)pw;
  summary[FRS_PH] = (double)ph;
  summary[FRS_ISTEP] = istep;
  summary[FRS_LO] = lo;
  summary[FRS_HI] = hi;
  summary[FRS_NAN_PIXELS] = (double)(counts & 0xffffffffull);
  summary[FRS_CONTOUR_PIXELS] = (double)(counts >> 32);
  summary[7] = 0.0;
}

}  // namespace vof
