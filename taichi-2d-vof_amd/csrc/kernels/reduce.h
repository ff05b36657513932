// kernels/reduce.h -- the fixed-order reduction of the solvers, the diagnostics and the interface: lane values -> one partial per block (block_publish), partials -> one block's LDS (fold_partials)
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions).
//
// A reduced value is a set of NS sums followed by NM maxima, all doubles.  The order, fixed, so that a result depends on
// the launch geometry alone (tests/_reduce_np.py restates it):
//   1. a lane accumulates its cells in double, in the order its kernel states;
//   2. lanes -> wave by __shfl_down with s = 32, 16, ... 1 (wave_fold): lane l takes l + s;
//   3. waves -> block through LDS: thread k folds value k of waves 0, 1, 2, 3 in that order, starting from wave 0's;
//   4. one partial of NS + NM doubles per block into a buffer indexed by block (block_publish);
//   5. ONE block of NT threads folds the buffer: thread t starts from the caller's `init` and takes partials t, t + NT, ...
//      in that order; then a tree over the threads, s = NT / 2 ... 1, thread t taking t + s (fold_partials).
// No floating-point atomics.  The launch boundary between 4 and 5 is what makes every block's partial visible.
// The maxima are plain __builtin_fmax: a kernel that wants "a NaN counts as +inf" accumulates with cg_amax / diag_max.
#pragma once
#include "common.h"

namespace vof {

// max with "a NaN counts as +inf" (norm_acc of kernels/jacobi.h): of |x|, and of signed values
__device__ __forceinline__ double cg_amax(double m, double x) {
  const double a = __builtin_fabs(x);
  return a != a ? __builtin_huge_val() : __builtin_fmax(m, a);
}
__device__ __forceinline__ double diag_max(double m, double x) { return x != x ? __builtin_huge_val() : __builtin_fmax(m, x); }

// w[0 .. NS) are added, w[NS .. NS + NM) are maxima: lane 0 ends with the wave's values
template <int NS, int NM>
__device__ __forceinline__ void wave_fold(double (&w)[NS + NM]) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
    for (int k = 0; k < NS; ++k) w[k] += __shfl_down(w[k], s, 64);
#pragma unroll
    for (int k = NS; k < NS + NM; ++k) w[k] = __builtin_fmax(w[k], __shfl_down(w[k], s, 64));
  }
}

// lane values -> one partial per block.  Every thread of a 256-thread block calls it.
template <int NS, int NM>
__device__ __forceinline__ void block_publish(const double (&a)[NS + NM], double* __restrict__ part) {
  constexpr int N = NS + NM;
  __shared__ double red[4][N];
  double w[N];
#pragma unroll
  for (int k = 0; k < N; ++k) w[k] = a[k];
  wave_fold<NS, NM>(w);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) red[wave][k] = w[k];
  }
  __syncthreads();
  if (threadIdx.x < N) {   // thread k folds value k of the four waves, in wave order
    const int k = threadIdx.x;
    double t = red[0][k];
    for (int n = 1; n < 4; ++n) t = k < NS ? t + red[n][k] : __builtin_fmax(t, red[n][k]);
    part[(size_t)blockIdx.x * N + k] = t;
  }
}

// block partials -> red[0][.], visible to every thread on return.  Every thread of a one-block kernel of NT threads calls
// it; red: NT rows of LDS.  init: what a launch without blocks reports (0 for a sum, the least value a maximum can take).
template <int NT, int NS, int NM>
__device__ __forceinline__ void fold_partials(const double* __restrict__ part, int nblocks, const double (&init)[NS + NM],
                                              double (*red)[NS + NM]) {
  constexpr int N = NS + NM;
  const int t = threadIdx.x;
  double a[N];
#pragma unroll
  for (int k = 0; k < N; ++k) a[k] = init[k];
  for (int b = t; b < nblocks; b += NT) {
    const double* o = part + (size_t)b * N;
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] += o[k];
#pragma unroll
    for (int k = NS; k < N; ++k) a[k] = __builtin_fmax(a[k], o[k]);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) red[t][k] = a[k];
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) {
    if (t < s) {
#pragma unroll
      for (int k = 0; k < NS; ++k) red[t][k] += red[t + s][k];
#pragma unroll
      for (int k = NS; k < N; ++k) red[t][k] = __builtin_fmax(red[t][k], red[t + s][k]);
    }
    __syncthreads();
  }
}

}  // namespace vof
