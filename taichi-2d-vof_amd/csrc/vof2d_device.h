// vof2d_device.h -- shared host/device definitions for the gfx950 kernels.
//
// Data layout in HBM (DESIGN.md "layout"): every field is a pitched 2-D array
//   element (i, j)  ->  base[(i - row_lo) * pitch + col0 + j]
// with j (y) contiguous, exactly the reference's (nx+2, ny+2) row-major order
// (2dvof.py:53) plus padding: col0 makes interior column j = 1
// start on a 128-byte boundary and the pitch is a multiple of 128 bytes, so a
// wave's 16-byte-per-lane accesses are aligned and never straddle rows.
//
// Work decomposition: one 64-lane wave owns a tile of 64*V contiguous columns
// (V = 2 elements per lane, VecWidth below) and marches along
// i over a chunk of rows, keeping the i-1 / i / i+1 rows in registers so each
// element is fetched from HBM once.  j-1 / j+V neighbours come from L1 hits or
// cross-lane shuffles.  Waves never synchronise with each other (no LDS, no
// barriers), so a 256-thread block is just four independent adjacent tiles.
#pragma once
#include <stdint.h>

namespace vof {

// Elements per lane and row: 2 for both precisions, i.e. a wave tile is 128 columns.  (16 bytes per
// lane -- 4 floats, 256-column tiles -- halves the number of tiles, and with it the chunk length a
// residency round allows, so the lead-in rows of every chunk weigh twice as much: fp32 at 4096^2
// 601 us/step with V = 4, 443 us/step with V = 2; 2048^2 249 -> 174 us.  The same in the pair kernels
// alone -- the kernels keep their V parameter, the runtime never asked for 4 outside experiments:
// k_jacobi_pair / k_tm<float, 4> need 128 / 135-149 VGPRs and ran 4096^2 fp32 at 0.62 ms/step against
// 0.35 with V = 2; wider tiles for k_jacobi_tb<double> lost the same way.  tools/probes/README.md.)
template <typename T> struct VecWidth { static constexpr int V = 2; };

// ------------------------------------------------------------------ tile geometry
// A marching kernel's wave loads and computes a tile of 64*V columns and stores all of it but H columns on either
// side (the neighbouring tiles do): tiles advance by STRIDE = 64*V - 2*H columns, the first one starts at column
// 1 - H, and tiles(ny) of them cover j = 1 .. ny.  The kernel takes H and STRIDE, the launch wrapper its tile count,
// from the one definition of its family below.  (Plain C++: this part of the file also compiles without HIP.)
template <int V, int HALO>
struct TileGeom {
  static constexpr int W = 64 * V, H = HALO, STRIDE = W - 2 * H;
  static constexpr int tiles(int ny) { return (ny + STRIDE - 1) / STRIDE; }
};
// Columns on each side of a tile that k_momentum / the FCT y stage load and compute but do not store.  The stencils
// need 2 and 4; 8 makes the tile stride 112 columns = 7 cache lines of doubles, so every tile's stored segment starts
// and ends on a 128-byte line (on a 64-byte sector in fp32).  With strides of 124 / 120 columns two waves -- often on
// different CUs -- each write part of the line between their tiles: the compute-free skeletons of the two kernels
// (tools/probes/stream_pattern.hip) run 11 % / 7 % faster at 112.
struct TileHalo { static constexpr int momentum = 2, transport = 8; };
template <int V> using MomentumGeom = TileGeom<V, TileHalo::momentum>;     // k_momentum
template <int V> using TransportGeom = TileGeom<V, TileHalo::transport>;   // k_fct_y, k_transport
// k_tm: 4 (transport) + 3 (momentum) invalid columns per side of the fused march, rounded up to even
template <int V> using TmGeom = TileGeom<V, 8>;
// k_jacobi_tb: TS - 1 from the cross-lane exchange of sweeps 2 .. TS, plus 1 where the first sweep also takes its
// j-neighbours from adjacent lanes (SQ), rounded up to V
template <int V, int TS, bool SQ> using JacobiTbGeom = TileGeom<V, ((TS - 1 + (SQ ? 1 : 0) + V - 1) / V) * V>;
// k_jacobi_pair: TS per side and march (TS - 1 cross-lane sweeps + the first sweep's DPP neighbours), two marches
template <int V, int TS> using JacobiPairGeom = TileGeom<V, ((2 * TS + V - 1) / V) * V>;

static_assert(MomentumGeom<2>::STRIDE == 124 && TransportGeom<2>::STRIDE == 112 && TmGeom<2>::STRIDE == 112, "tile strides");
static_assert(JacobiTbGeom<2, 5, true>::STRIDE == 116 && JacobiTbGeom<2, 5, false>::STRIDE == 120, "tile strides");
static_assert(JacobiTbGeom<2, 2, true>::STRIDE == 124 && JacobiTbGeom<2, 2, false>::STRIDE == 124, "tile strides");
static_assert(JacobiPairGeom<2, 5>::STRIDE == 108, "tile strides");

}  // namespace vof

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

namespace vof {

struct Geom {
  int nx, ny;            // global interior cells
  int row_lo, row_hi;    // stored rows (global, inclusive)
  int ilo, ihi;          // computable interior rows: max(1,row_lo+1) .. min(nx,row_hi-1)
  int own_lo, own_hi;    // rows whose counters/residuals this handle reports
  int wall_lo, wall_hi;  // 1 if this strip holds the i = 0 / i = nx+1 ghost row
  int64_t pitch;         // elements per stored row
  int col0;              // column offset of j = 0
  int ntj;               // column tiles of 64*V columns covering j = 1 .. ny
};

// k_tm's zero maps (kernels/fused_tm.h): one 32-bit word per (interior row i, k_tm tile column tj) of F (src, read)
// and of its twin (dst, written), at [(i - 1) * stride + tj + 1], stride = tiles + 2 (the words of tiles -1 and `tiles` stay 0).
// 1: the columns tile tj stores in row i of that array hold the bit pattern of +0.0 in every cell; 0: unknown.  Both maps lie in one
// allocation, at byte offsets src and dst >= 4 * stride * 4 behind base (one buffer descriptor and one load per row in the march, whose
// lanes reach four rows back from a word).  Null base: no maps.
struct ZeroMaps {
  unsigned* base;
  int src, dst;
  int stride;
};

// Constants rounded once from Python-double folded values.
template <typename T>
struct Consts {
  T dt, dx, dy, dxi, dyi, dxi2, dyi2, rho_l, rho_g, nu_l, nu_g, sigma, gx, gy;
  T nrm_x, nrm_y, kap_x, kap_y, dxdy, dtdy, dtdx, cfl_x, cfl_y, half_dx, half_dy, sqrt2dx, tiny;
  T inv_dx, inv_dy, inv_dt, inv_dxdy;  // correctly rounded reciprocals (div_by_const)
  T dt_rho_l, dt_rho_g;                // dt / rho_l, dt / rho_g: update_uv's dt / r (2dvof.py:273) where both cells hold pure liquid / gas
  // set_init_F literals (2dvof.py:141-159), folded in double then rounded
  T ic1_x2, ic1_y2, ic_r, ic_cx, ic2_cy, ic3_cy, ic3_pool;
};

template <typename T, int V>
struct alignas(sizeof(T) * V) Pack {
  T v[V];
};

// ti.max / ti.min.  The oracle evaluates them as comparisons (a > b ? a : b); v_max_f64 / v_min_f64
// return the same VALUE for every non-NaN pair (only the sign of a +-0 tie can differ, which no
// later operation observes) at a third of the instructions of compare + 2x v_cndmask_b32.
template <typename T> __device__ __forceinline__ T vmax(T a, T b);
template <typename T> __device__ __forceinline__ T vmin(T a, T b);
template <> __device__ __forceinline__ double vmax<double>(double a, double b) { return __builtin_fmax(a, b); }
template <> __device__ __forceinline__ double vmin<double>(double a, double b) { return __builtin_fmin(a, b); }
template <> __device__ __forceinline__ float vmax<float>(float a, float b) { return __builtin_fmaxf(a, b); }
template <> __device__ __forceinline__ float vmin<float>(float a, float b) { return __builtin_fminf(a, b); }

// 2dvof.py:192-195  var(a, b, c) = a + b + c - max(a,b,c) - min(a,b,c), left to right
template <typename T> __device__ __forceinline__ T var3(T a, T b, T c) {
  return ((a + b) + c) - vmax(vmax(a, b), c) - vmin(vmin(a, b), c);
}

// 2dvof.py:201-203 for one cell: rho, nu from F
template <typename T> __device__ __forceinline__ T rho_of(const Consts<T>& c, T F) {
  T Fc = var3((T)0.0, (T)1.0, F);
  return c.rho_g * ((T)1 - Fc) + c.rho_l * Fc;
}
template <typename T> __device__ __forceinline__ T nu_of(const Consts<T>& c, T F) {
  T Fc = var3((T)0.0, (T)1.0, F);
  return c.nu_l * Fc + c.nu_g * ((T)1.0 - Fc);
}

template <typename T> __device__ __forceinline__ T dsqrt(T x);
template <> __device__ __forceinline__ double dsqrt<double>(double x) { return __builtin_sqrt(x); }
template <> __device__ __forceinline__ float dsqrt<float>(float x) { return __builtin_sqrtf(x); }
template <typename T> __device__ __forceinline__ T dabs(T x);
template <> __device__ __forceinline__ double dabs<double>(double x) { return __builtin_fabs(x); }
template <> __device__ __forceinline__ float dabs<float>(float x) { return __builtin_fabsf(x); }

}  // namespace vof
#endif  // __HIPCC__
