// kernels/energy.h -- the energy budget of the flow reduced on the device (k_energy, kEnergyRow): kinetic energy on the faces, the moments of the density, the interface measure, and the power of every term of the momentum predictor
//
// Part of the gfx950 kernel set of the 2-D VOF hot path (see vof2d_kernels.h for the conventions:
// reference line citations, expression order, one wave = 64*V columns marching along i).
//
// Extension, not part of the reference (include/vof2d.h, vof_energy).  Whole-domain handles only.  One pass over F, u, v, p on
// the cells i in [1, nx], j in [1, ny].  Every operand is converted to double first, the constants are the doubles of vof_get_param; then, in
// this order (a NumPy restatement follows it term for term, tests/_energy_np.py).  Every sum is left to right, `c ? x : y` is a select on
// exactly that comparison (a NaN takes `y`).
// A cell (a, b), from the stored F (ghost cells included):
//   Fc = fmin(fmax(F[a,b], 0), 1)       rho = rho_g * (1 - Fc) + rho_l * Fc (:202)       nu = nu_l * Fc + nu_g * (1.0 - Fc) (:203)
//   kappa(a, b) = KAPPA_CSF of kernels/curvature.h (kappa_csf there), for (a, b) in [1, nx] x [1, ny]: the normal of a cell outside is (0, 0)
// The cell (i, j) adds, first:
//   SUM_RHO   += rho[i,j]           SUM_RHO_I += rho[i,j] * i           SUM_RHO_J += rho[i,j] * j        (global integer indices as doubles)
//   SUM_GRADF += sqrt(mxsum * mxsum + mysum * mysum), (mxsum, mysum) = S(i, j), Youngs' sums of kernels/curvature.h (young_sums)
// then, if i >= 2, its west face -- the u face (i, j), 2dvof.py:209-219 --
//   w = u[i,j]      here = 0.25 * (((v[i-1,j] + v[i-1,j+1]) + v[i,j]) + v[i,j+1])
//   ddx = w > 0 ? (w - u[i-1,j]) * dxi : (u[i+1,j] - w) * dxi          ddy = here > 0 ? (w - u[i,j-1]) * dyi : (u[i,j+1] - w) * dyi
//   VX = (nu[i,j] * ((u[i-1,j] - 2 * w) + u[i+1,j])) * dxi2            VY = (nu[i,j] * ((u[i,j-1] - 2 * w) + u[i,j+1])) * dyi2
//   AX = w * ddx                                                       AY = here * ddy
//   SG = F[i,j] == F[i-1,j] ? 0 : (((((-sigma) * (F[i,j] - F[i-1,j])) * ((kappa(i,j) + kappa(i-1,j)) / 2.0)) / dx) * 2) / (rho[i,j] + rho[i-1,j])
//   A  = ((((VX + VY) - AX) - AY) + gx) + SG       (on an f64 handle w + dt * A is the predictor's u_star[i,j], bit for bit; not summed)
//   r  = (rho[i,j] + rho[i-1,j]) * 0.5 (:272)      m = r * w           dpd = (p[i,j] - p[i-1,j]) * dxi
//   KE_U += (m * w) * 0.5    P_VISC += m * (VX + VY)    P_ADV += -(m * (AX + AY))    P_GRAV += m * gx    P_SIGMA += m * SG    P_PRES += -(w * dpd)
//   MAX_ACC_SIGMA = max(MAX_ACC_SIGMA, |SG|)       (a NaN counts as +inf: cg_amax of kernels/reduce.h; starts at 0)
// then, if j >= 2, its south face -- the v face (i, j), :222-232, :277 --
//   w = v[i,j]      here = 0.25 * (((u[i,j-1] + u[i,j]) + u[i+1,j-1]) + u[i+1,j])
//   ddx = here > 0 ? (w - v[i-1,j]) * dxi : (v[i+1,j] - w) * dxi       ddy = w > 0 ? (w - v[i,j-1]) * dyi : (v[i,j+1] - w) * dyi
//   VX = (nu[i,j] * ((v[i-1,j] - 2 * w) + v[i+1,j])) * dxi2            VY = (nu[i,j] * ((v[i,j-1] - 2 * w) + v[i,j+1])) * dyi2
//   AX = here * ddx                                                    AY = w * ddy
//   SG = F[i,j] == F[i,j-1] ? 0 : (((((-sigma) * (F[i,j] - F[i,j-1])) * ((kappa(i,j) + kappa(i,j-1)) / 2.0)) / dy) * 2) / (rho[i,j] + rho[i,j-1])
//   A  = ((((VX + VY) - AX) - AY) + gy) + SG       r = (rho[i,j] + rho[i,j-1]) * 0.5       m = r * w       dpd = (p[i,j] - p[i,j-1]) * dyi
//   KE_V += (m * w) * 0.5, and the other six exactly as above with gy for gx
// SG uses the raw F, as the reference does; the skip at equal F is part of the definition (there the reference's term is a zero
// times a finite kappa), and it is what lets a lane gather kappa only where the interface crosses one of its faces.  A NaN operand
// reaches exactly the sums whose terms hold it.  No contraction: each term is the bits of the line above in either build -- every product whose
// result an addition or subtraction takes goes through mul_rounded (kernels/cells.h).
//
// Order of the sums, fixed: a lane adds its cells row by row, column by column, per cell in the order above; from there the reduction of
// kernels/reduce.h, eleven sums and one maximum wide: one partial of kEnergyPart doubles per block, folded by k_row_finish (kernels/cells.h,
// one block of 256 threads) into the row kEnergyRow describes.  No atomics, no LDS beyond the reduction.
//
// The march: a wave keeps the rows i - 1, i, i + 1 of F, u and v and the rows i - 1, i of p in registers and rotates them (four array
// passes); j -+ 1 come from the rows' edge elements, as in k_cell_rows (kernels/cell_rows.h).  The lanes that hold a face with F[i,j] != F[i-1,j] or F[i,j] != F[i,j-1]
// gather kappa of the face's two cells with the clamped loads of young_unit (rows the march has just streamed: L2 hits); a row of the
// tile without such a face skips the gather wave-uniformly.  Every face gathers for itself: taking the kappa the
// lane formed a row earlier, or the one the lane below holds, was measured and lost (profiles/energy.md).
#pragma once
#include "curvature.h"

namespace vof {

// slots of a row (= VOF_ENERGY_* of include/vof2d.h)
enum : int { EN_ISTEP = 0, EN_CELLS, EN_KE_U, EN_KE_V, EN_P_VISC, EN_P_ADV, EN_P_GRAV, EN_P_SIGMA, EN_P_PRES, EN_SUM_RHO, EN_SUM_RHO_I, EN_SUM_RHO_J,
              EN_SUM_GRADF, EN_MAX_ACC_SIGMA, EN_N = 16 };
// the reduced values: kEnergySums sums, then one maximum
enum : int { ENP_KE_U = 0, ENP_KE_V, ENP_VISC, ENP_ADV, ENP_GRAV, ENP_SIGMA, ENP_PRES, ENP_RHO, ENP_RHO_I, ENP_RHO_J, ENP_GRADF, ENP_MAX_SG };
constexpr int kEnergySums = 11, kEnergyPart = 12;
constexpr RowMap<kEnergySums, kEnergyPart - kEnergySums> kEnergyRow = {EN_N, {{ROW_ISTEP, 0}, {ROW_CELLS, 0}, {ROW_VALUE, ENP_KE_U}, {ROW_VALUE, ENP_KE_V},
    {ROW_VALUE, ENP_VISC}, {ROW_VALUE, ENP_ADV}, {ROW_VALUE, ENP_GRAV}, {ROW_VALUE, ENP_SIGMA}, {ROW_VALUE, ENP_PRES}, {ROW_VALUE, ENP_RHO},
    {ROW_VALUE, ENP_RHO_I}, {ROW_VALUE, ENP_RHO_J}, {ROW_VALUE, ENP_GRADF}, {ROW_VALUE, ENP_MAX_SG}},
    {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
static_assert(EN_KE_U == 2 && EN_P_PRES == 8 && EN_SUM_RHO == 9 && EN_SUM_GRADF == 12 && EN_MAX_ACC_SIGMA == 13, "kEnergyRow lists the slots in this order");

struct EnergyConsts {
  CurvConsts cv;   // cx, cy, kx, ky of Youngs' sums and KAPPA_CSF (eps is not read)
  double dxi, dyi, dxi2, dyi2, sigma, gx, gy, rho_g, rho_l, nu_l, nu_g;
};

__device__ __forceinline__ double energy_rho(const EnergyConsts& c, double f) {
  const double Fc = clamp01(f);
  return mul_rounded(c.rho_g, 1.0 - Fc) + mul_rounded(c.rho_l, Fc);
}
__device__ __forceinline__ double energy_nu(const EnergyConsts& c, double f) {
  const double Fc = clamp01(f);
  return mul_rounded(c.nu_l, Fc) + mul_rounded(c.nu_g, 1.0 - Fc);
}
// SG of a face between the cell (raw F f0, density r0, curvature k0) and the cell it looks back to (fb, rb, kb); h: dx or dy
__device__ __forceinline__ double energy_sg(const EnergyConsts& c, double f0, double fb, double k0, double kb, double h, double r0, double rb) {
  const double fk = (((-c.sigma) * (f0 - fb)) * ((k0 + kb) / 2.0)) / h;
  return f0 == fb ? 0.0 : (fk * 2.0) / (r0 + rb);
}
// One face: w the face's velocity, xm / xp and ym / yp its neighbours along i and j, posx / posy the upwind selections, advx / advy what
// multiplies ddx / ddy, g the gravity along the component, r the face density, dpd the pressure gradient across the face.  KE: ENP_KE_U or ENP_KE_V.
template <int KE>
__device__ __forceinline__ void energy_face(const EnergyConsts& c, double w, double xm, double xp, double ym, double yp, bool posx, bool posy, double advx,
                                            double advy, double nu, double g, double SG, double r, double dpd, double (&acc)[kEnergyPart]) {
  const double ddx = posx ? (w - xm) * c.dxi : (xp - w) * c.dxi;
  const double ddy = posy ? (w - ym) * c.dyi : (yp - w) * c.dyi;
  const double w2 = mul_rounded(2.0, w);
  const double VX = mul_rounded(nu * ((xm - w2) + xp), c.dxi2);
  const double VY = mul_rounded(nu * ((ym - w2) + yp), c.dyi2);
  const double AX = mul_rounded(advx, ddx), AY = mul_rounded(advy, ddy);
  const double m = r * w;
  acc[KE] += mul_rounded(m * w, 0.5);
  acc[ENP_VISC] += mul_rounded(m, VX + VY);
  acc[ENP_ADV] += -mul_rounded(m, AX + AY);
  acc[ENP_GRAV] += mul_rounded(m, g);
  acc[ENP_SIGMA] += mul_rounded(m, SG);
  acc[ENP_PRES] += -mul_rounded(w, dpd);
  acc[ENP_MAX_SG] = cg_amax(acc[ENP_MAX_SG], SG);
}

// ------------------------------------------------------------------ the pass over F, u, v, p
template <typename T, int V>
__global__ __launch_bounds__(256) void k_energy(Geom g, const T* __restrict__ F, const T* __restrict__ u, const T* __restrict__ v, const T* __restrict__ p, int R,
                                                 EnergyConsts c, double* __restrict__ part) {
  int j0, ra, rb;
  const bool active = cell_tile<V>(g, R, j0, ra, rb);
  double acc[kEnergyPart] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (active) {
    const int ny = g.ny;
    const int64_t pitch = g.pitch;
    size_t o = at(g, ra, j0);
    Row<T, V> Fm, F0, Fp, um, u0, up, vm, v0, vp, p0;
    T pm[V];
    load_row<T, V>(Fm, F + o - pitch);
    load_row<T, V>(F0, F + o);
    load_row<T, V>(um, u + o - pitch);
    load_row<T, V>(u0, u + o);
    load_row<T, V>(vm, v + o - pitch);
    load_row<T, V>(v0, v + o);
    load_c<T, V>(pm, p + o - pitch);
    for (int i = ra; i <= rb; ++i) {
      load_row<T, V>(Fp, F + o + pitch);
      load_row<T, V>(up, u + o + pitch);
      load_row<T, V>(vp, v + o + pitch);
      load_c<T, V>(p0.c, p + o);
      p0.l = p[o - 1];
      const bool has_west = i >= 2;   // (wave-uniform)
      // ---- the interface gather: kappa of the cell, of its west and of its south neighbour, where a face of the cell needs them
      bool fw[V], fs[V];
      bool any = false;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const bool live = j0 + q <= ny;
        fw[q] = live && has_west && F0.c[q] != Fm.c[q];
        fs[q] = live && j0 + q >= 2 && F0.c[q] != left_of(F0, q);
        any = any || fw[q] || fs[q];
      }
      double kc[V], kw[V], ks[V];
#pragma unroll
      for (int q = 0; q < V; ++q) kc[q] = kw[q] = ks[q] = 0.0;
      if (__builtin_amdgcn_ballot_w64(any) != 0ull) {   // (wave-uniform skip: the rows of a tile in which F is flat hold no such face)
#pragma unroll
        for (int q = 0; q < V; ++q) {
          if (fw[q] || fs[q]) kc[q] = kappa_csf<T>(c.cv, g, F, i, j0 + q);
          if (fw[q]) kw[q] = kappa_csf<T>(c.cv, g, F, i - 1, j0 + q);
          if (fs[q]) ks[q] = kappa_csf<T>(c.cv, g, F, i, j0 + q - 1);
        }
      }
      const double di = (double)i;
#pragma unroll
      for (int q = 0; q < V; ++q) {
        const int j = j0 + q;
        if (j <= ny) {
          const double fm[3] = {(double)left_of(Fm, q), (double)Fm.c[q], (double)right_of(Fm, q)};
          const double f0[3] = {(double)left_of(F0, q), (double)F0.c[q], (double)right_of(F0, q)};
          const double fp[3] = {(double)left_of(Fp, q), (double)Fp.c[q], (double)right_of(Fp, q)};
          const double rho = energy_rho(c, f0[1]), nu = energy_nu(c, f0[1]);
          acc[ENP_RHO] += rho;
          acc[ENP_RHO_I] += mul_rounded(rho, di);
          acc[ENP_RHO_J] += mul_rounded(rho, (double)j);
          double mxsum, mysum;
          young_sums(c.cv, fm, f0, fp, mxsum, mysum);
          acc[ENP_GRADF] += __builtin_sqrt(mul_rounded(mxsum, mxsum) + mul_rounded(mysum, mysum));
          const double u00 = (double)u0.c[q], v00 = (double)v0.c[q], p00 = (double)p0.c[q];
          if (has_west) {
            const double here = 0.25 * ((((double)vm.c[q] + (double)right_of(vm, q)) + v00) + (double)right_of(v0, q));
            const double rhob = energy_rho(c, fm[1]);
            const double SG = energy_sg(c, f0[1], fm[1], kc[q], kw[q], c.cv.dx, rho, rhob);
            energy_face<ENP_KE_U>(c, u00, (double)um.c[q], (double)up.c[q], (double)left_of(u0, q), (double)right_of(u0, q), u00 > 0.0, here > 0.0, u00, here,
                                  nu, c.gx, SG, (rho + rhob) * 0.5, (p00 - (double)pm[q]) * c.dxi, acc);
          }
          if (j >= 2) {
            const double here = 0.25 * ((((double)left_of(u0, q) + u00) + (double)left_of(up, q)) + (double)up.c[q]);
            const double rhob = energy_rho(c, f0[0]);
            const double SG = energy_sg(c, f0[1], f0[0], kc[q], ks[q], c.cv.dy, rho, rhob);
            energy_face<ENP_KE_V>(c, v00, (double)vm.c[q], (double)vp.c[q], (double)left_of(v0, q), (double)right_of(v0, q), here > 0.0, v00 > 0.0, here, v00,
                                  nu, c.gy, SG, (rho + rhob) * 0.5, (p00 - (double)left_of(p0, q)) * c.dyi, acc);
          }
        }
      }
      Fm = F0; F0 = Fp;
      um = u0; u0 = up;
      vm = v0; v0 = vp;
#pragma unroll
      for (int q = 0; q < V; ++q) pm[q] = p0.c[q];
      o += pitch;
    }
  }
  block_publish<kEnergySums, kEnergyPart - kEnergySums>(acc, part);
}

}  // namespace vof
