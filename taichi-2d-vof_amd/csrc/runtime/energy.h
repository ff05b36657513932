// runtime/energy.h -- vof_energy and vof_step_energy: the launch of k_energy on the reduced-row path (runtime/diag_reduce.h), the stepping loop that records rows
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "cell_rows.h"

namespace {

static_assert(EN_N == VOF_ENERGY_N && EN_ISTEP == VOF_ENERGY_ISTEP && EN_CELLS == VOF_ENERGY_CELLS && EN_KE_U == VOF_ENERGY_KE_U && EN_KE_V == VOF_ENERGY_KE_V &&
                  EN_P_VISC == VOF_ENERGY_P_VISC && EN_P_ADV == VOF_ENERGY_P_ADV && EN_P_GRAV == VOF_ENERGY_P_GRAV && EN_P_SIGMA == VOF_ENERGY_P_SIGMA &&
                  EN_P_PRES == VOF_ENERGY_P_PRES && EN_SUM_RHO == VOF_ENERGY_SUM_RHO && EN_SUM_RHO_I == VOF_ENERGY_SUM_RHO_I && EN_SUM_RHO_J == VOF_ENERGY_SUM_RHO_J &&
                  EN_SUM_GRADF == VOF_ENERGY_SUM_GRADF && EN_MAX_ACC_SIGMA == VOF_ENERGY_MAX_ACC_SIGMA,
              "kernels/energy.h and include/vof2d.h name the same slots");

constexpr ReducedVerb<kEnergySums, kEnergyPart - kEnergySums> kEnergyVerb = {&WorkBufs::energy, kEnergyRow, "vof_energy: no memory for the reduction buffer",
                                                                             "vof_step_energy: no memory for the rows"};
// One row of the energy budget into slot `slot` of the device rows (reduced_enqueue settles the ghost cells first: the stencils of the
// cells beside a wall hold them).  The chunk length is diag_chunk's: it fixes the order of the sums.
int energy_enqueue(vof2d_ctx* h, int64_t slot) {
  const ConstsD& d = h->cd;
  const EnergyConsts c = {{0.0, 1.0, d.nrm_x, d.nrm_y, d.dx, d.dy, d.kap_x, d.kap_y}, d.dxi, d.dyi, d.dxi2, d.dyi2, d.sigma, d.gx, d.gy, d.rho_g, d.rho_l, d.nu_l, d.nu_g};
  return reduced_enqueue(h, kEnergyVerb, slot, [&](auto t, const Geom& g, unsigned nb, int R, double* part) {
    using T = decltype(t);
    launch(h, kOther, k_energy<T, VecWidth<T>::V>, dim3(nb), 0, g, (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), (const T*)F_<T>(h, fP), R, c,
           part);
  });
}

// step_groups_n (runtime/step.h) with a row behind every group, one read-back at the end
int step_energy_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, double* out, int64_t* rows_written) {
  const int64_t rows = nsteps / every;
  int rc = reduced_prepare(h, kEnergyVerb, rows);
  if (rc) return rc;
  if ((rc = step_groups_n(h, nsteps, every, cycles, criterion, [&](int64_t r) { return energy_enqueue(h, r); }))) return rc;
  if (rows > 0 && (rc = read_back(h, out, h->buf.energy.rows.p, (size_t)rows * EN_N * sizeof(double)))) return rc;
  if (rows_written) *rows_written = rows;
  return VOF_OK;
}

}  // namespace
