// runtime/diag_reduce.h -- vof_diagnostics and vof_step_diag: the handle's buffers, the launch of k_diag + k_diag_finish, the stepping loop that records rows
//
// Part of the host-side runtime of libvof2d_hip.so; included (once, in this order) by vof2d_api.hip:
// context.h (with state.h), launches.h, graphs.h, schedule.h, multigrid.h, step.h, diag_reduce.h, comm.h, selftest.h.  Everything here has
// internal linkage.  (runtime/diag.h is something else: the vof_debug_* entry points of the diagnostic build.)
#pragma once
#include "step.h"

namespace {

static_assert(DG_N == VOF_DIAG_N && DG_CELLS == VOF_DIAG_CELLS && DG_MAX_F == VOF_DIAG_MAX_F, "kernels/diag.h and include/vof2d.h name the same slots");

// The cells a handle reports: its owned interior rows, inside what it can compute (row own_hi + 1 of u is read: a strip
// stores it as a halo row, a full domain as the wall's ghost row)
inline void diag_rows_of(const vof2d_ctx* h, int& lo, int& hi) {
  lo = h->d.own_lo > h->g.ilo ? h->d.own_lo : h->g.ilo;
  hi = h->d.own_hi < h->g.ihi ? h->d.own_hi : h->g.ihi;
}
// rows per wave chunk: the cells-per-wave rule (every chunk re-reads one row of u; few, long chunks keep the partials few)
inline int diag_chunk(const vof2d_ctx* h) { return chunk_rows(h, h->g.ntj, 2, 16); }
inline unsigned diag_blocks(const vof2d_ctx* h) {
  int lo, hi;
  diag_rows_of(h, lo, hi);
  return hi < lo ? 0u : blocks_rows(hi - lo + 1, h->g.ntj, diag_chunk(h));
}

// The partials buffer (once) and room for `rows` rows of diagnostics on the device (grown on demand: the old rows are
// given up, nobody reads them after the call that recorded them).  Called before anything of the call is enqueued.
int diag_prepare(vof2d_ctx* h, int64_t rows) {
  if (!h->diag_part) {
    const size_t n = (size_t)diag_blocks(h) * kDiagPart + 1;
    if (hipMalloc(reinterpret_cast<void**>(&h->diag_part), n * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      h->diag_part = nullptr;
      return fail(h, VOF_ENOMEM, "vof_diagnostics: no memory for the reduction buffer");
    }
  }
  if (rows < 1) rows = 1;
  if (h->diag_cap >= rows) return VOF_OK;
  if (h->diag_rows) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    (void)hipFree(h->diag_rows);
    h->diag_rows = nullptr;
    h->diag_cap = 0;
  }
  if (hipMalloc(reinterpret_cast<void**>(&h->diag_rows), (size_t)rows * DG_N * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    h->diag_rows = nullptr;
    return fail(h, VOF_ENOMEM, "vof_step_diag: no memory for the rows");
  }
  h->diag_cap = rows;
  return VOF_OK;
}
void diag_release(vof2d_ctx* h) {
  if (h->diag_part) (void)hipFree(h->diag_part);
  if (h->diag_rows) (void)hipFree(h->diag_rows);
  h->diag_part = h->diag_rows = nullptr;
  h->diag_cap = 0;
}

// One row of diagnostics of the fields as vof_get_field would return them now, into slot `slot` of the device rows:
// settle_ghosts first (the wall faces u[1,j], u[nx+1,j] are ghost-like and may be virtual after a fused step; a k_tm
// batch may have left the predictor ahead), then the current views of F, u, v.  Enqueues only.
template <typename T>
void diag_launch(vof2d_ctx* h, int64_t slot) {
  constexpr int V = VecWidth<T>::V;
  int lo, hi;
  diag_rows_of(h, lo, hi);
  const unsigned nb = diag_blocks(h);
  Geom g = h->g;
  g.ilo = lo; g.ihi = hi;   // (cg_tile cuts [g.ilo, g.ihi] into chunks)
  if (nb)
    launch(h, kOther, k_diag<T, V>, dim3(nb), 0, g, (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), diag_chunk(h),
           h->cd.dxi, h->cd.dyi, h->cd.rho_g, h->cd.rho_l, h->diag_part);
  const double cells = hi < lo ? 0.0 : (double)(hi - lo + 1) * (double)h->g.ny;
  launch(h, kOther, k_diag_finish, dim3(1), 0, (const double*)h->diag_part, (int)nb, h->diag_rows + slot * DG_N, (double)h->istep, cells);
}
int diag_enqueue(vof2d_ctx* h, int64_t slot) {
  settle_ghosts(h);
  DISPATCH_T(h, diag_launch<double>(h, slot), diag_launch<float>(h, slot));
  return ensure_ok(h);
}

// nsteps steps in groups of `every`, a row behind every group, one read-back at the end.  The entry point has checked
// the arguments, that the handle is a full domain and that no phased step is in progress.
int step_diag_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, double* out, int64_t* rows_written) {
  const int64_t rows = nsteps / every;
  int rc = diag_prepare(h, rows);
  if (rc) return rc;
  auto steps = [&](int64_t n) { return cycles > 0 ? step_mg_n(h, n, cycles, criterion, nullptr, nullptr, nullptr) : step_n(h, n); };
  for (int64_t r = 0; r < rows; ++r) {
    if ((rc = steps(every))) return rc;
    if ((rc = diag_enqueue(h, r))) return rc;
  }
  if (nsteps % every && (rc = steps(nsteps % every))) return rc;
  if (rows > 0) {
    HIPCHK(h, hipMemcpyAsync(out, h->diag_rows, (size_t)rows * DG_N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  if (rows_written) *rows_written = rows;
  return VOF_OK;
}

}  // namespace
