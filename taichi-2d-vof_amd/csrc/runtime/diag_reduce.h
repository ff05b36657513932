// runtime/diag_reduce.h -- vof_diagnostics and vof_step_diag: the handle's buffers, the launch of k_diag + k_diag_finish, the stepping loop that records rows
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
// (runtime/diag.h is something else: the vof_debug_* entry points of the diagnostic build.)
#pragma once
#include "step.h"

namespace {

static_assert(DG_N == VOF_DIAG_N && DG_CELLS == VOF_DIAG_CELLS && DG_MAX_F == VOF_DIAG_MAX_F, "kernels/diag.h and include/vof2d.h name the same slots");

// The cells a handle reports (ReportedRows, runtime/rows.h) and the geometry a launch on them gets: cg_tile cuts [g.ilo, g.ihi] into chunks
struct Reported : ReportedRows { Geom g; };
inline Reported reported(const vof2d_ctx* h) {
  Reported r{reported_rows(h->d.row_lo, h->d.row_hi, h->d.own_lo, h->d.own_hi, h->d.nx, h->g.ny, h->g.ntj), h->g};
  r.g.ilo = r.range.first; r.g.ihi = r.range.last;
  return r;
}
// rows per wave chunk: the cells-per-wave rule (every chunk re-reads one row of u; few, long chunks keep the partials few)
inline int diag_chunk(const vof2d_ctx* h) { return chunk_rows(h, h->g.ntj, 2, 16); }

// The partials buffer (once) and room for `rows` rows of diagnostics on the device (grown on demand: the old rows are
// given up, nobody reads them after the call that recorded them).  Called before anything of the call is enqueued.
int diag_prepare(vof2d_ctx* h, int64_t rows) {
  const size_t part = (size_t)reported(h).blocks(diag_chunk(h)) * kDiagPart + 1;
  if (const int rc = h->buf.diag_part.reserve(h, part * sizeof(double), "vof_diagnostics: no memory for the reduction buffer")) return rc;
  return h->buf.diag_rows.reserve(h, (size_t)(rows < 1 ? 1 : rows) * DG_N * sizeof(double), "vof_step_diag: no memory for the rows");
}

// One row of diagnostics of the fields as vof_get_field would return them now, into slot `slot` of the device rows:
// settle_ghosts first (the wall faces u[1,j], u[nx+1,j] are ghost-like and may be virtual after a fused step; a k_tm
// batch may have left the predictor ahead), then the current views of F, u, v.  Enqueues only.
template <typename T>
void diag_launch(vof2d_ctx* h, int64_t slot) {
  constexpr int V = VecWidth<T>::V;
  const Reported rep = reported(h);
  const unsigned nb = rep.blocks(diag_chunk(h));
  double* const part = h->buf.diag_part.as<double>();
  if (nb)
    launch(h, kOther, k_diag<T, V>, dim3(nb), 0, rep.g, (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), diag_chunk(h),
           h->cd.dxi, h->cd.dyi, h->cd.rho_g, h->cd.rho_l, part);
  launch(h, kOther, k_diag_finish, dim3(1), 0, (const double*)part, (int)nb, h->buf.diag_rows.as<double>() + slot * DG_N, (double)h->istep, (double)rep.cells());
}
int diag_enqueue(vof2d_ctx* h, int64_t slot) {
  settle_ghosts(h);
  DISPATCH_T(h, diag_launch<double>(h, slot), diag_launch<float>(h, slot));
  return ensure_ok(h);
}

// step_groups_n (runtime/step.h) with a row behind every group, one read-back at the end
int step_diag_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, double* out, int64_t* rows_written) {
  const int64_t rows = nsteps / every;
  int rc = diag_prepare(h, rows);
  if (rc) return rc;
  if ((rc = step_groups_n(h, nsteps, every, cycles, criterion, [&](int64_t r) { return diag_enqueue(h, r); }))) return rc;
  if (rows > 0 && (rc = read_back(h, out, h->buf.diag_rows.p, (size_t)rows * DG_N * sizeof(double)))) return rc;
  if (rows_written) *rows_written = rows;
  return VOF_OK;
}

}  // namespace
