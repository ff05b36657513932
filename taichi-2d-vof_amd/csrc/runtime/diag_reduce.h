// runtime/diag_reduce.h -- vof_diagnostics and vof_step_diag: the reduced-row path they share with vof_dye_stats (reduced_prepare, reduced_enqueue), the launch of k_diag, the stepping loop that records rows
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
// (runtime/diag.h is something else: the vof_debug_* entry points of the diagnostic build.)
#pragma once
#include "step.h"

namespace {

static_assert(DG_N == VOF_DIAG_N && DG_CELLS == VOF_DIAG_CELLS && DG_MAX_F == VOF_DIAG_MAX_F, "kernels/diag.h and include/vof2d.h name the same slots");

// The cells a handle reports (ReportedRows, runtime/rows.h) and the geometry a launch on them gets: cell_tile cuts [g.ilo, g.ihi] into chunks
struct Reported : ReportedRows { Geom g; };
inline Reported reported(const vof2d_ctx* h) {
  Reported r{reported_rows(h->d.row_lo, h->d.row_hi, h->d.own_lo, h->d.own_hi, h->d.nx, h->g.ny, h->g.ntj), h->g};
  r.g.ilo = r.range.first; r.g.ihi = r.range.last;
  return r;
}
// rows per wave chunk: the cells-per-wave rule (every chunk re-reads one row of u; few, long chunks keep the partials few)
inline int diag_chunk(const vof2d_ctx* h) { return chunk_rows(h, h->g.ntj, 2, 16); }

// ------------------------------------------------------------------ the reduced-row path
// A verb that reduces the reported cells to rows of map.n doubles (a pass that ends in block_publish<NS, NM>, then k_row_finish of
// kernels/cells.h): its two buffers, the row from the reduced values, what it says when there is no memory
template <int NS, int NM>
struct ReducedVerb { RowBufs WorkBufs::*bufs; RowMap<NS, NM> map; const char* no_part; const char* no_rows; };
// The partials buffer (once) and room for `rows` rows on the device (grown on demand: the old rows are given up, nobody
// reads them after the call that recorded them).  Called before anything of the call is enqueued.
template <int NS, int NM>
int reduced_prepare(vof2d_ctx* h, const ReducedVerb<NS, NM>& verb, int64_t rows) {
  RowBufs& b = h->buf.*verb.bufs;
  const size_t part = (size_t)reported(h).blocks(diag_chunk(h)) * (NS + NM) + 1;
  if (const int rc = b.part.reserve(h, part * sizeof(double), verb.no_part)) return rc;
  return b.rows.reserve(h, (size_t)(rows < 1 ? 1 : rows) * verb.map.n * sizeof(double), verb.no_rows);
}
// One row of the fields as vof_get_field would return them now, into slot `slot` of the device rows: settle_ghosts first (the wall faces
// u[1,j], u[nx+1,j] are ghost-like and may be virtual after a fused step; a k_tm batch may have left the predictor ahead), then pass(T(), geometry,
// blocks, chunk rows, partials) -- the verb's kernel; not launched where no cell is reported: the finish forms the row from map.init.  Enqueues only.
template <int NS, int NM, typename Pass>
int reduced_enqueue(vof2d_ctx* h, const ReducedVerb<NS, NM>& verb, int64_t slot, Pass&& pass) {
  settle_ghosts(h);
  const Reported rep = reported(h);
  const unsigned nb = rep.blocks(diag_chunk(h));
  RowBufs& b = h->buf.*verb.bufs;
  double* const part = b.part.as<double>();
  if (nb) DISPATCH_T(h, pass(double(), rep.g, nb, diag_chunk(h), part), pass(float(), rep.g, nb, diag_chunk(h), part));
  launch(h, kOther, k_row_finish<NS, NM>, dim3(1), 0, (const double*)part, (int)nb, b.rows.as<double>() + slot * verb.map.n, (double)h->istep,
         (double)rep.cells(), verb.map);
  return ensure_ok(h);
}

// ------------------------------------------------------------------ vof_diagnostics, vof_step_diag
constexpr ReducedVerb<kDiagSums, kDiagPart - kDiagSums> kDiagVerb = {&WorkBufs::diag, kDiagRow, "vof_diagnostics: no memory for the reduction buffer",
                                                                     "vof_step_diag: no memory for the rows"};
int diag_enqueue(vof2d_ctx* h, int64_t slot) {
  return reduced_enqueue(h, kDiagVerb, slot, [&](auto t, const Geom& g, unsigned nb, int R, double* part) {
    using T = decltype(t);
    launch(h, kOther, k_diag<T, VecWidth<T>::V>, dim3(nb), 0, g, (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), R, h->cd.dxi,
           h->cd.dyi, h->cd.rho_g, h->cd.rho_l, part);
  });
}

// step_groups_n (runtime/step.h) with a row behind every group, one read-back at the end
int step_diag_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, double* out, int64_t* rows_written) {
  const int64_t rows = nsteps / every;
  int rc = reduced_prepare(h, kDiagVerb, rows);
  if (rc) return rc;
  if ((rc = step_groups_n(h, nsteps, every, cycles, criterion, [&](int64_t r) { return diag_enqueue(h, r); }))) return rc;
  if (rows > 0 && (rc = read_back(h, out, h->buf.diag.rows.p, (size_t)rows * DG_N * sizeof(double)))) return rc;
  if (rows_written) *rows_written = rows;
  return VOF_OK;
}

}  // namespace
