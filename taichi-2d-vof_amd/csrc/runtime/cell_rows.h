// runtime/cell_rows.h -- vof_interface and vof_curvature: the one host path of the verbs that emit a row per interface cell (kernels/cell_rows.h): the handle's buffers, the launches of k_cell_rows (count), k_cell_rows_scan, k_cell_rows (emit), the copies out
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "diag_reduce.h"

namespace {

static_assert(IF_N == VOF_IFACE_N && IF_NY == VOF_IFACE_NY && IFS_N == VOF_IFACE_SUM_N && IFS_ISTEP == VOF_IFACE_SUM_ISTEP,
              "kernels/interface.h and include/vof2d.h name the same slots");
static_assert(CV_N == VOF_CURV_N && CV_KAPPA == VOF_CURV_KAPPA && CV_KAPPA_CSF == VOF_CURV_KAPPA_CSF && CV_F == VOF_CURV_F, "kernels/curvature.h and include/vof2d.h name the same slots of a row");
static_assert(CVS_N == VOF_CURV_SUM_N && CVS_ROWS == VOF_CURV_SUM_ROWS && CVS_VALID == VOF_CURV_SUM_VALID && CVS_MAX_K == VOF_CURV_SUM_MAX_K &&
                  CVS_MAX_CSF == VOF_CURV_SUM_MAX_CSF && CVS_ISTEP == VOF_CURV_SUM_ISTEP,
              "kernels/curvature.h and include/vof2d.h name the same slots of the summary");

// rows per wave chunk: the cells-per-wave rule (every chunk re-reads two rows of F; the chunk length fixes the order of the
// sums, so it depends on the geometry alone).  vof_blobs marches in the same chunks (runtime/blobs.h).
inline int cell_rows_chunk(const vof2d_ctx* h) { return chunk_rows(h, h->g.ntj, 4, 32); }

// A verb of kernels/cell_rows.h on the host: its two buffers, the constants its kernels get, the slot of the summary that holds
// the number of rows, what it says when there is no memory.  The widths of a row, the partials and the summary are the kernel verb's.
template <typename Verb>
struct CellRowsVerb {
  CellRowBufs WorkBufs::*bufs;
  typename Verb::Consts (*consts)(const vof2d_ctx* h, double eps);
  int count_slot;
  const char* no_work;
  const char* no_rows;
};
constexpr CellRowsVerb<IfaceVerb> kIfaceRows = {
    &WorkBufs::iface, [](const vof2d_ctx* h, double eps) { return IfaceConsts{eps, 1.0 - eps, h->cd.nrm_x, h->cd.nrm_y, h->cd.dx, h->cd.dy}; }, IFS_SEGMENTS,
    "vof_interface: no memory for the counts", "vof_interface: no memory for the segments"};
constexpr CellRowsVerb<CurvVerb> kCurvRows = {
    &WorkBufs::curv,
    [](const vof2d_ctx* h, double eps) { return CurvConsts{eps, 1.0 - eps, h->cd.nrm_x, h->cd.nrm_y, h->cd.dx, h->cd.dy, h->cd.kap_x, h->cd.kap_y}; }, CVS_ROWS,
    "vof_curvature: no memory for the counts", "vof_curvature: no memory for the rows"};

template <typename Verb>
inline CellRowsCarve cell_rows_carve(const vof2d_ctx* h) {
  const Reported rep = reported(h);
  return carve_cell_rows((size_t)rep.entries(), (size_t)rep.blocks(cell_rows_chunk(h)) * (Verb::NS + Verb::NM), Verb::SUM_N);
}

// The work buffer (once: the counts / offsets, the block partials, the summary) and room for `rows` rows on the device (grown on
// demand).  Called while nothing of the call is enqueued.
template <typename Verb>
int cell_rows_prepare(vof2d_ctx* h, const CellRowsVerb<Verb>& verb, int64_t rows) {
  CellRowBufs& b = h->buf.*verb.bufs;
  if (const int rc = b.work.reserve(h, cell_rows_carve<Verb>(h).total, verb.no_work)) return rc;
  return b.rows.reserve(h, (size_t)rows * Verb::ROW_N * sizeof(double), verb.no_rows);
}

template <typename T, bool EMIT, typename Verb>
void cell_rows_launch(vof2d_ctx* h, const CellRowsVerb<Verb>& verb, double eps, int64_t cap) {
  constexpr int V = VecWidth<T>::V;
  const Reported rep = reported(h);
  const CellRowsCarve cv = cell_rows_carve<Verb>(h);
  const unsigned nb = rep.blocks(cell_rows_chunk(h));
  const CellRowBufs& b = h->buf.*verb.bufs;
  int* const cnt = b.work.as<int>(cv.cnt);
  double* const part = b.work.as<double>(cv.part);
  if (nb)
    launch(h, kOther, k_cell_rows<Verb, T, V, EMIT>, dim3(nb), 0, rep.g, (const T*)F_<T>(h, fF), cell_rows_chunk(h), verb.consts(h, eps), cnt, part,
           b.rows.as<double>(), (long long)cap);
  if (!EMIT)
    launch_block(h, kOther, k_cell_rows_scan<Verb>, dim3(1), (unsigned)kScanThreads, 0, cnt, (long long)rep.entries(), (const double*)part, (int)nb,
                 b.work.as<double>(cv.sum), (double)h->istep);
}

// The rows of the field F as vof_get_field would return it now: settle_ghosts first (the stencils of a cell beside a wall hold
// ghost cells, which a fused step may have left virtual), count + scan, the summary to the host, then -- the stream is idle
// again -- room for min(rows counted, cap_rows) rows, the emit pass and the copy of those rows.
template <typename Verb>
int cell_rows_run(vof2d_ctx* h, const CellRowsVerb<Verb>& verb, double eps, double* rows, int64_t cap_rows, double* summary) {
  int rc = cell_rows_prepare(h, verb, 0);
  if (rc) return rc;
  settle_ghosts(h);
  DISPATCH_T(h, (cell_rows_launch<double, false>(h, verb, eps, 0)), (cell_rows_launch<float, false>(h, verb, eps, 0)));
  if ((rc = ensure_ok(h))) return rc;
  const CellRowBufs& b = h->buf.*verb.bufs;
  if ((rc = read_back(h, summary, b.work.as<double>(cell_rows_carve<Verb>(h).sum), Verb::SUM_N * sizeof(double)))) return rc;
  int64_t n = (int64_t)summary[verb.count_slot];
  if (n > cap_rows) n = cap_rows;
  if (n <= 0) return VOF_OK;
  if ((rc = cell_rows_prepare(h, verb, n))) return rc;
  DISPATCH_T(h, (cell_rows_launch<double, true>(h, verb, eps, n)), (cell_rows_launch<float, true>(h, verb, eps, n)));
  if ((rc = ensure_ok(h))) return rc;
  return read_back(h, rows, b.rows.p, (size_t)n * Verb::ROW_N * sizeof(double));
}

}  // namespace
