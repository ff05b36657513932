// runtime/curvature.h -- vof_curvature: the handle's buffers, the launches of k_curv (count), k_curv_scan, k_curv (emit), the copies out
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "interface.h"

namespace {

static_assert(CV_N == VOF_CURV_N && CV_KAPPA == VOF_CURV_KAPPA && CV_KAPPA_CSF == VOF_CURV_KAPPA_CSF && CV_F == VOF_CURV_F, "kernels/curvature.h and include/vof2d.h name the same slots of a row");
static_assert(CVS_N == VOF_CURV_SUM_N && CVS_ROWS == VOF_CURV_SUM_ROWS && CVS_VALID == VOF_CURV_SUM_VALID && CVS_MAX_K == VOF_CURV_SUM_MAX_K &&
                  CVS_MAX_CSF == VOF_CURV_SUM_MAX_CSF && CVS_ISTEP == VOF_CURV_SUM_ISTEP,
              "kernels/curvature.h and include/vof2d.h name the same slots of the summary");

// rows per wave chunk: that of vof_interface (every chunk re-reads two rows of F; the chunk length fixes the order of the sums, so it
// depends on the geometry alone)
inline int curv_chunk(const vof2d_ctx* h) { return iface_chunk(h); }
inline CurvCarve curv_carve(const vof2d_ctx* h) {
  const Reported rep = reported(h);
  return carve_curv((size_t)rep.entries(), (size_t)rep.blocks(curv_chunk(h)) * CVP_N, CVS_N);
}

// The work buffer (once: the counts / offsets, the block partials, the summary) and room for `rows` rows on the device (grown on
// demand).  Called while nothing of the call is enqueued.
int curv_prepare(vof2d_ctx* h, int64_t rows) {
  if (const int rc = h->buf.curv_work.reserve(h, curv_carve(h).total, "vof_curvature: no memory for the counts")) return rc;
  return h->buf.curv_rows.reserve(h, (size_t)rows * CV_N * sizeof(double), "vof_curvature: no memory for the rows");
}

template <typename T, bool EMIT>
void curv_launch(vof2d_ctx* h, double eps, int64_t cap) {
  constexpr int V = VecWidth<T>::V;
  const Reported rep = reported(h);
  const CurvCarve cv = curv_carve(h);
  const unsigned nb = rep.blocks(curv_chunk(h));
  int* const cnt = h->buf.curv_work.as<int>(cv.cnt);
  double* const part = h->buf.curv_work.as<double>(cv.part);
  const CurvConsts c = {eps, 1.0 - eps, h->cd.nrm_x, h->cd.nrm_y, h->cd.dx, h->cd.dy, h->cd.kap_x, h->cd.kap_y};
  if (nb)
    launch(h, kOther, k_curv<T, V, EMIT>, dim3(nb), 0, rep.g, (const T*)F_<T>(h, fF), curv_chunk(h), c, cnt, part, h->buf.curv_rows.as<double>(),
           (long long)cap);
  if (!EMIT)
    launch_block(h, kOther, k_curv_scan, dim3(1), (unsigned)kCurvScanThreads, 0, cnt, (long long)rep.entries(), (const double*)part, (int)nb,
                 h->buf.curv_work.as<double>(cv.sum), (double)h->istep);
}

// The curvature rows of the field F as vof_get_field would return it now: settle_ghosts first (the stencils of a cell beside a wall
// hold ghost cells, which a fused step may have left virtual), count + scan, the summary to the host, then -- the stream is idle
// again -- room for min(ROWS, cap_rows) rows, the emit pass and the copy of those rows.
int curv_run(vof2d_ctx* h, double eps, double* rows, int64_t cap_rows, double* summary) {
  int rc = curv_prepare(h, 0);
  if (rc) return rc;
  settle_ghosts(h);
  DISPATCH_T(h, (curv_launch<double, false>(h, eps, 0)), (curv_launch<float, false>(h, eps, 0)));
  if ((rc = ensure_ok(h))) return rc;
  if ((rc = read_back(h, summary, h->buf.curv_work.as<double>(curv_carve(h).sum), CVS_N * sizeof(double)))) return rc;
  int64_t n = (int64_t)summary[CVS_ROWS];
  if (n > cap_rows) n = cap_rows;
  if (n <= 0) return VOF_OK;
  if ((rc = curv_prepare(h, n))) return rc;
  DISPATCH_T(h, (curv_launch<double, true>(h, eps, n)), (curv_launch<float, true>(h, eps, n)));
  if ((rc = ensure_ok(h))) return rc;
  return read_back(h, rows, h->buf.curv_rows.p, (size_t)n * CV_N * sizeof(double));
}

}  // namespace
