// runtime/interface.h -- vof_interface: the handle's buffers, the launches of k_iface (count), k_iface_scan, k_iface (emit), the copies out
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "diag_reduce.h"

namespace {

static_assert(IF_N == VOF_IFACE_N && IF_NY == VOF_IFACE_NY && IFS_N == VOF_IFACE_SUM_N && IFS_ISTEP == VOF_IFACE_SUM_ISTEP,
              "kernels/interface.h and include/vof2d.h name the same slots");

// rows per wave chunk: the cells-per-wave rule (every chunk re-reads two rows of F; the chunk length fixes the order of the
// LENGTH sum, so it depends on the geometry alone)
inline int iface_chunk(const vof2d_ctx* h) { return chunk_rows(h, h->g.ntj, 4, 32); }

// The work buffer (once: the counts / offsets, the block partials, the summary) and room for `rows` segments on the device
// (grown on demand).  Called while nothing of the call is enqueued.
int iface_prepare(vof2d_ctx* h, int64_t rows) {
  const Reported rep = reported(h);
  const IfaceCarve c = carve_iface((size_t)rep.entries(), (size_t)rep.blocks(iface_chunk(h)) * kIfacePart + IFS_N);
  if (const int rc = h->buf.iface_work.reserve(h, c.total, "vof_interface: no memory for the counts")) return rc;
  h->iface_part = h->buf.iface_work.as<double>(c.part);
  return h->buf.iface_rows.reserve(h, (size_t)rows * IF_N * sizeof(double), "vof_interface: no memory for the segments");
}

template <typename T, bool EMIT>
void iface_launch(vof2d_ctx* h, double eps, int64_t cap) {
  constexpr int V = VecWidth<T>::V;
  const Reported rep = reported(h);
  const unsigned nb = rep.blocks(iface_chunk(h));
  int* const cnt = h->buf.iface_work.as<int>();
  double* const part = h->iface_part;
  const IfaceConsts c = {eps, 1.0 - eps, h->cd.nrm_x, h->cd.nrm_y, h->cd.dx, h->cd.dy};
  if (nb)
    launch(h, kOther, k_iface<T, V, EMIT>, dim3(nb), 0, rep.g, (const T*)F_<T>(h, fF), iface_chunk(h), c, cnt, part, h->buf.iface_rows.as<double>(),
           (long long)cap);
  if (!EMIT)
    launch_block(h, kOther, k_iface_scan, dim3(1), (unsigned)kIfaceScanThreads, 0, cnt, (long long)rep.entries(), (const double*)part, (int)nb,
           part + (size_t)nb * kIfacePart, (double)h->istep);
}

// The segments of the field F as vof_get_field would return it now: settle_ghosts first (the 3 x 3 neighbourhood of a cell
// beside a wall holds ghost cells, which a fused step may have left virtual), count + scan, the summary to the host, then --
// the stream is idle again -- room for min(SEGMENTS, cap_rows) rows, the emit pass and the copy of those rows.
int iface_run(vof2d_ctx* h, double eps, double* rows, int64_t cap_rows, double* summary) {
  int rc = iface_prepare(h, 0);
  if (rc) return rc;
  settle_ghosts(h);
  DISPATCH_T(h, (iface_launch<double, false>(h, eps, 0)), (iface_launch<float, false>(h, eps, 0)));
  if ((rc = ensure_ok(h))) return rc;
  if ((rc = read_back(h, summary, h->iface_part + (size_t)reported(h).blocks(iface_chunk(h)) * kIfacePart, IFS_N * sizeof(double)))) return rc;
  int64_t n = (int64_t)summary[IFS_SEGMENTS];
  if (n > cap_rows) n = cap_rows;
  if (n <= 0) return VOF_OK;
  if ((rc = iface_prepare(h, n))) return rc;
  DISPATCH_T(h, (iface_launch<double, true>(h, eps, n)), (iface_launch<float, true>(h, eps, n)));
  if ((rc = ensure_ok(h))) return rc;
  return read_back(h, rows, h->buf.iface_rows.p, (size_t)n * IF_N * sizeof(double));
}

}  // namespace
