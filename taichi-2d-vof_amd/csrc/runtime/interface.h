// runtime/interface.h -- vof_interface: the handle's buffers, the launches of k_iface (count), k_iface_scan, k_iface (emit), the copies out
//
// Part of the host-side runtime of libvof2d_hip.so; included (once, in this order) by vof2d_api.hip:
// context.h (with state.h), launches.h, graphs.h, schedule.h, multigrid.h, step.h, diag_reduce.h, interface.h, comm.h, selftest.h.  Everything
// here has internal linkage.
#pragma once
#include "diag_reduce.h"

namespace {

static_assert(IF_N == VOF_IFACE_N && IF_NY == VOF_IFACE_NY && IFS_N == VOF_IFACE_SUM_N && IFS_ISTEP == VOF_IFACE_SUM_ISTEP,
              "kernels/interface.h and include/vof2d.h name the same slots");

// rows per wave chunk: the cells-per-wave rule (every chunk re-reads two rows of F; the chunk length fixes the order of the
// LENGTH sum, so it depends on the geometry alone)
inline int iface_chunk(const vof2d_ctx* h) { return chunk_rows(h, h->g.ntj, 4, 32); }
inline unsigned iface_blocks(const vof2d_ctx* h) {
  int lo, hi;
  diag_rows_of(h, lo, hi);
  return hi < lo ? 0u : blocks_rows(hi - lo + 1, h->g.ntj, iface_chunk(h));
}
inline int64_t iface_entries(const vof2d_ctx* h) {
  int lo, hi;
  diag_rows_of(h, lo, hi);
  return hi < lo ? 0 : (int64_t)(hi - lo + 1) * h->g.ntj;
}

// The work buffer (once: the counts / offsets, the block partials, the summary) and room for `rows` segments on the device
// (grown on demand).  Called while nothing of the call is enqueued.
int iface_prepare(vof2d_ctx* h, int64_t rows) {
  if (!h->iface_cnt) {
    const size_t ints = ((size_t)iface_entries(h) + 2) & ~(size_t)1;   // (the doubles behind them stay 8-byte aligned)
    const size_t dbl = (size_t)iface_blocks(h) * kIfacePart + IFS_N;
    char* p = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&p), ints * sizeof(int) + dbl * sizeof(double)) != hipSuccess) {
      (void)hipGetLastError();
      return fail(h, VOF_ENOMEM, "vof_interface: no memory for the counts");
    }
    h->iface_cnt = reinterpret_cast<int*>(p);
    h->iface_part = reinterpret_cast<double*>(p + ints * sizeof(int));
  }
  if (h->iface_cap >= rows) return VOF_OK;
  if (h->iface_rows) {
    (void)hipFree(h->iface_rows);
    h->iface_rows = nullptr;
    h->iface_cap = 0;
  }
  if (hipMalloc(reinterpret_cast<void**>(&h->iface_rows), (size_t)rows * IF_N * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    h->iface_rows = nullptr;
    return fail(h, VOF_ENOMEM, "vof_interface: no memory for the segments");
  }
  h->iface_cap = rows;
  return VOF_OK;
}
void iface_release(vof2d_ctx* h) {
  if (h->iface_cnt) (void)hipFree(h->iface_cnt);
  if (h->iface_rows) (void)hipFree(h->iface_rows);
  h->iface_cnt = nullptr;
  h->iface_part = h->iface_rows = nullptr;
  h->iface_cap = 0;
}

template <typename T, bool EMIT>
void iface_launch(vof2d_ctx* h, double eps, int64_t cap) {
  constexpr int V = VecWidth<T>::V;
  int lo, hi;
  diag_rows_of(h, lo, hi);
  const unsigned nb = iface_blocks(h);
  Geom g = h->g;
  g.ilo = lo; g.ihi = hi;   // (cg_tile cuts [g.ilo, g.ihi] into chunks)
  const IfaceConsts c = {eps, 1.0 - eps, h->cd.nrm_x, h->cd.nrm_y, h->cd.dx, h->cd.dy};
  if (nb)
    launch(h, kOther, k_iface<T, V, EMIT>, dim3(nb), 0, g, (const T*)F_<T>(h, fF), iface_chunk(h), c, h->iface_cnt, h->iface_part, h->iface_rows,
           (long long)cap);
  if (!EMIT)
    launch_block(h, kOther, k_iface_scan, dim3(1), (unsigned)kIfaceScanThreads, 0, h->iface_cnt, (long long)iface_entries(h), (const double*)h->iface_part, (int)nb,
           h->iface_part + (size_t)nb * kIfacePart, (double)h->istep);
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
  HIPCHK(h, hipMemcpyAsync(summary, h->iface_part + (size_t)iface_blocks(h) * kIfacePart, IFS_N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  int64_t n = (int64_t)summary[IFS_SEGMENTS];
  if (n > cap_rows) n = cap_rows;
  if (n <= 0) return VOF_OK;
  if ((rc = iface_prepare(h, n))) return rc;
  DISPATCH_T(h, (iface_launch<double, true>(h, eps, n)), (iface_launch<float, true>(h, eps, n)));
  if ((rc = ensure_ok(h))) return rc;
  HIPCHK(h, hipMemcpyAsync(rows, h->iface_rows, (size_t)n * IF_N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VOF_OK;
}

}  // namespace
