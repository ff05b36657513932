// runtime/blobs.h -- vof_blobs: the handle's buffers, the launches of the k_blob_* kernels and of k_iface_scan, the copies out
//
// Part of the host-side runtime of libvof2d_hip.so; included (once, in this order) by vof2d_api.hip:
// context.h (with state.h), launches.h, graphs.h, schedule.h, multigrid.h, step.h, diag_reduce.h, interface.h, blobs.h, comm.h, selftest.h.
// Everything here has internal linkage.
#pragma once
#include "interface.h"

namespace {

static_assert(BL_N == VOF_BLOB_N && BL_SUM_WV == VOF_BLOB_SUM_WV && BL_JMAX == VOF_BLOB_JMAX && BLS_N == VOF_BLOB_SUM_N && BLS_ISTEP == VOF_BLOB_SUM_ISTEP,
              "kernels/blobs.h and include/vof2d.h name the same slots");

inline int64_t blob_cells(const vof2d_ctx* h) {
  int lo, hi;
  diag_rows_of(h, lo, hi);
  return hi < lo ? 0 : (int64_t)(hi - lo + 1) * h->g.ny;
}

// a device buffer of the handle grown to `want` elements (the old contents are given up)
template <typename T>
int blob_grow(vof2d_ctx* h, T*& p, int64_t& cap, int64_t want, size_t per) {
  if (cap >= want) return VOF_OK;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  if (hipMalloc(reinterpret_cast<void**>(&p), (size_t)want * per * sizeof(T)) != hipSuccess) {
    (void)hipGetLastError();
    p = nullptr;
    return fail(h, VOF_ENOMEM, "vof_blobs: no memory for its work buffers");
  }
  cap = want;
  return VOF_OK;
}

// The buffers the geometry fixes (once): parent / labels and the roots' indices (one int per owned cell each), the root
// counts per (row, tile), two ints of k_blob_stats, and behind them 8 doubles: the summary, the total of a scan.  Called while nothing of the call is enqueued.
int blobs_prepare(vof2d_ctx* h) {
  if (h->blob_lab) return VOF_OK;
  const size_t n = (size_t)blob_cells(h);
  const size_t ints = (2 * n + (size_t)iface_entries(h) + 4) & ~(size_t)1;   // (the doubles behind them stay 8-byte aligned)
  char* p = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&p), ints * sizeof(int) + 8 * sizeof(double)) != hipSuccess) {
    (void)hipGetLastError();
    return fail(h, VOF_ENOMEM, "vof_blobs: no memory for the labels");
  }
  h->blob_lab = reinterpret_cast<int*>(p);
  h->blob_idx = h->blob_lab + n;
  h->blob_cnt = h->blob_idx + n;
  h->blob_sum = reinterpret_cast<double*>(p + ints * sizeof(int));
  return VOF_OK;
}
void blobs_release(vof2d_ctx* h) {
  if (h->blob_lab) (void)hipFree(h->blob_lab);
  if (h->blob_rec) (void)hipFree(h->blob_rec);
  if (h->blob_off) (void)hipFree(h->blob_off);
  if (h->blob_rows) (void)hipFree(h->blob_rows);
  if (h->blob_part) (void)hipFree(h->blob_part);
  h->blob_lab = h->blob_idx = h->blob_cnt = h->blob_rec = h->blob_off = nullptr;
  h->blob_sum = h->blob_rows = h->blob_part = nullptr;
  h->blob_rec_cap = h->blob_off_cap = h->blob_rows_cap = h->blob_part_cap = 0;
}

inline Geom blob_geom(const vof2d_ctx* h) {
  Geom g = h->g;
  diag_rows_of(h, g.ilo, g.ihi);   // (cg_tile cuts [g.ilo, g.ihi] into chunks)
  return g;
}
// k_iface_scan on n counts: exclusive offsets in place, the total into blob_sum[4]
inline void blob_scan(vof2d_ctx* h, int* cnt, int64_t n) {
  launch_block(h, kOther, k_iface_scan, dim3(1), (unsigned)kIfaceScanThreads, 0, cnt, (long long)n, (const double*)h->blob_sum, 0, h->blob_sum + 4, 0.0);
}

template <typename T>
void blob_label_launch(vof2d_ctx* h, int phase, double thr) {
  constexpr int V = VecWidth<T>::V;
  const Geom g = blob_geom(h);
  const int R = iface_chunk(h);
  const dim3 nb(iface_blocks(h));
  launch(h, kOther, k_blob_init<T, V>, nb, 0, g, (const T*)F_<T>(h, fF), R, phase, thr, h->blob_lab);
  launch(h, kOther, k_blob_merge<T, V>, nb, 0, g, (const T*)F_<T>(h, fF), R, phase, thr, h->blob_lab);
  launch(h, kOther, k_blob_flatten<V>, nb, 0, g, R, h->blob_lab, h->blob_cnt);
  blob_scan(h, h->blob_cnt, iface_entries(h));
}
template <typename T>
void blob_number_launch(vof2d_ctx* h, int64_t nblobs) {
  constexpr int V = VecWidth<T>::V;
  const Geom g = blob_geom(h);
  const int R = iface_chunk(h);
  const dim3 nb(iface_blocks(h));
  launch(h, kOther, k_blob_number<V>, nb, 0, g, R, (const int*)h->blob_lab, (const int*)h->blob_cnt, h->blob_idx, h->blob_rec);
  launch(h, kOther, k_blob_label<V>, nb, 0, g, R, h->blob_lab, (const int*)h->blob_idx, h->blob_rec);
  int* stat = h->blob_cnt + iface_entries(h);
  (void)hipMemsetAsync(stat, 0, 2 * sizeof(int), h->stream);
  if (nblobs > 0)
    launch(h, kOther, k_blob_stats, dim3((unsigned)((nblobs + 256 * kBlobStatPer - 1) / (256 * kBlobStatPer))), 0, (const int*)h->blob_rec, (long long)nblobs, stat);
  launch_block(h, kOther, k_blob_summary, dim3(1), 64u, 0, (const int*)stat, (long long)nblobs, h->blob_sum, (double)h->istep);
}
template <typename T>
void blob_plan_launch(vof2d_ctx* h, int nsel) {
  constexpr int V = VecWidth<T>::V;
  launch(h, kOther, k_blob_plan<V>, dim3((unsigned)(nsel / 256 + 1)), 0, (const int*)h->blob_rec, nsel, h->blob_off);
  blob_scan(h, h->blob_off, (int64_t)nsel + 1);
}
template <typename T>
void blob_sums_launch(vof2d_ctx* h, int nsel, int64_t waves, int phase) {
  constexpr int V = VecWidth<T>::V;
  const Geom g = blob_geom(h);
  launch(h, kOther, k_blob_sums<T, V>, dim3((unsigned)((waves + 3) / 4)), 0, g, (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV),
         (const int*)h->blob_lab, (const int*)h->blob_rec, (const int*)h->blob_off, nsel, phase, h->blob_part);
  launch(h, kOther, k_blob_rows, dim3((unsigned)((nsel + 3) / 4)), 0, (const int*)h->blob_rec, (const int*)h->blob_off, nsel, (const double*)h->blob_part, g.ilo,
         g.ny, h->blob_rows);
}

// The blobs of the fields as vof_get_field would return them now: settle_ghosts first (u[1,j], u[nx+1,j] may be virtual after a
// fused step), labelling and the root count; the host reads BLOBS and makes room for the records; numbering, labels, records,
// summary and the plan of the sum pass; the host reads the summary and the number of waves and makes room for the partials; the
// sums, the rows, the copies.
int blobs_run(vof2d_ctx* h, int phase, double thr, double* rows, int64_t cap_rows, int32_t* labels, double* summary) {
  const int64_t n = blob_cells(h);
  if (n == 0) {
    summary[BLS_BLOBS] = summary[BLS_MEMBER_CELLS] = summary[BLS_MAX_CELLS] = 0.0;
    summary[BLS_ISTEP] = (double)h->istep;
    return VOF_OK;
  }
  int rc = blobs_prepare(h);
  if (rc) return rc;
  settle_ghosts(h);
  DISPATCH_T(h, blob_label_launch<double>(h, phase, thr), blob_label_launch<float>(h, phase, thr));
  if ((rc = ensure_ok(h))) return rc;
  double host[8];
  HIPCHK(h, hipMemcpyAsync(host + 4, h->blob_sum + 4, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const int64_t nblobs = (int64_t)host[4];
  if ((rc = blob_grow(h, h->blob_rec, h->blob_rec_cap, nblobs > 0 ? nblobs : 1, kBlobRec))) return rc;
  DISPATCH_T(h, blob_number_launch<double>(h, nblobs), blob_number_launch<float>(h, nblobs));
  const int nsel = (int)(nblobs < cap_rows ? nblobs : cap_rows);
  if (nsel > 0) {
    if ((rc = blob_grow(h, h->blob_off, h->blob_off_cap, (int64_t)nsel + 1, 1))) return rc;
    if ((rc = blob_grow(h, h->blob_rows, h->blob_rows_cap, nsel, BL_N))) return rc;
    DISPATCH_T(h, blob_plan_launch<double>(h, nsel), blob_plan_launch<float>(h, nsel));
  }
  if ((rc = ensure_ok(h))) return rc;
  HIPCHK(h, hipMemcpyAsync(host, h->blob_sum, 5 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (nsel > 0) {
    const int64_t waves = (int64_t)host[4];
    if (waves > (int64_t)INT32_MAX) return fail(h, VOF_ENOMEM, "vof_blobs: the boxes of the blobs asked for add up to more than 2^31 - 1 waves; ask for fewer rows");
    if ((rc = blob_grow(h, h->blob_part, h->blob_part_cap, waves, kBlobSums))) return rc;
    DISPATCH_T(h, blob_sums_launch<double>(h, nsel, waves, phase), blob_sums_launch<float>(h, nsel, waves, phase));
    if ((rc = ensure_ok(h))) return rc;
    HIPCHK(h, hipMemcpyAsync(rows, h->blob_rows, (size_t)nsel * BL_N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (labels) HIPCHK(h, hipMemcpyAsync(labels, h->blob_lab, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < BLS_N; ++k) summary[k] = host[k];
  return VOF_OK;
}

}  // namespace
