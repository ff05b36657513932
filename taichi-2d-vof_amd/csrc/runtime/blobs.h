// runtime/blobs.h -- vof_blobs: the handle's buffers, the launches of the k_blob_* kernels and of the scan of kernels/cell_rows.h, the copies out
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "cell_rows.h"

namespace {

static_assert(BL_N == VOF_BLOB_N && BL_SUM_WV == VOF_BLOB_SUM_WV && BL_JMAX == VOF_BLOB_JMAX && BLS_N == VOF_BLOB_SUM_N && BLS_ISTEP == VOF_BLOB_SUM_ISTEP,
              "kernels/blobs.h and include/vof2d.h name the same slots");

// The buffer the geometry fixes (once; BlobCarve, runtime/carve.h).  Called while nothing of the call is enqueued.
int blobs_prepare(vof2d_ctx* h) {
  const Reported rep = reported(h);
  const BlobCarve c = carve_blobs((size_t)rep.cells(), (size_t)rep.entries());
  DevBuf& w = h->buf.blob_work;
  if (const int rc = w.reserve(h, c.total, "vof_blobs: no memory for the labels")) return rc;
  h->blob_idx = w.as<int>(c.idx);
  h->blob_cnt = w.as<int>(c.cnt);
  h->blob_sum = w.as<double>(c.sum);
  return VOF_OK;
}
constexpr const char* kBlobNoMem = "vof_blobs: no memory for its work buffers";   // (the buffers grown on demand)

// the scan of kernels/cell_rows.h (vof_interface's, without partials) on n counts: exclusive offsets in place, the total into blob_sum[4]
inline void blob_scan(vof2d_ctx* h, int* cnt, int64_t n) {
  launch_block(h, kOther, k_cell_rows_scan<IfaceVerb>, dim3(1), (unsigned)kScanThreads, 0, cnt, (long long)n, (const double*)h->blob_sum, 0, h->blob_sum + 4, 0.0);
}

template <typename T>
void blob_label_launch(vof2d_ctx* h, int phase, double thr) {
  constexpr int V = VecWidth<T>::V;
  const Reported rep = reported(h);
  const Geom& g = rep.g;
  const int R = cell_rows_chunk(h);
  const dim3 nb(rep.blocks(R));
  int* const lab = h->buf.blob_work.as<int>();
  launch(h, kOther, k_blob_init<T, V>, nb, 0, g, (const T*)F_<T>(h, fF), R, phase, thr, lab);
  launch(h, kOther, k_blob_merge<T, V>, nb, 0, g, (const T*)F_<T>(h, fF), R, phase, thr, lab);
  launch(h, kOther, k_blob_flatten<V>, nb, 0, g, R, lab, h->blob_cnt);
  blob_scan(h, h->blob_cnt, rep.entries());
}
template <typename T>
void blob_number_launch(vof2d_ctx* h, int64_t nblobs) {
  constexpr int V = VecWidth<T>::V;
  const Reported rep = reported(h);
  const Geom& g = rep.g;
  const int R = cell_rows_chunk(h);
  const dim3 nb(rep.blocks(R));
  int* const lab = h->buf.blob_work.as<int>();
  int* const rec = h->buf.blob_rec.as<int>();
  launch(h, kOther, k_blob_number<V>, nb, 0, g, R, (const int*)lab, (const int*)h->blob_cnt, h->blob_idx, rec);
  launch(h, kOther, k_blob_label<V>, nb, 0, g, R, lab, (const int*)h->blob_idx, rec);
  int* stat = h->blob_cnt + rep.entries();
  (void)hipMemsetAsync(stat, 0, 2 * sizeof(int), h->stream);
  if (nblobs > 0)
    launch(h, kOther, k_blob_stats, dim3((unsigned)((nblobs + 256 * kBlobStatPer - 1) / (256 * kBlobStatPer))), 0, (const int*)rec, (long long)nblobs, stat);
  launch_block(h, kOther, k_blob_summary, dim3(1), 64u, 0, (const int*)stat, (long long)nblobs, h->blob_sum, (double)h->istep);
}
template <typename T>
void blob_plan_launch(vof2d_ctx* h, int nsel) {
  constexpr int V = VecWidth<T>::V;
  int* const off = h->buf.blob_off.as<int>();
  launch(h, kOther, k_blob_plan<V>, dim3((unsigned)(nsel / 256 + 1)), 0, h->buf.blob_rec.as<const int>(), nsel, off);
  blob_scan(h, off, (int64_t)nsel + 1);
}
template <typename T>
void blob_sums_launch(vof2d_ctx* h, int nsel, int64_t waves, int phase) {
  constexpr int V = VecWidth<T>::V;
  const Geom g = reported(h).g;
  const WorkBufs& b = h->buf;
  launch(h, kOther, k_blob_sums<T, V>, dim3((unsigned)((waves + 3) / 4)), 0, g, (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV),
         b.blob_work.as<const int>(), b.blob_rec.as<const int>(), b.blob_off.as<const int>(), nsel, phase, b.blob_part.as<double>());
  launch(h, kOther, k_blob_rows, dim3((unsigned)((nsel + 3) / 4)), 0, b.blob_rec.as<const int>(), b.blob_off.as<const int>(), nsel, b.blob_part.as<const double>(), g.ilo,
         g.ny, b.blob_rows.as<double>());
}

// The blobs of the fields as vof_get_field would return them now: settle_ghosts first (u[1,j], u[nx+1,j] may be virtual after a
// fused step), labelling and the root count; the host reads BLOBS and makes room for the records; numbering, labels, records,
// summary and the plan of the sum pass; the host reads the summary and the number of waves and makes room for the partials; the
// sums, the rows, the copies.
int blobs_run(vof2d_ctx* h, int phase, double thr, double* rows, int64_t cap_rows, int32_t* labels, double* summary) {
  const int64_t n = reported(h).cells();
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
  if ((rc = read_back(h, host + 4, h->blob_sum + 4, sizeof(double)))) return rc;
  const int64_t nblobs = (int64_t)host[4];
  if ((rc = h->buf.blob_rec.reserve(h, (size_t)(nblobs > 0 ? nblobs : 1) * kBlobRec * sizeof(int), kBlobNoMem))) return rc;
  DISPATCH_T(h, blob_number_launch<double>(h, nblobs), blob_number_launch<float>(h, nblobs));
  const int nsel = (int)(nblobs < cap_rows ? nblobs : cap_rows);
  if (nsel > 0) {
    if ((rc = h->buf.blob_off.reserve(h, ((size_t)nsel + 1) * sizeof(int), kBlobNoMem))) return rc;
    if ((rc = h->buf.blob_rows.reserve(h, (size_t)nsel * BL_N * sizeof(double), kBlobNoMem))) return rc;
    DISPATCH_T(h, blob_plan_launch<double>(h, nsel), blob_plan_launch<float>(h, nsel));
  }
  if ((rc = ensure_ok(h)) || (rc = read_back(h, host, h->blob_sum, 5 * sizeof(double)))) return rc;
  if (nsel > 0) {
    const int64_t waves = (int64_t)host[4];
    if (waves > (int64_t)INT32_MAX) return fail(h, VOF_ENOMEM, "vof_blobs: the boxes of the blobs asked for add up to more than 2^31 - 1 waves; ask for fewer rows");
    if ((rc = h->buf.blob_part.reserve(h, (size_t)waves * kBlobSums * sizeof(double), kBlobNoMem))) return rc;
    DISPATCH_T(h, blob_sums_launch<double>(h, nsel, waves, phase), blob_sums_launch<float>(h, nsel, waves, phase));
    if ((rc = ensure_ok(h))) return rc;
    HIPCHK(h, hipMemcpyAsync(rows, h->buf.blob_rows.p, (size_t)nsel * BL_N * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  }
  if (labels) HIPCHK(h, hipMemcpyAsync(labels, h->buf.blob_work.p, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < BLS_N; ++k) summary[k] = host[k];
  return VOF_OK;
}

}  // namespace
