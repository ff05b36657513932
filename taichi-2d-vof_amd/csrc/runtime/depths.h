// runtime/depths.h -- vof_depths, vof_gauges_set / _get and vof_step_gauges: the handle's buffers, the launches of k_depths,
// k_depths_fold, k_depths_finish and k_gauge_sample, the stepping loop that records the gauges
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "tracers.h"

namespace {

static_assert(DPS_N == VOF_DEPTH_SUM_N && DPS_ROWS == VOF_DEPTH_SUM_ROWS && DPS_ISTEP == VOF_DEPTH_SUM_ISTEP && DPS_FRONT_LO == VOF_DEPTH_SUM_FRONT_LO &&
              DPS_FRONT_HI == VOF_DEPTH_SUM_FRONT_HI && DPS_TOP_J == VOF_DEPTH_SUM_TOP_J && DPS_SUM == VOF_DEPTH_SUM_SUM && GA_N == VOF_GAUGE_N &&
              GA_X == VOF_GAUGE_X && GA_Y == VOF_GAUGE_Y && GA_U == VOF_GAUGE_U && GA_V == VOF_GAUGE_V && GA_F == VOF_GAUGE_F && GA_P == VOF_GAUGE_P &&
              GA_DEPTH == VOF_GAUGE_DEPTH && GA_TOP == VOF_GAUGE_TOP && GAS_N == VOF_GAUGE_SUM_N && GAS_COUNT == VOF_GAUGE_SUM_COUNT &&
              GAS_ISTEP == VOF_GAUGE_SUM_ISTEP && GAS_RECORDS == VOF_GAUGE_SUM_RECORDS,
              "kernels/depths.h and include/vof2d.h name the same slots");

constexpr size_t kGaugeRowBytes = GA_N * sizeof(double);

// What a pass on the handle's reported rows launches and where its results lie in buf.depths_work
struct DepthsPlan { Reported rep; DepthsGeom dg; DepthsCarve at; };
inline DepthsPlan depths_plan(const vof2d_ctx* h) {
  const Reported rep = reported(h);
  const DepthsGeom dg = depths_geom(rep, depths_chunk_rows(h->d.row_lo, h->d.row_hi, h->d.nx, h->g.ntj));
  return {rep, dg, carve_depths((size_t)rep.rows(), (size_t)rep.ny, (size_t)dg.row_partials, (size_t)dg.col_partials)};
}
// Room for the pass (the geometry fixes it: allocated by the first call) and, for vof_depths, for its results on the host.
// Called before anything of the call is enqueued.
int depths_prepare(vof2d_ctx* h) { return h->buf.depths_work.reserve(h, depths_plan(h).at.total, "vof_depths: no memory for the partials"); }
int depths_prepare_host(vof2d_ctx* h, size_t bytes) {
  if (h->h_depths_bytes >= bytes) return VOF_OK;
  if (h->h_depths) (void)hipHostFree(h->h_depths);
  h->h_depths = nullptr;
  h->h_depths_bytes = 0;
  if (hipHostMalloc(reinterpret_cast<void**>(&h->h_depths), bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    h->h_depths = nullptr;
    return fail(h, VOF_ENOMEM, "vof_depths: no pinned host memory for the results");
  }
  h->h_depths_bytes = bytes;
  return VOF_OK;
}

// One pass over the current view of F: the words zeroed, k_depths, the fold, the summary.  Enqueues only.
template <typename T>
int depths_launch(vof2d_ctx* h) {
  constexpr int V = VecWidth<T>::V;
  const DepthsPlan pl = depths_plan(h);
  const DevBuf& w = h->buf.depths_work;
  int* const top = w.as<int>(pl.at.top);
  HIPCHK(h, hipMemsetAsync(top, 0, pl.at.top_bytes, h->stream));
  if (pl.dg.blocks)
    launch(h, kOther, k_depths<T, V>, dim3(pl.dg.blocks), 0, pl.rep.g, (const T*)F_<T>(h, fF), pl.dg.R, w.as<double>(pl.at.rowpart), w.as<double>(pl.at.colpart), top);
  launch(h, kOther, k_depths_fold, dim3(pl.dg.row_blocks + pl.dg.col_blocks), 0, (const double*)w.as<double>(pl.at.rowpart), (const double*)w.as<double>(pl.at.colpart),
         pl.rep.rows(), pl.rep.ntj, pl.dg.chunks, pl.rep.ny, (int)pl.dg.row_blocks, w.as<double>(pl.at.depth_i), w.as<double>(pl.at.depth_j));
  launch_block(h, kOther, k_depths_finish, dim3(1), 64u, 0, (const double*)w.as<double>(pl.at.depth_i), (const int*)top, pl.rep.rows(), w.as<double>(pl.at.sum),
               (double)h->istep);
  return VOF_OK;
}
// ... of the fields as vof_get_field would return them now: settle_ghosts first, like the other readers (a k_tm batch may
// have left the predictor ahead; F itself is final, the call leaves the state as vof_get_field would)
int depths_enqueue(vof2d_ctx* h) {
  settle_ghosts(h);
  int rc;
  DISPATCH_T(h, rc = depths_launch<double>(h), rc = depths_launch<float>(h));
  return rc ? rc : ensure_ok(h);
}

// vof_depths: room, the pass, ONE copy of the results (depth_i, depth_j, the summary, top: consecutive in the arena) into the
// handle's pinned host buffer, one wait; then what was asked for goes to the caller's arrays.  The entry point has checked the
// arguments.  (Four copies into the caller's pageable arrays cost four trips through the runtime's staging path.)
int depths_run(vof2d_ctx* h, double* depth_i, double* depth_j, int32_t* top, double* summary) {
  const DepthsPlan pl = depths_plan(h);
  const size_t rows = (size_t)pl.rep.rows(), first = pl.at.depth_i, bytes = pl.at.total - first;
  int rc = depths_prepare(h);
  if (rc) return rc;
  if ((rc = depths_prepare_host(h, bytes))) return rc;
  if ((rc = depths_enqueue(h))) return rc;
  if ((rc = read_back(h, h->h_depths, h->buf.depths_work.as<char>(first), bytes))) return rc;
  const char* const res = h->h_depths;   // (the arena from `first` on)
  if (depth_i && rows) memcpy(depth_i, res + (pl.at.depth_i - first), rows * sizeof(double));
  if (depth_j) memcpy(depth_j, res + (pl.at.depth_j - first), (size_t)pl.rep.ny * sizeof(double));
  if (top && rows) memcpy(top, res + (pl.at.top - first), rows * sizeof(int32_t));
  memcpy(summary, res + (pl.at.sum - first), DPS_N * sizeof(double));
  return VOF_OK;
}

// ---- the gauges
// A new set (the entry point has checked the positions, as vof_tracers_set does): room first -- only a larger set gives the old
// buffer up, and a failure there leaves the handle without gauges, said in the message --, then the copy, waited for: xy is the caller's.
int gauges_set(vof2d_ctx* h, const double* xy, int64_t n) {
  if (n > 0) {
    const size_t bytes = (size_t)n * 2 * sizeof(double);
    if (bytes > h->buf.gauge_pos.bytes) h->gauge_n = 0;
    if (const int rc = h->buf.gauge_pos.reserve(h, bytes, "vof_gauges_set: no memory for the positions (the handle has no gauges now)")) return rc;
    HIPCHK(h, hipMemcpyAsync(h->buf.gauge_pos.p, xy, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  h->gauge_n = n;
  h->gauge_records = 0;
  return VOF_OK;
}

template <typename T>
void gauge_sample_launch(vof2d_ctx* h, double* rows) {
  const DepthsPlan pl = depths_plan(h);
  const DevBuf& w = h->buf.depths_work;
  launch(h, kOther, k_gauge_sample<T>, tracer_grid(h->gauge_n), 0, h->g, tracer_consts(h), (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV),
         (const T*)F_<T>(h, fP), (long long)h->gauge_n, (const double*)h->buf.gauge_pos.as<double>(), (const double*)w.as<double>(pl.at.depth_i),
         (const int*)w.as<int>(pl.at.top), pl.rep.range.first, h->cd.dy, rows);
}
// One record of every gauge into `rows` (device; buf.gauge_rows or a slot of buf.gauge_recs) on the fields vof_get_field
// would return now: the vof_depths pass, then the samples.  gauge_n > 0; the buffers are there.  Enqueues only.
int gauges_record(vof2d_ctx* h, double* rows) {
  if (const int rc = depths_enqueue(h)) return rc;
  DISPATCH_T(h, gauge_sample_launch<double>(h, rows), gauge_sample_launch<float>(h, rows));
  return ensure_ok(h);
}

// vof_gauges_get: room (while nothing of the call is enqueued), one record, the copy, one wait.  The summary is the host's.
int gauges_get(vof2d_ctx* h, double* rows, int64_t cap_rows, double* summary) {
  const int64_t n = h->gauge_n;
  if (n > 0) {
    int rc = depths_prepare(h);
    if (rc) return rc;
    if ((rc = h->buf.gauge_rows.reserve(h, (size_t)n * kGaugeRowBytes, "vof_gauges_get: no memory for the rows"))) return rc;
    if ((rc = gauges_record(h, h->buf.gauge_rows.as<double>()))) return rc;
    const int64_t out = n < cap_rows ? n : cap_rows;
    if (out > 0) HIPCHK(h, hipMemcpyAsync(rows, h->buf.gauge_rows.p, (size_t)out * kGaugeRowBytes, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  } else {
    settle_ghosts(h);   // (the call leaves the handle as it does with gauges)
    if (const int rc = ensure_ok(h)) return rc;
  }
  for (int k = 0; k < GAS_N; ++k) summary[k] = 0.0;
  summary[GAS_COUNT] = (double)n;
  summary[GAS_ISTEP] = (double)h->istep;
  summary[GAS_RECORDS] = (double)h->gauge_records;
  return VOF_OK;
}

// step_groups_n (runtime/step.h) with a record of all gauges behind every group, one read-back at the end.  (The entry point
// has checked that the handle has gauges where a record is due.)
int step_gauges_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, double* out, int64_t* records_written) {
  const int64_t records = nsteps / every;
  const size_t rec_bytes = (size_t)h->gauge_n * kGaugeRowBytes;
  int rc;
  if (records > 0) {
    if ((rc = depths_prepare(h))) return rc;
    if ((rc = h->buf.gauge_recs.reserve(h, (size_t)records * rec_bytes, "vof_step_gauges: no memory for the records"))) return rc;
  }
  if ((rc = step_groups_n(h, nsteps, every, cycles, criterion, [&](int64_t r) { return gauges_record(h, h->buf.gauge_recs.as<double>((size_t)r * rec_bytes)); })))
    return rc;
  if (records > 0 && (rc = read_back(h, out, h->buf.gauge_recs.p, (size_t)records * rec_bytes))) return rc;
  h->gauge_records += records;
  if (records_written) *records_written = records;
  return VOF_OK;
}

}  // namespace
