// runtime/tracers.h -- vof_tracers_set / _advance / _get and vof_step_tracers: the handle's buffers, the launches of k_tracer_advance,
// k_tracer_sample and k_tracer_finish, the stepping loop that advances the tracers and records snapshots
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "blobs.h"

namespace {

static_assert(TR_N == VOF_TRACER_N && TR_X == VOF_TRACER_X && TR_Y == VOF_TRACER_Y && TR_U == VOF_TRACER_U && TR_V == VOF_TRACER_V && TR_F == VOF_TRACER_F &&
              TRS_N == VOF_TRACER_SUM_N && TRS_COUNT == VOF_TRACER_SUM_COUNT && TRS_LOST == VOF_TRACER_SUM_LOST && TRS_IN_LIQUID == VOF_TRACER_SUM_IN_LIQUID &&
              TRS_ISTEP == VOF_TRACER_SUM_ISTEP && TRS_TIME == VOF_TRACER_SUM_TIME,
              "kernels/tracers.h and include/vof2d.h name the same slots");

constexpr size_t kTracerRowBytes = TR_N * sizeof(double);
constexpr size_t kTracerSumAt = 16;   // byte offset of the summary behind the TRC_N counters in buf.tracer_cnt
static_assert(TRC_N * sizeof(unsigned) <= kTracerSumAt, "the summary sits behind the counters");

inline TracerConsts tracer_consts(const vof2d_ctx* h) { return {h->cd.dxi, h->cd.dyi, h->d.Lx, h->d.Ly}; }
inline dim3 tracer_grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }   // (n <= 2^31 - 1: at most 2^23 blocks)

// Positions as vof_tracers_set checks them: finite and inside the closed domain
inline bool tracer_positions_ok(const vof2d_ctx* h, const double* xy, int64_t n) {
  const double Lx = h->d.Lx, Ly = h->d.Ly;
  for (int64_t k = 0; k < n; ++k) {
    const double x = xy[2 * k], y = xy[2 * k + 1];
    if (!(x >= 0.0 && x <= Lx && y >= 0.0 && y <= Ly)) return false;   // (a NaN fails every comparison)
  }
  return true;
}

// A new set (the entry point has checked the positions): room first -- only a larger set gives the old buffer up, and a
// failure there leaves the handle without tracers, said in the message --, then the copy, waited for: xy is the caller's.
int tracers_set(vof2d_ctx* h, const double* xy, int64_t n) {
  if (n > 0) {
    const size_t bytes = (size_t)n * 2 * sizeof(double);
    if (bytes > h->buf.tracer_pos.bytes) h->tracer_n = 0;
    if (const int rc = h->buf.tracer_pos.reserve(h, bytes, "vof_tracers_set: no memory for the positions (the handle has no tracers now)")) return rc;
    HIPCHK(h, hipMemcpyAsync(h->buf.tracer_pos.p, xy, bytes, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
  }
  h->tracer_n = n;
  h->tracer_time = 0.0;
  return VOF_OK;
}

template <typename T>
void tracer_advance_launch(vof2d_ctx* h, double time) {
  launch(h, kOther, k_tracer_advance<T>, tracer_grid(h->tracer_n), 0, h->g, tracer_consts(h), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), time,
         (long long)h->tracer_n, h->buf.tracer_pos.as<double>());
}
// One advance of every tracer on the u, v vof_get_field would return now: settle_ghosts first (the wall faces and ghost
// cells a fused step left virtual are operands of a sample beside a wall; a k_tm batch may have left the predictor ahead).
// Enqueues only; TIME is the host's sum, in call order.
int tracers_advance(vof2d_ctx* h, double time) {
  h->tracer_time += time;
  if (h->tracer_n == 0) return VOF_OK;   // (nothing to launch; TIME counts all the same)
  settle_ghosts(h);
  DISPATCH_T(h, tracer_advance_launch<double>(h, time), tracer_advance_launch<float>(h, time));
  return ensure_ok(h);
}

// The rows of all tracers at their current positions into `rows` (device; buf.tracer_rows or a snapshot slot); with
// `summary`, the counters are zeroed in front and k_tracer_finish forms the summary behind.  Enqueues only.
template <typename T>
void tracer_sample_launch(vof2d_ctx* h, double* rows, bool summary) {
  unsigned* const cnt = summary ? h->buf.tracer_cnt.as<unsigned>() : nullptr;
  if (summary) (void)hipMemsetAsync(cnt, 0, TRC_N * sizeof(unsigned), h->stream);
  launch(h, kOther, k_tracer_sample<T>, tracer_grid(h->tracer_n), 0, h->g, tracer_consts(h), (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV),
         (long long)h->tracer_n, (const double*)h->buf.tracer_pos.as<double>(), rows, cnt);
  if (summary)
    launch_block(h, kOther, k_tracer_finish, dim3(1), 64u, 0, (const unsigned*)cnt, h->buf.tracer_cnt.as<double>(kTracerSumAt), (double)h->tracer_n, (double)h->istep,
                 h->tracer_time);
}

// vof_tracers_get: room (while nothing of the call is enqueued), settle_ghosts, sample + finish, the copies, one wait
int tracers_get(vof2d_ctx* h, double* rows, int64_t cap_rows, double* summary) {
  const int64_t n = h->tracer_n;
  if (n == 0) {
    for (int k = 0; k < TRS_N; ++k) summary[k] = 0.0;
    summary[TRS_ISTEP] = (double)h->istep;
    summary[TRS_TIME] = h->tracer_time;
    return VOF_OK;
  }
  int rc = h->buf.tracer_cnt.reserve(h, kTracerSumAt + TRS_N * sizeof(double), "vof_tracers_get: no memory for the counters");
  if (rc) return rc;
  if ((rc = h->buf.tracer_rows.reserve(h, (size_t)n * kTracerRowBytes, "vof_tracers_get: no memory for the rows"))) return rc;
  settle_ghosts(h);
  DISPATCH_T(h, tracer_sample_launch<double>(h, h->buf.tracer_rows.as<double>(), true), tracer_sample_launch<float>(h, h->buf.tracer_rows.as<double>(), true));
  if ((rc = ensure_ok(h))) return rc;
  const int64_t out = n < cap_rows ? n : cap_rows;
  if (out > 0) HIPCHK(h, hipMemcpyAsync(rows, h->buf.tracer_rows.p, (size_t)out * kTracerRowBytes, hipMemcpyDeviceToHost, h->stream));
  return read_back(h, summary, h->buf.tracer_cnt.as<double>(kTracerSumAt), TRS_N * sizeof(double));
}

// The snapshots a call of vof_step_tracers owes
inline int64_t tracer_snaps_due(int64_t nsteps, int64_t every, int64_t snap_every) { return snap_every >= 1 ? (nsteps / every) / snap_every : 0; }

// step_groups_n (runtime/step.h) with an advance by every * dt behind every group and a snapshot of all rows behind every
// snap_every-th advance, one read-back at the end
int step_tracers_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, int64_t snap_every, double* snaps, int64_t* snaps_written) {
  const int64_t due = tracer_snaps_due(nsteps, every, snap_every);
  const size_t snap_bytes = (size_t)h->tracer_n * kTracerRowBytes;
  int rc;
  if (due > 0 && snap_bytes > 0 && (rc = h->buf.tracer_snaps.reserve(h, (size_t)due * snap_bytes, "vof_step_tracers: no memory for the snapshots"))) return rc;
  const double span = (double)every * h->cd.dt;
  int64_t taken = 0;
  rc = step_groups_n(h, nsteps, every, cycles, criterion, [&](int64_t r) {
    if (const int rc = tracers_advance(h, span)) return rc;
    if (snap_every < 1 || (r + 1) % snap_every != 0) return VOF_OK;
    if (snap_bytes > 0) {
      double* const slot = h->buf.tracer_snaps.as<double>((size_t)taken * snap_bytes);
      DISPATCH_T(h, tracer_sample_launch<double>(h, slot, false), tracer_sample_launch<float>(h, slot, false));
      if (const int rc = ensure_ok(h)) return rc;
    }
    ++taken;
    return VOF_OK;
  });
  if (rc) return rc;
  if (taken > 0 && snap_bytes > 0 && (rc = read_back(h, snaps, h->buf.tracer_snaps.p, (size_t)taken * snap_bytes))) return rc;
  if (snaps_written) *snaps_written = taken;
  return VOF_OK;
}

}  // namespace
