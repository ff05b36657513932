// runtime/stats.h -- vof_stats_begin / _sample / _get / _summary and vof_step_stats: the handle's accumulator planes, the launches of
// k_stats, k_stats_fill, k_stats_summary and k_row_finish, the stepping loop that takes a sample behind every group of steps
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "frames.h"

namespace {

static_assert(ST_PLANES == VOF_STATS_PLANES && ST_PLANES == kStatsPlanes && kStatsMoments == kStatsMomentPlanes && ST_SUM_F == VOF_STATS_SUM_F &&
              ST_SUM_F2 == VOF_STATS_SUM_F2 && ST_SUM_U == VOF_STATS_SUM_U && ST_SUM_V == VOF_STATS_SUM_V && ST_SUM_UU == VOF_STATS_SUM_UU &&
              ST_SUM_VV == VOF_STATS_SUM_VV && ST_SUM_UV == VOF_STATS_SUM_UV && ST_SUM_FU == VOF_STATS_SUM_FU && ST_SUM_FV == VOF_STATS_SUM_FV &&
              ST_MAX_F == VOF_STATS_MAX_F && ST_MAX_SPEED2 == VOF_STATS_MAX_SPEED2 && ST_WET == VOF_STATS_WET && ST_ARRIVAL == VOF_STATS_ARRIVAL &&
              STM_MOMENTS == VOF_STATS_MOMENTS && STM_ENVELOPE == VOF_STATS_ENVELOPE && STS_N == VOF_STATS_SUM_N && STS_SAMPLES == VOF_STATS_SUM_SAMPLES &&
              STS_ISTEP_FIRST == VOF_STATS_SUM_ISTEP_FIRST && STS_ISTEP_LAST == VOF_STATS_SUM_ISTEP_LAST && STS_MASK == VOF_STATS_SUM_MASK &&
              STS_LEVEL == VOF_STATS_SUM_LEVEL && STS_CELLS == VOF_STATS_SUM_CELLS && STS_EVER_WET == VOF_STATS_SUM_EVER_WET &&
              STS_MAX_SPEED2 == VOF_STATS_SUM_MAX_SPEED2,
              "kernels/stats.h, runtime/carve.h and include/vof2d.h name the same slots");

// What a launch on a whole-domain handle gets and where the planes of `mask` lie in buf.stats
struct StatsPlan { Reported rep; int R; unsigned blocks; size_t pitch; StatsCarve at; };
inline StatsPlan stats_plan(const vof2d_ctx* h, int mask) {
  const Reported rep = reported(h);
  const int R = h->stats_chunk > 0 ? h->stats_chunk : diag_chunk(h);
  const unsigned blocks = rep.blocks(diag_chunk(h));   // (of the summary: the chunks of k_diag)
  const size_t pitch = stats_pitch((size_t)h->g.ny, (size_t)64 * h->V);
  return {rep, R, blocks, pitch, carve_stats((size_t)h->d.nx, pitch, mask, (size_t)blocks * kStatsPart + 1)};
}
inline StatsPlanes stats_planes(const vof2d_ctx* h, const StatsPlan& pl) {
  StatsPlanes p;
  for (int k = 0; k < ST_PLANES; ++k) p.p[k] = pl.at.plane[k] == kNoRange ? nullptr : h->buf.stats.as<double>(pl.at.plane[k]);
  p.pitch = (long long)pl.pitch;
  return p;
}

// vof_stats_begin (the entry point has checked the arguments): room -- a failure there leaves the handle without statistics, said in
// the message --, every plane 0, ARRIVAL -1, the counts back to none.  mask == 0: the handle gives the statistics up.
int stats_begin(vof2d_ctx* h, int mask, double level) {
  if (mask == 0) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->buf.stats.release();
    h->stats_mask = 0;
    return VOF_OK;
  }
  const StatsPlan pl = stats_plan(h, mask);
  if (pl.at.total > h->buf.stats.bytes) h->stats_mask = 0;
  if (const int rc = h->buf.stats.reserve(h, pl.at.total, "vof_stats_begin: no memory for the planes (the handle has no statistics now)")) return rc;
  HIPCHK(h, hipMemsetAsync(h->buf.stats.p, 0, pl.at.planes_total, h->stream));
  if (mask & STM_ENVELOPE) {
    const long long n = (long long)(pl.at.plane_bytes / sizeof(double));
    const long long nb = (n + 255) / 256;
    launch(h, kOther, k_stats_fill, dim3((unsigned)(nb < 4096 ? nb : 4096)), 0, h->buf.stats.as<double>(pl.at.plane[ST_ARRIVAL]), n, -1.0);
  }
  h->stats_mask = mask;
  h->stats_level = level;
  h->stats_samples = 0;
  h->stats_first = h->stats_last = 0;
  return ensure_ok(h);
}

template <typename T>
void stats_launch(vof2d_ctx* h) {
  constexpr int V = VecWidth<T>::V;
  const StatsPlan pl = stats_plan(h, h->stats_mask);
  const unsigned nb = blocks_rows(pl.rep.rows(), pl.rep.ntj, pl.R);
  if (!nb) return;
  const StatsPlanes planes = stats_planes(h, pl);
  dispatch([&](auto M1, auto M2) {
    constexpr int MASK = (M1() ? STM_MOMENTS : 0) | (M2() ? STM_ENVELOPE : 0);
    if constexpr (MASK != 0)
      launch(h, kOther, k_stats<T, V, MASK>, dim3(nb), 0, pl.rep.g, (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), pl.R,
             planes, h->stats_level, (double)h->istep);
  }, (h->stats_mask & STM_MOMENTS) != 0, (h->stats_mask & STM_ENVELOPE) != 0);
}
// One sample of the fields as vof_get_field would return them now: settle_ghosts first, like the other readers (the wall faces of u
// may be virtual after a fused step; a k_tm batch may have left the predictor ahead).  Enqueues only.
int stats_sample(vof2d_ctx* h) {
  settle_ghosts(h);
  DISPATCH_T(h, stats_launch<double>(h), stats_launch<float>(h));
  if (h->stats_samples++ == 0) h->stats_first = h->istep;
  h->stats_last = h->istep;
  return ensure_ok(h);
}

// vof_stats_get: one plane, dense (nx, ny) doubles, waited for.  The entry point has checked the slot, its group and the cap.
int stats_get(vof2d_ctx* h, int slot, double* dst) {
  const StatsPlan pl = stats_plan(h, h->stats_mask);
  const size_t width = (size_t)h->g.ny * sizeof(double);
  HIPCHK(h, hipMemcpy2DAsync(dst, width, h->buf.stats.as<char>(pl.at.plane[slot]), pl.pitch * sizeof(double), width, (size_t)h->d.nx, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VOF_OK;
}

// vof_stats_summary: with the envelope the two reduced values come from the device (one copy, one wait); the rest is the host's.
int stats_summary(vof2d_ctx* h, double* out) {
  double red[kStatsPart] = {0.0, 0.0};
  const StatsPlan pl = stats_plan(h, h->stats_mask);
  if (h->stats_mask & STM_ENVELOPE) {
    const DevBuf& w = h->buf.stats;
    double* const part = w.as<double>(pl.at.part);
    if (pl.blocks)
      launch(h, kOther, k_stats_summary<2>, dim3(pl.blocks), 0, pl.rep.g, (const double*)w.as<double>(pl.at.plane[ST_ARRIVAL]),
             (const double*)w.as<double>(pl.at.plane[ST_MAX_SPEED2]), (long long)pl.pitch, diag_chunk(h), part);
    launch(h, kOther, k_row_finish<1, 1>, dim3(1), 0, (const double*)part, (int)pl.blocks, w.as<double>(pl.at.sum), 0.0, 0.0, kStatsRow);
    if (const int rc = ensure_ok(h)) return rc;
    if (const int rc = read_back(h, red, w.as<double>(pl.at.sum), sizeof(red))) return rc;
  }
  for (int k = 0; k < STS_N; ++k) out[k] = 0.0;
  out[STS_SAMPLES] = (double)h->stats_samples;
  out[STS_ISTEP_FIRST] = (double)h->stats_first;
  out[STS_ISTEP_LAST] = (double)h->stats_last;
  out[STS_MASK] = (double)h->stats_mask;
  out[STS_LEVEL] = h->stats_level;
  out[STS_CELLS] = (double)pl.rep.cells();
  out[STS_EVER_WET] = red[0];
  out[STS_MAX_SPEED2] = red[1];
  return VOF_OK;
}

// step_groups_n (runtime/step.h) with a sample behind every group; nothing is read back
int step_stats_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, int64_t* samples_taken) {
  if (const int rc = step_groups_n(h, nsteps, every, cycles, criterion, [&](int64_t) { return stats_sample(h); })) return rc;
  if (samples_taken) *samples_taken = nsteps / every;
  return VOF_OK;
}

}  // namespace
