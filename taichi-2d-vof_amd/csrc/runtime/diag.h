// runtime/diag.h -- diagnostic build only (-DVOF_WAVE_TIMES): launches of the pair kernels in their ablated forms, and
// the vof_debug_* entry points that time them
//
// Included by vof2d_api.hip behind selftest.h; never part of the product library.
#pragma once
#include "schedule.h"

namespace {

template <int ABL>
void dbg_pair(vof2d_ctx* h, int plan) {
  typedef double T; constexpr int V = VecWidth<T>::V;
  int ntt = 0;
  const int R = L<T>::jacobi_pair_geom(h, ntt);
  const TbPlan tp = L<T>::tb_plan(h, plan ? (int)(h->istep & 1) : -1, PlanFor::kJacobiPair);
  const unsigned pairs = tp.masks ? (unsigned)tp.waves : (unsigned)(((h->g.ihi - h->g.ilo + R) / R) * ntt);
  launch_block(h, kJacobiPair, k_jacobi_pair<T, V, 5, true, ABL>, dim3(pairs), 128u, 0, h->g, L<T>::C(h), (const T*)F_<T>(h, fP),
               (const T*)F_<T>(h, fRHS), F_<T>(h, fPT), R, ntt, tp, h->g.ilo, h->g.ihi);
}
template <bool YFIRST, int ABL>
void dbg_tm(vof2d_ctx* h) {
  typedef double T; constexpr int V = VecWidth<T>::V;
  const int ntf = TmGeom<V>::tiles(h->g.ny), first = h->g.ilo, last = h->g.ihi;
  const RowSegments rows = L<T>::tm_chunk_rows(h, first, last, ntf, resident(h, k_tm<T, V, YFIRST, false, true, ABL>, 128));
  const TbPlan tp{nullptr, nullptr, 0, 0, 0, 0, 0};
  const unsigned pairs = (unsigned)(row_chunks(rows) * ntf);
  h->tm_segments_last = row_used_segments(rows);
  step_wrote_F(h->state);   // (the probe writes the twin of F, with values of its own: no zero map holds over it)
  launch_block(h, kTM, k_tm<T, V, YFIRST, false, true, ABL>, dim3(pairs), 128u, 0, h->g, L<T>::C(h), (const T*)F_<T>(h, fF), F_<T>(h, fF2), ntf,
               (const T*)F_<T>(h, fUS), (const T*)F_<T>(h, fVS), (const T*)F_<T>(h, fP), F_<T>(h, fU), F_<T>(h, fV),
               F_<T>(h, fMX), F_<T>(h, fMY), F_<T>(h, fRHS), h->d_courant + 3, tp, rows, ZeroMaps{nullptr, 0, 0, 0});
}

}  // namespace

// Diagnostic build only (make wavetimes; tools/wave_balance.py).  Arms the per-wave start/end
// stamps for kernel `kid` (KernelId) with room for `cap` waves, or reads them back (out != NULL).
extern "C" int vof_debug_wave_times(vof2d_handle h, int32_t kid, uint64_t* out, uint32_t cap) {
  static unsigned long long* buf = nullptr;
  static unsigned int bufcap = 0;
  if (!h) return VOF_EINVAL;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (out) {
    if (!buf || cap > bufcap) return VOF_EINVAL;
    if (kid == -2) {   // the second half: cycles inside barriers, cycles in all (the pair kernels)
      if (cap != bufcap) return VOF_EINVAL;
      HIPCHK(h, hipMemcpy(out, buf + 2 * (size_t)bufcap, (size_t)cap * 16, hipMemcpyDeviceToHost));
      return VOF_OK;
    }
    HIPCHK(h, hipMemcpy(out, buf, (size_t)cap * 16, hipMemcpyDeviceToHost));
    return VOF_OK;
  }
  if (cap > bufcap) {
    if (buf) (void)hipFree(buf);
    HIPCHK(h, hipMalloc(&buf, (size_t)cap * 32));   // start / end stamps, then (barrier cycles, all cycles) per wave
    bufcap = cap;
  }
  HIPCHK(h, hipMemset(buf, 0, (size_t)bufcap * 32));
  int k = kid;
  HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(vof::vof_wave_times), &buf, sizeof(buf)));
  HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(vof::vof_wave_kid), &k, sizeof(k)));
  HIPCHK(h, hipMemcpyToSymbol(HIP_SYMBOL(vof::vof_wave_cap), &bufcap, sizeof(bufcap)));
  return VOF_OK;
}
// Diagnostic build only (tools/probes/pair_bound.py): `reps` launches of one pair kernel on the handle's current state
// between one event pair -- k_jacobi_pair (which = 0; p, rhs -> pt, no swap) or k_tm (1: y first, 2: x first; F, u*, v*, p ->
// the twin of F, the second u* / v* pair, rhs: all scratch outside a batch) -- in the ablated form `abl` (ABL_* bits,
// kernels/common.h; wrong values, the state the steps run on is not touched).  plan != 0: k_jacobi_pair on the step's work plan.
extern "C" int vof_debug_time_kernel(vof2d_handle h, int32_t which, int32_t abl, int32_t plan, int32_t reps, float* avg_us) {
  if (!h || !avg_us || reps < 1 || h->d.dtype != VOF_F64 || !buffer_stores_ok(h)) return VOF_EINVAL;
  // abl bit 256: every launch timed on its own behind a 268 MB fill of two arrays the kernels do not touch (rho, nu) --
  // the launch finds neither its inputs nor its last outputs in the L2 / MALL, as it does inside a step
  const bool cold = (abl & 256) != 0;
  abl &= 255;
  double sum_ms = 0.0;
  if (!cold) HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  for (int r = 0; r < reps; ++r) {
    if (cold) {
      HIPCHK(h, hipMemsetAsync(h->fld[fRHO], 0, h->field_elems * h->esz, h->stream));
      HIPCHK(h, hipMemsetAsync(h->fld[fNU], 0, h->field_elems * h->esz, h->stream));
      HIPCHK(h, hipEventRecord(h->ev0, h->stream));
    }
#define ABL_CASE(a) case a: if (which == 0) dbg_pair<a>(h, plan); else if (which == 1) dbg_tm<true, a>(h); else dbg_tm<false, a>(h); break;
    switch (abl) {
      ABL_CASE(0) ABL_CASE(1) ABL_CASE(2) ABL_CASE(3) ABL_CASE(4) ABL_CASE(8) ABL_CASE(16) ABL_CASE(32) ABL_CASE(48) ABL_CASE(19) ABL_CASE(35) ABL_CASE(64) ABL_CASE(192)
      default: return fail(h, VOF_EINVAL, "ablation not instantiated");
    }
#undef ABL_CASE
    if (cold) {
      HIPCHK(h, hipEventRecord(h->ev1, h->stream));
      HIPCHK(h, hipEventSynchronize(h->ev1));
      float ms1 = 0.f;
      HIPCHK(h, hipEventElapsedTime(&ms1, h->ev0, h->ev1));
      sum_ms += ms1;
    }
  }
  float ms = 0.f;
  if (!cold) {
    HIPCHK(h, hipEventRecord(h->ev1, h->stream));
    HIPCHK(h, hipEventSynchronize(h->ev1));
    HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  } else {
    ms = (float)sum_ms;
  }
  *avg_us = 1e3f * ms / (float)reps;
  return ensure_ok(h);
}
// Diagnostic build only (tools/probes/overlap_tail.py): what would it buy to let the NEXT step's k_jacobi_pair run in the slots
// the tail of k_tm leaves empty?  `reps` times [k_tm, k_jacobi_pair] on the handle's current state, timing only (the Jacobi
// launch reads the rhs the k_tm launch beside it is writing: wrong values, the state the steps run on is not touched):
//   mode 0  both on one stream, one after the other (what the step does);
//   mode 1  k_tm on a stream of the highest priority, k_jacobi_pair on one of the lowest, started together: the dispatcher
//           should hand the Jacobi launch's workgroups only the slots k_tm's pending workgroups do not want;
//   mode 2  the same without priorities (two plain streams);
//   mode 3  the priorities the other way round.
extern "C" int vof_debug_time_overlap(vof2d_handle h, int32_t mode, int32_t reps, float* avg_us) {
  if (!h || !avg_us || reps < 1 || h->d.dtype != VOF_F64 || !buffer_stores_ok(h)) return VOF_EINVAL;
  static hipStream_t sa = nullptr, sb = nullptr, sc = nullptr, sd = nullptr;
  static hipEvent_t e0 = nullptr, ea = nullptr, eb = nullptr;
  if (!sa) {
    int least = 0, greatest = 0;
    HIPCHK(h, hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(h, hipStreamCreateWithPriority(&sa, hipStreamNonBlocking, greatest));
    HIPCHK(h, hipStreamCreateWithPriority(&sb, hipStreamNonBlocking, least));
    HIPCHK(h, hipStreamCreateWithFlags(&sc, hipStreamNonBlocking));
    HIPCHK(h, hipStreamCreateWithFlags(&sd, hipStreamNonBlocking));
    HIPCHK(h, hipEventCreateWithFlags(&e0, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&ea, hipEventDisableTiming));
    HIPCHK(h, hipEventCreateWithFlags(&eb, hipEventDisableTiming));
    if (getenv("VOF2D_DEBUG")) fprintf(stderr, "[vof2d] stream priorities: least %d, greatest %d\n", least, greatest);
  }
  hipStream_t const st = h->stream;
  hipStream_t const s_tm = mode == 1 ? sa : mode == 3 ? sb : sc, s_j = mode == 1 ? sb : mode == 3 ? sa : sd;
  HIPCHK(h, hipEventRecord(h->ev0, st));
  for (int r = 0; r < reps; ++r) {
    const bool yf = (r & 1) == 0;
    if (mode == 0) {
      if (yf) dbg_tm<true, 0>(h); else dbg_tm<false, 0>(h);
      dbg_pair<0>(h, 0);
      continue;
    }
    HIPCHK(h, hipEventRecord(e0, st));
    HIPCHK(h, hipStreamWaitEvent(s_tm, e0, 0));
    HIPCHK(h, hipStreamWaitEvent(s_j, e0, 0));
    { StreamScope on(h, s_tm); if (yf) dbg_tm<true, 0>(h); else dbg_tm<false, 0>(h); }
    { StreamScope on(h, s_j); dbg_pair<0>(h, 0); }
    HIPCHK(h, hipEventRecord(ea, s_tm));
    HIPCHK(h, hipEventRecord(eb, s_j));
    HIPCHK(h, hipStreamWaitEvent(st, ea, 0));
    HIPCHK(h, hipStreamWaitEvent(st, eb, 0));
  }
  HIPCHK(h, hipEventRecord(h->ev1, st));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  float ms = 0.f;
  HIPCHK(h, hipEventElapsedTime(&ms, h->ev0, h->ev1));
  *avg_us = 1e3f * ms / (float)reps;
  return ensure_ok(h);
}
