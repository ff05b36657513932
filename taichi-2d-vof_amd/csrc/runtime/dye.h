// runtime/dye.h -- vof_dye_set / _get / _advance / _stats and vof_step_dye: the handle's dye arrays, the launches of k_dye (or
// the two sweeps), k_dye_stats, the stepping loop that moves the dye behind every step and records rows
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "depths.h"

namespace {

static_assert(DY_N == VOF_DYE_N && DY_ISTEP == VOF_DYE_ISTEP && DY_CELLS == VOF_DYE_CELLS && DY_SUM_C == VOF_DYE_SUM_C && DY_SUM_CI == VOF_DYE_SUM_CI &&
              DY_SUM_CJ == VOF_DYE_SUM_CJ && DY_SUM_C2 == VOF_DYE_SUM_C2 && DY_SUM_CF == VOF_DYE_SUM_CF && DY_SUM_CU == VOF_DYE_SUM_CU &&
              DY_SUM_CV == VOF_DYE_SUM_CV && DY_MIN_C == VOF_DYE_MIN_C && DY_MAX_C == VOF_DYE_MAX_C && DY_MAX_EXCESS == VOF_DYE_MAX_EXCESS,
              "kernels/dye.h and include/vof2d.h name the same slots");

// The dye and its twin: two arrays in the fields' layout (pitch, col0, tail pad), one behind the other in buf.dye; dye_cur
// says which of them holds the dye.  State, not scratch.
inline size_t dye_array_bytes(const vof2d_ctx* h) { return h->field_elems * h->esz; }
template <typename T> T* dye_array(const vof2d_ctx* h, int which) { return h->buf.dye.as<T>((size_t)which * dye_array_bytes(h)); }
inline size_t dye_dense_bytes(const vof2d_ctx* h) { return (size_t)(h->d.nx + 2) * (size_t)(h->g.ny + 2) * h->esz; }

// dense (nx+2, ny+2) host array <-> one of the two arrays, waited for
int dye_copy_host(vof2d_ctx* h, int which, void* host, bool to_host) {
  const size_t width = (size_t)(h->g.ny + 2) * h->esz, rows = (size_t)(h->d.nx + 2), dpitch = (size_t)h->g.pitch * h->esz;
  char* const dev = dye_array<char>(h, which) + (size_t)h->g.col0 * h->esz;
  if (to_host) HIPCHK(h, hipMemcpy2DAsync(host, width, dev, dpitch, width, rows, hipMemcpyDeviceToHost, h->stream));
  else HIPCHK(h, hipMemcpy2DAsync(dev, dpitch, host, width, width, rows, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return VOF_OK;
}

// A new dye (the entry point has checked nbytes): room on first use -- zeroed, so that the padding the tiles load is
// finite --, then the caller's cells, ghosts included, into BOTH arrays (the two-launch form reads the twin's ghost cells
// between its sweeps, as the sweeps of F do).  src == NULL: the handle gives the dye up.
int dye_set(vof2d_ctx* h, const void* src) {
  if (!src) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->buf.dye.release();
    h->dye_on = false;
    return VOF_OK;
  }
  if (const int rc = h->buf.dye.reserve(h, 2 * dye_array_bytes(h), "vof_dye_set: no memory for the dye and its twin", true)) return rc;
  for (int which = 0; which < 2; ++which)
    if (const int rc = dye_copy_host(h, which, const_cast<void*>(src), false)) return rc;
  h->dye_on = true;
  h->dye_cur = 0;
  return VOF_OK;
}

// One transport of the dye: solve_VOF_rudman(istep) with C for F, post_process_f, the F lines of set_BC -- on the pair
// (C, twin), the u, v the handle holds and the parity of its istep.  Knob dye_fused: 1 (default) k_dye, the result in the
// twin (dye_cur flips); 0 the two sweeps k_fct_x<CORR = false> / k_fct_y of the parent schedule, k_post, the result back
// in the array it started from.  The boundary launch writes the ghost ring of both arrays.
template <typename T>
void dye_advance_launch(vof2d_ctx* h) {
  constexpr int V = VecWidth<T>::V;
  const bool y_first = h->istep % 2 == 0;   // :312-318
  T* const C = dye_array<T>(h, h->dye_cur);
  T* const Cn = dye_array<T>(h, h->dye_cur ^ 1);
  if (h->dye_fused) {
    const int R = L<T>::transport_rows(h);
    dispatch([&](auto YF) {
      launch(h, kOther, k_dye<T, V, YF()>, dim3(blocks_rows(interior_rows(h), h->nty, R)), 0, h->g, L<T>::C(h), (const T*)C, Cn, h->nty,
             (const T*)F_<T>(h, fU), (const T*)F_<T>(h, fV), R);
    }, y_first);
    h->dye_cur ^= 1;
  } else {
    if (y_first) {
      L<T>::template fct_y<false, false>(h, 0, 0, C, Cn);
      L<T>::template fct_x<false, false>(h, 0, 0, Cn, C);
    } else {
      L<T>::template fct_x<false, false>(h, 0, 0, C, Cn);
      L<T>::template fct_y<false, false>(h, 0, 0, Cn, C);
    }
    L<T>::post(h, C, Cn);
  }
  L<T>::bc_F_pair(h, dye_array<T>(h, h->dye_cur), dye_array<T>(h, h->dye_cur ^ 1));
}
// ... on the u, v vof_get_field would return now: settle_ghosts first (the sweeps read set_BC's zeros on the wall faces; a
// k_tm batch may have left the predictor ahead).  Enqueues only.
int dye_advance(vof2d_ctx* h) {
  settle_ghosts(h);
  DISPATCH_T(h, dye_advance_launch<double>(h), dye_advance_launch<float>(h));
  return ensure_ok(h);
}

// ---- the statistics: one row of the dye and the fields on the reduced-row path of runtime/diag_reduce.h
constexpr ReducedVerb<kDyeSums, kDyePart - kDyeSums> kDyeVerb = {&WorkBufs::dye_stats, kDyeRow, "vof_dye_stats: no memory for the reduction buffer",
                                                                 "vof_step_dye: no memory for the rows"};
int dye_stats_enqueue(vof2d_ctx* h, int64_t slot) {
  return reduced_enqueue(h, kDyeVerb, slot, [&](auto t, const Geom& g, unsigned nb, int R, double* part) {
    using T = decltype(t);
    launch(h, kOther, k_dye_stats<T, VecWidth<T>::V>, dim3(nb), 0, g, (const T*)dye_array<T>(h, h->dye_cur), (const T*)F_<T>(h, fF), (const T*)F_<T>(h, fU),
           (const T*)F_<T>(h, fV), R, part);
  });
}

// step_groups_n (runtime/step.h) in groups of ONE step (the dye needs u, v of every step in memory, so no batch graph) with
// one advance of the dye behind each, and a row behind every `every`-th step (0: none); one read-back at the end
int step_dye_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, double* out, int64_t* rows_written) {
  const int64_t rows = every > 0 ? nsteps / every : 0;
  int rc;
  if (rows > 0 && (rc = reduced_prepare(h, kDyeVerb, rows))) return rc;
  rc = step_groups_n(h, nsteps, 1, cycles, criterion, [&](int64_t s) {
    if (const int rc = dye_advance(h)) return rc;
    return every > 0 && (s + 1) % every == 0 ? dye_stats_enqueue(h, (s + 1) / every - 1) : VOF_OK;
  });
  if (rc) return rc;
  if (rows > 0 && (rc = read_back(h, out, h->buf.dye_stats.rows.p, (size_t)rows * DY_N * sizeof(double)))) return rc;
  if (rows_written) *rows_written = rows;
  return VOF_OK;
}

}  // namespace
