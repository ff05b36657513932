// runtime/frames.h -- vof_frame_set_lut, vof_frame and vof_step_frames: the handle's buffers, the launches of k_frame_cols,
// k_frame_fold and k_frame_paint, the stepping loop that records a frame behind every group of steps
//
// Part of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip).  Everything here has internal linkage.
#pragma once
#include "dye.h"

namespace {

static_assert(FQ_F == VOF_FRAME_F && FQ_U == VOF_FRAME_U && FQ_V == VOF_FRAME_V && FQ_SPEED == VOF_FRAME_SPEED && FQ_P == VOF_FRAME_P && FQ_VORT == VOF_FRAME_VORT &&
              FQ_DYE == VOF_FRAME_DYE && FRF_CONTOUR == VOF_FRAME_CONTOUR && FRF_SYMMETRIC == VOF_FRAME_SYMMETRIC && FRS_N == VOF_FRAME_SUM_N &&
              FRS_PW == VOF_FRAME_SUM_PW && FRS_PH == VOF_FRAME_SUM_PH && FRS_ISTEP == VOF_FRAME_SUM_ISTEP && FRS_LO == VOF_FRAME_SUM_LO && FRS_HI == VOF_FRAME_SUM_HI &&
              FRS_NAN_PIXELS == VOF_FRAME_SUM_NAN_PIXELS && FRS_CONTOUR_PIXELS == VOF_FRAME_SUM_CONTOUR_PIXELS && kFrameLutRows == VOF_FRAME_LUT_ROWS,
              "kernels/frames.h and include/vof2d.h name the same quantities, flags and slots");

constexpr size_t kFrameLutBytes = (size_t)kFrameLutRows * 3, kFrameSumBytes = FRS_N * sizeof(double);

// What a frame of `spec` launches on the handle (a whole domain) and where its work and results lie in buf.frame_work.  The
// means of F are kept beside the quantity's only where the contour is on and the quantity is not F itself.
struct FramePlan { FrameGeom fg; FrameCarve at; bool contour, f_beside; };
inline FramePlan frame_plan(const vof2d_ctx* h, const vof2d_frame_spec& spec) {
  FramePlan pl;
  pl.fg = frame_geom(h->d.nx, h->d.ny, h->g.ntj, 64 * h->V, spec.bx, spec.by);
  pl.contour = (spec.flags & FRF_CONTOUR) != 0;
  pl.f_beside = pl.contour && spec.quantity != FQ_F;
  pl.at = carve_frame((size_t)pl.fg.col_partials, (size_t)pl.fg.pixels, pl.f_beside ? (size_t)pl.fg.col_partials : 0, pl.f_beside ? (size_t)pl.fg.pixels : 0);
  return pl;
}

// The colour table: 258 x 3 bytes on the device -- state, not scratch.  NULL: the default, a grey ramp, a black contour, magenta for NaN.
int frame_set_lut(vof2d_ctx* h, const uint8_t* lut) {
  uint8_t def[kFrameLutBytes];
  if (!lut) {
    for (int k = 0; k < 256; ++k) def[3 * k] = def[3 * k + 1] = def[3 * k + 2] = (uint8_t)k;
    def[3 * kFrameLutContour] = def[3 * kFrameLutContour + 1] = def[3 * kFrameLutContour + 2] = 0;
    def[3 * kFrameLutNan] = 255; def[3 * kFrameLutNan + 1] = 0; def[3 * kFrameLutNan + 2] = 255;
    lut = def;
  }
  if (const int rc = h->buf.frame_lut.reserve(h, kFrameLutBytes, "vof_frame_set_lut: no memory for the colour table")) return rc;
  HIPCHK(h, hipMemcpyAsync(h->buf.frame_lut.p, lut, kFrameLutBytes, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));   // (lut is the caller's, or this frame's)
  return VOF_OK;
}

// Room for a frame of the plan, the table on first use; for vof_frame, room for its results on the host.  Called before
// anything of the call is enqueued.
int frame_prepare(vof2d_ctx* h, const FramePlan& pl) {
  if (!h->buf.frame_lut.p)
    if (const int rc = frame_set_lut(h, nullptr)) return rc;
  return h->buf.frame_work.reserve(h, pl.at.total, "vof_frame: no memory for the partials and the picture");
}
int frame_prepare_host(vof2d_ctx* h, size_t bytes) {
  if (h->h_frame_bytes >= bytes) return VOF_OK;
  if (h->h_frame) (void)hipHostFree(h->h_frame);
  h->h_frame = nullptr;
  h->h_frame_bytes = 0;
  if (hipHostMalloc(reinterpret_cast<void**>(&h->h_frame), bytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    h->h_frame = nullptr;
    return fail(h, VOF_ENOMEM, "vof_frame: no pinned host memory for the results");
  }
  h->h_frame_bytes = bytes;
  return VOF_OK;
}

// One frame of the current view of the fields: the words zeroed, the pass, the fold, the picture into `rgb` and the summary
// into `summary` (device: the arena's ranges, or a slot of buf.frame_recs).  Enqueues only.
template <typename T>
int frame_launch(vof2d_ctx* h, const vof2d_frame_spec& spec, const FramePlan& pl, unsigned char* rgb, double* summary) {
  constexpr int V = VecWidth<T>::V;
  const DevBuf& w = h->buf.frame_work;
  const FrameGeom& fg = pl.fg;
  unsigned long long* const words = w.as<unsigned long long>(pl.at.words);
  double* const colq = w.as<double>(pl.at.colq);
  double* const colF = pl.f_beside ? w.as<double>(pl.at.colF) : nullptr;
  double* const means = w.as<double>(pl.at.means);
  double* const mF = pl.f_beside ? w.as<double>(pl.at.mF) : nullptr;
  const T* const F = F_<T>(h, fF);
  const T* const u = F_<T>(h, fU);
  const T* const v = F_<T>(h, fV);
  const T* const s = spec.quantity == FQ_P ? (const T*)F_<T>(h, fP) : (spec.quantity == FQ_DYE ? (const T*)dye_array<T>(h, h->dye_cur) : F);
  const double hx = 0.5 * h->cd.dxi, hy = 0.5 * h->cd.dyi;
  HIPCHK(h, hipMemsetAsync(words, 0, pl.at.words_bytes, h->stream));
  dispatch([&](auto BESIDE) {
    constexpr bool B = decltype(BESIDE)::value;
    auto go = [&](auto QC) {
      launch(h, kOther, k_frame_cols<T, V, decltype(QC)::value, B>, dim3(fg.cols_blocks), 0, h->g, s, u, v, F, fg.R, fg.bx, fg.cpitch, hx, hy, colq, colF);
    };
    switch (spec.quantity) {
      case FQ_U: go(IC<FQ_U>{}); break;
      case FQ_V: go(IC<FQ_V>{}); break;
      case FQ_SPEED: go(IC<FQ_SPEED>{}); break;
      case FQ_VORT: go(IC<FQ_VORT>{}); break;
      default: go(IC<FQ_F>{}); break;   // F, p, the dye: the cell of `s`
    }
  }, pl.f_beside);
  launch(h, kOther, k_frame_fold, dim3(fg.pixel_blocks), 0, (const double*)colq, (const double*)colF, h->d.nx, h->d.ny, fg.bx, fg.by, fg.pw, fg.ph, fg.cpitch, means, mF, words);
  const bool auto_range = spec.lo == spec.hi;
  launch(h, kOther, k_frame_paint, dim3(fg.pixel_blocks), 0, (const double*)means, (const double*)(pl.contour ? (pl.f_beside ? mF : means) : nullptr), fg.pw, fg.ph,
         (int)spec.flags, (int)auto_range, spec.lo, spec.hi, (const unsigned char*)h->buf.frame_lut.as<unsigned char>(), words, rgb, summary, (double)h->istep);
  return VOF_OK;
}
// ... of the fields as vof_get_field would return them now: settle_ghosts first, like the other readers (VORT reads the ghost
// cells of u and v; a k_tm batch may have left the predictor ahead)
int frame_enqueue(vof2d_ctx* h, const vof2d_frame_spec& spec, const FramePlan& pl, unsigned char* rgb, double* summary) {
  settle_ghosts(h);
  int rc;
  DISPATCH_T(h, rc = frame_launch<double>(h, spec, pl, rgb, summary), rc = frame_launch<float>(h, spec, pl, rgb, summary));
  return rc ? rc : ensure_ok(h);
}

// vof_frame: room, the frame, ONE copy of the results (the means, the summary, the picture: consecutive in the arena, and of
// them the range from the first to the last that was asked for -- the means are eight bytes a pixel, the picture three) into
// the handle's pinned host buffer, one wait; then what was asked for goes to the caller's arrays.  The entry point has
// checked the arguments.
int frame_run(vof2d_ctx* h, const vof2d_frame_spec& spec, uint8_t* rgb, double* means, double* summary) {
  const FramePlan pl = frame_plan(h, spec);
  const size_t first = means ? pl.at.means : pl.at.sum, bytes = (rgb ? pl.at.total : pl.at.sum + kFrameSumBytes) - first;
  int rc = frame_prepare(h, pl);
  if (rc) return rc;
  if ((rc = frame_prepare_host(h, bytes))) return rc;
  const DevBuf& w = h->buf.frame_work;
  if ((rc = frame_enqueue(h, spec, pl, w.as<unsigned char>(pl.at.rgb), w.as<double>(pl.at.sum)))) return rc;
  if ((rc = read_back(h, h->h_frame, w.as<char>(first), bytes))) return rc;
  const char* const res = h->h_frame;   // (the arena from `first` on)
  if (means) memcpy(means, res + (pl.at.means - first), (size_t)pl.fg.pixels * sizeof(double));
  if (rgb) memcpy(rgb, res + (pl.at.rgb - first), pl.at.rgb_bytes);
  memcpy(summary, res + (pl.at.sum - first), kFrameSumBytes);
  return VOF_OK;
}

// step_groups_n (runtime/step.h) with a frame behind every group -- its picture and its summary written by k_frame_paint
// into slot r of buf.frame_recs (the pictures first, the summaries behind them) --, one read-back each at the end
int step_frames_n(vof2d_ctx* h, int64_t nsteps, int64_t every, int cycles, int criterion, const vof2d_frame_spec& spec, uint8_t* out_rgb, double* out_summaries,
                  int64_t* frames_written) {
  const int64_t frames = nsteps / every;
  const FramePlan pl = frame_plan(h, spec);
  const size_t rgb_bytes = pl.at.rgb_bytes;
  Carve recs;
  const size_t at_rgb = recs.take((size_t)frames * rgb_bytes), at_sum = recs.doubles((size_t)frames * FRS_N);
  int rc;
  if (frames > 0) {
    if ((rc = frame_prepare(h, pl))) return rc;
    if ((rc = h->buf.frame_recs.reserve(h, recs.total, "vof_step_frames: no memory for the frames"))) return rc;
  }
  rc = step_groups_n(h, nsteps, every, cycles, criterion, [&](int64_t r) {
    return frame_enqueue(h, spec, pl, h->buf.frame_recs.as<unsigned char>(at_rgb + (size_t)r * rgb_bytes), h->buf.frame_recs.as<double>(at_sum) + r * FRS_N);
  });
  if (rc) return rc;
  if (frames > 0) {
    HIPCHK(h, hipMemcpyAsync(out_rgb, h->buf.frame_recs.as<char>(at_rgb), (size_t)frames * rgb_bytes, hipMemcpyDeviceToHost, h->stream));
    if ((rc = read_back(h, out_summaries, h->buf.frame_recs.as<char>(at_sum), (size_t)frames * kFrameSumBytes))) return rc;
  }
  if (frames_written) *frames_written = frames;
  return VOF_OK;
}

}  // namespace
