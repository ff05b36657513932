// runtime/scene.h -- vof_set_scene: what is refused before anything changes (scene_check), the records as the device reads them
// (scene_pack), the layout of the handle's scene buffer; with HIP, the upload, the launch of k_scene and the summary
//
// The first part is plain C++ (no HIP): the CPU tests compile it on its own (tests/host/scene_check.cpp).  The second part is part
// of the host-side runtime of libvof2d_hip.so (the include order: vof2d_api.hip) and has internal linkage.
#pragma once
#include <cmath>
#include <stddef.h>
#include <stdint.h>

#include "../../../include/vof2d.h"

namespace vof {

// The scene buffer of a handle: room for the longest list; behind it the counters, kSceneSlots slots of kSceneSlotWords 64-bit
// words (64 bytes: the waves of k_scene spread their atomics over the slots), of which a slot uses the first two
constexpr size_t kSceneShapesBytes = (size_t)VOF_SCENE_MAX_SHAPES * VOF_SHAPE_N * sizeof(double);
constexpr size_t kSceneSlots = 256, kSceneSlotWords = 8;
constexpr size_t kSceneWordsBytes = kSceneSlots * kSceneSlotWords * sizeof(unsigned long long);
constexpr size_t kSceneBufBytes = kSceneShapesBytes + kSceneWordsBytes;

inline bool scene_samples_ok(int32_t samples) { return samples == 1 || samples == 2 || samples == 4 || samples == 8 || samples == 16; }

// NULL if record r (VOF_SHAPE_N doubles) can be painted, else what is wrong with it
inline const char* scene_check_record(const double* r) {
  for (int k = 0; k < VOF_SHAPE_N; ++k)
    if (!std::isfinite(r[k])) return "a shape record holds a number that is not finite";
  const double kind = r[VOF_SHAPE_KIND], phase = r[VOF_SHAPE_PHASE];
  if (kind != VOF_SHAPE_BOX && kind != VOF_SHAPE_ELLIPSE && kind != VOF_SHAPE_HALFPLANE && kind != VOF_SHAPE_TRIANGLE)
    return "a shape's KIND is not one of VOF_SHAPE_BOX .. VOF_SHAPE_TRIANGLE";
  if (phase != VOF_SCENE_GAS && phase != VOF_SCENE_LIQUID) return "a shape's PHASE is not VOF_SCENE_GAS or VOF_SCENE_LIQUID";
  const double* const a = r + VOF_SHAPE_A0;
  if (kind == VOF_SHAPE_BOX || kind == VOF_SHAPE_ELLIPSE) {
    if (a[2] < 0.0 || a[3] < 0.0) return "a box or an ellipse has a negative half extent";
    if (!(std::fabs(a[4] * a[4] + a[5] * a[5] - 1.0) <= 1e-9)) return "c, s of a box or an ellipse are not a cosine and a sine: |c*c + s*s - 1| > 1e-9";
  } else if (kind == VOF_SHAPE_HALFPLANE) {
    if (a[2] == 0.0 && a[3] == 0.0) return "a half-plane has a zero normal";
  }
  return nullptr;
}

// NULL if vof_set_scene may go on with these arguments (the handle apart), else the message of its VOF_EINVAL
inline const char* scene_check(const double* shapes, int64_t n, int32_t samples, int32_t flags) {
  if (n < 0 || n > VOF_SCENE_MAX_SHAPES) return "n must lie in [0, VOF_SCENE_MAX_SHAPES]";
  if (!shapes && n > 0) return "shapes is NULL with n > 0";
  if (!scene_samples_ok(samples)) return "samples must be 1, 2, 4, 8 or 16";
  if (flags & ~VOF_SCENE_CLEAR) return "flags has a bit outside VOF_SCENE_CLEAR";
  for (int64_t k = 0; k < n; ++k)
    if (const char* const msg = scene_check_record(shapes + k * VOF_SHAPE_N)) return msg;
  return nullptr;
}

// The records as k_scene reads them, into out (n x VOF_SHAPE_N doubles): the fields a kind does not use read 0, so that two lists
// that paint the same are the same bytes.  The list has passed scene_check.
inline void scene_pack(const double* shapes, int64_t n, double* out) {
  for (int64_t k = 0; k < n; ++k) {
    const double* const r = shapes + k * VOF_SHAPE_N;
    double* const o = out + k * VOF_SHAPE_N;
    const int used = r[VOF_SHAPE_KIND] == VOF_SHAPE_HALFPLANE ? VOF_SHAPE_A0 + 4 : VOF_SHAPE_N;
    for (int c = 0; c < VOF_SHAPE_N; ++c) o[c] = c < used ? r[c] : 0.0;
  }
}

}  // namespace vof

#ifdef __HIPCC__
namespace {

static_assert(SHK_BOX == VOF_SHAPE_BOX && SHK_ELLIPSE == VOF_SHAPE_ELLIPSE && SHK_HALFPLANE == VOF_SHAPE_HALFPLANE && SHK_TRIANGLE == VOF_SHAPE_TRIANGLE &&
              SHP_GAS == VOF_SCENE_GAS && SHP_LIQUID == VOF_SCENE_LIQUID && SHR_KIND == VOF_SHAPE_KIND && SHR_PHASE == VOF_SHAPE_PHASE &&
              SHR_A0 == VOF_SHAPE_A0 && SHR_N == VOF_SHAPE_N && SCF_CLEAR == VOF_SCENE_CLEAR && SCW_SLOTS == (int)kSceneSlots && SCW_STRIDE == (int)kSceneSlotWords,
              "kernels/scene.h, runtime/scene.h and include/vof2d.h name the same things");

template <typename T>
void scene_launch(vof2d_ctx* h, int n, int samples, int flags) {
  const Reported rep = reported(h);
  const dim3 grid((h->g.ny + 2 + 255) / 256, h->g.row_hi - h->g.row_lo + 1);
  const double* const shapes = h->buf.scene.as<double>();
  unsigned long long* const words = h->buf.scene.as<unsigned long long>(kSceneShapesBytes);
  const int clear = (flags & SCF_CLEAR) ? 1 : 0, shortcuts = h->scene_shortcuts ? 1 : 0;
#define VOF_SCENE_CASE(S) \
  case S: launch(h, kOther, k_scene<T, S>, grid, 0, h->g, F_<T>(h, fF), F_<T>(h, fF2), shapes, n, clear, shortcuts, h->cd.dx, h->cd.dy, rep.range.first, rep.range.last, words); break
  switch (samples) {
    VOF_SCENE_CASE(1);
    VOF_SCENE_CASE(2);
    VOF_SCENE_CASE(4);
    VOF_SCENE_CASE(8);
    VOF_SCENE_CASE(16);
  }
#undef VOF_SCENE_CASE
}

// vof_set_scene behind its checks: the list to the device, the counters zeroed, the pass; then F counts as written from outside,
// like vof_set_init_F's.  The counters are read back (one wait), so the host copy of the list may be reused by the next call.
int scene_run(vof2d_ctx* h, const double* shapes, int64_t n, int samples, int flags, double* summary) {
  unsigned long long painted = 0ull, mixed = 0ull;
  if (n > 0 || (flags & SCF_CLEAR)) {   // (an empty list without CLEAR is the identity: nothing is enqueued, no state changes)
    if (const int rc = h->buf.scene.reserve(h, kSceneBufBytes, "vof_set_scene: no memory for the shape list")) return rc;
    settle_ghosts(h);
    if (n > 0) {
      h->scene_host.resize((size_t)n * VOF_SHAPE_N);
      scene_pack(shapes, n, h->scene_host.data());
      HIPCHK(h, hipMemcpyAsync(h->buf.scene.p, h->scene_host.data(), (size_t)n * VOF_SHAPE_N * sizeof(double), hipMemcpyHostToDevice, h->stream));
    }
    unsigned long long* const d_words = h->buf.scene.as<unsigned long long>(kSceneShapesBytes);
    HIPCHK(h, hipMemsetAsync(d_words, 0, kSceneWordsBytes, h->stream));
    DISPATCH_T(h, scene_launch<double>(h, (int)n, samples, flags), scene_launch<float>(h, (int)n, samples, flags));
    if (field_written(h->state, fF, h->g.wall_lo && h->g.wall_hi, false)) forget_batch_form(h);
    if (tm_by_rule(h)) (void)post_gas_count(h);   // (see vof_set_init_F)
    if (const int rc = ensure_ok(h)) return rc;
    h->scene_words.resize(kSceneSlots * kSceneSlotWords);
    if (const int rc = read_back(h, h->scene_words.data(), d_words, kSceneWordsBytes)) return rc;
    for (size_t s = 0; s < kSceneSlots; ++s) {
      painted += h->scene_words[s * kSceneSlotWords + SCW_PAINTED];
      mixed += h->scene_words[s * kSceneSlotWords + SCW_MIXED];
    }
  }
  if (summary) {
    for (int k = 0; k < VOF_SCENE_SUM_N; ++k) summary[k] = 0.0;
    summary[VOF_SCENE_SUM_SHAPES] = (double)n;
    summary[VOF_SCENE_SUM_SAMPLES] = (double)samples;
    summary[VOF_SCENE_SUM_PAINTED] = (double)painted;
    summary[VOF_SCENE_SUM_MIXED] = (double)mixed;
    summary[VOF_SCENE_SUM_ISTEP] = (double)h->istep;
  }
  return VOF_OK;
}

}  // namespace
#endif  // __HIPCC__
