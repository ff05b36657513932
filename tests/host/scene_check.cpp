// Stand-alone check (host compiler, no HIP) of what vof_set_scene does on the host before anything reaches the device
// (runtime/scene.h): scene_check refuses every argument and every record include/vof2d.h lists, with a message, and passes what it
// allows; scene_pack copies a list -- the longest one too -- record for record into a buffer of exactly n records, zeroing the fields
// a kind does not use; the scene buffer has room for the longest list and the counter slots.
// Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "runtime/scene.h"

using namespace vof;

static int failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

struct Rec { double v[VOF_SHAPE_N]; };
static Rec rec(double kind, double phase, double a0, double a1, double a2, double a3, double a4, double a5) { return Rec{{kind, phase, a0, a1, a2, a3, a4, a5}}; }
static const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

static bool refused(const Rec& r) { return scene_check(r.v, 1, 8, 0) != nullptr && scene_check_record(r.v) != nullptr; }
static bool allowed(const Rec& r) { return scene_check(r.v, 1, 8, VOF_SCENE_CLEAR) == nullptr && scene_check_record(r.v) == nullptr; }

int main() {
  long n = 0;
  const double c = std::cos(0.7), s = std::sin(0.7);
  const Rec good[] = {
      rec(VOF_SHAPE_BOX, VOF_SCENE_LIQUID, 0.05, 0.05, 0.01, 0.02, c, s),   rec(VOF_SHAPE_BOX, VOF_SCENE_GAS, 0.05, 0.05, 0.0, 0.0, 1.0, 0.0),
      rec(VOF_SHAPE_ELLIPSE, VOF_SCENE_GAS, -3.0, 9.0, 0.5, 0.0, -s, c),    rec(VOF_SHAPE_ELLIPSE, VOF_SCENE_LIQUID, 0, 0, 1, 1, 1.0 + 4e-10, 0.0),
      rec(VOF_SHAPE_HALFPLANE, VOF_SCENE_LIQUID, 0.0, 0.04, 0.0, 1e-300, 0.0, 0.0),
      rec(VOF_SHAPE_HALFPLANE, VOF_SCENE_GAS, 0.0, 0.04, -1.0, 0.0, 5.0, 6.0),   // (A4, A5 of a half-plane: finite, otherwise free)
      rec(VOF_SHAPE_TRIANGLE, VOF_SCENE_LIQUID, 0, 0, 1, 0, 0, 1),          rec(VOF_SHAPE_TRIANGLE, VOF_SCENE_GAS, 2, 2, 2, 2, 2, 2),
  };
  for (const Rec& r : good) { CHECK(allowed(r), "kind %g", r.v[0]); ++n; }

  // ---- every refusal of a record
  const Rec bad[] = {
      rec(4.0, VOF_SCENE_LIQUID, 0, 0, 1, 1, 1, 0),            rec(-1.0, VOF_SCENE_LIQUID, 0, 0, 1, 1, 1, 0),
      rec(0.5, VOF_SCENE_LIQUID, 0, 0, 1, 1, 1, 0),            rec(VOF_SHAPE_BOX, 2.0, 0, 0, 1, 1, 1, 0),
      rec(VOF_SHAPE_BOX, -1.0, 0, 0, 1, 1, 1, 0),              rec(VOF_SHAPE_BOX, 0.25, 0, 0, 1, 1, 1, 0),
      rec(VOF_SHAPE_BOX, VOF_SCENE_LIQUID, 0, 0, -1e-300, 1, 1, 0),   rec(VOF_SHAPE_ELLIPSE, VOF_SCENE_LIQUID, 0, 0, 1, -2, 1, 0),
      rec(VOF_SHAPE_BOX, VOF_SCENE_LIQUID, 0, 0, 1, 1, 1, 1e-4),      rec(VOF_SHAPE_ELLIPSE, VOF_SCENE_GAS, 0, 0, 1, 1, 0, 0),
      rec(VOF_SHAPE_BOX, VOF_SCENE_LIQUID, 0, 0, 1, 1, 1.0 + 1e-8, 0),   rec(VOF_SHAPE_BOX, VOF_SCENE_LIQUID, 0, 0, 1, 1, 1e200, 0),
      rec(VOF_SHAPE_HALFPLANE, VOF_SCENE_LIQUID, 0.1, 0.1, 0.0, 0.0, 0, 0),   rec(VOF_SHAPE_HALFPLANE, VOF_SCENE_LIQUID, 0.1, 0.1, -0.0, 0.0, 0, 0),
  };
  for (const Rec& r : bad) { CHECK(refused(r), "kind %g phase %g", r.v[0], r.v[1]); ++n; }
  for (const Rec& g : good)
    for (int k = 0; k < VOF_SHAPE_N; ++k)
      for (double x : {kNan, kInf, -kInf}) {                   // a number that is not finite, in every field of every kind
        Rec r = g;
        r.v[k] = x;
        CHECK(refused(r), "kind %g field %d = %g", g.v[0], k, x);
        ++n;
      }

  // ---- the arguments
  CHECK(scene_check(nullptr, 0, 8, 0) == nullptr && scene_check(nullptr, 0, 1, VOF_SCENE_CLEAR) == nullptr, "an empty list is valid");
  CHECK(scene_check(good[0].v, 0, 16, 0) == nullptr, "n == 0 with a pointer");
  CHECK(scene_check(nullptr, 1, 8, 0) != nullptr, "NULL with n > 0");
  CHECK(scene_check(good[0].v, -1, 8, 0) != nullptr && scene_check(nullptr, -1, 8, 0) != nullptr, "n < 0");
  for (int samples : {1, 2, 4, 8, 16}) CHECK(scene_check(good[0].v, 1, samples, 0) == nullptr && scene_samples_ok(samples), "samples %d", samples);
  for (int samples : {0, -1, -8, 3, 5, 6, 7, 9, 12, 15, 17, 32, 64, 1 << 30}) CHECK(scene_check(good[0].v, 1, samples, 0) != nullptr && !scene_samples_ok(samples), "samples %d", samples);
  for (int flags : {2, 3, 4, -1, 1 << 30}) CHECK(scene_check(good[0].v, 1, 8, flags) != nullptr, "flags %d", flags);
  n += 30;

  // ---- lists: a bad record anywhere is found; the longest list passes, one more does not (and is not read)
  {
    std::vector<double> list((size_t)VOF_SCENE_MAX_SHAPES * VOF_SHAPE_N);
    for (int k = 0; k < VOF_SCENE_MAX_SHAPES; ++k) std::memcpy(&list[(size_t)k * VOF_SHAPE_N], good[k % 8].v, sizeof(Rec));
    CHECK(scene_check(list.data(), VOF_SCENE_MAX_SHAPES, 8, 0) == nullptr, "the longest list");
    CHECK(scene_check(list.data(), (int64_t)VOF_SCENE_MAX_SHAPES + 1, 8, 0) != nullptr, "one more than the longest list");   // (would read past the end if it looked)
    CHECK(scene_check(list.data(), INT64_MAX, 8, 0) != nullptr && scene_check(list.data(), INT64_MIN, 8, 0) != nullptr, "n at the ends of its type");
    for (int at : {0, 1, 511, VOF_SCENE_MAX_SHAPES - 1}) {
      std::vector<double> l2 = list;
      l2[(size_t)at * VOF_SHAPE_N + VOF_SHAPE_PHASE] = 3.0;
      CHECK(scene_check(l2.data(), VOF_SCENE_MAX_SHAPES, 8, 0) != nullptr, "a bad record at %d", at);
      CHECK(scene_check(l2.data(), at, 8, 0) == nullptr, "the records in front of %d", at);
    }
    // packing: into exactly n records (the sanitizer sees a write past the end), record for record
    std::vector<double> out((size_t)VOF_SCENE_MAX_SHAPES * VOF_SHAPE_N, -7.0);
    scene_pack(list.data(), VOF_SCENE_MAX_SHAPES, out.data());
    for (int k = 0; k < VOF_SCENE_MAX_SHAPES; ++k) {
      const double* const r = &list[(size_t)k * VOF_SHAPE_N];
      const double* const o = &out[(size_t)k * VOF_SHAPE_N];
      const int used = r[VOF_SHAPE_KIND] == VOF_SHAPE_HALFPLANE ? 6 : VOF_SHAPE_N;
      for (int c2 = 0; c2 < VOF_SHAPE_N; ++c2) CHECK(o[c2] == (c2 < used ? r[c2] : 0.0), "record %d field %d", k, c2);
    }
    std::vector<double> three(3 * VOF_SHAPE_N, -7.0), none;
    scene_pack(list.data(), 3, three.data());
    scene_pack(list.data(), 0, none.data());
    CHECK(std::memcmp(three.data(), out.data(), three.size() * sizeof(double)) == 0, "a prefix packs like the list");
    n += 12 + VOF_SCENE_MAX_SHAPES;
  }

  // ---- the buffer
  CHECK(kSceneShapesBytes == (size_t)1024 * 64 && kSceneShapesBytes % 16 == 0, "the words behind the list are aligned");
  CHECK(kSceneWordsBytes == 256 * 64 && kSceneBufBytes == kSceneShapesBytes + kSceneWordsBytes && kSceneSlotWords >= 2, "the list and the slots of the two counters, 64 bytes apart");
  CHECK((kSceneSlots & (kSceneSlots - 1)) == 0, "a wave finds its slot with a mask");
  n += 2;

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld scene checks ok\n", n);
  return 0;
}
