// Stand-alone check (host compiler, no HIP) of what vof_stats_begin lays out on the host: the pitch of the accumulator planes
// (stats_pitch) and the arena (carve_stats, runtime/carve.h) over grids, masks and both dtypes -- every range aligned to 16
// bytes, in slot order, disjoint, inside the total; a plane of a group that is off has no range; every 16-byte vector a lane of
// k_stats or k_stats_summary forms (kernels/stats.h) lies inside its row of its plane.
// Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <cstdio>

#include "runtime/carve.h"

using namespace vof;

static int failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

// V = 2 elements per lane for both dtypes (vof2d_device.h): a wave tile is 128 columns; the planes are doubles whatever the fields are
static void check_stats(int nx, int ny, int mask, int esz, int V, size_t part_doubles) {
  const char* const fmt = "%dx%d mask %d, %d-byte fields";
#define CTX fmt, nx, ny, mask, esz
  const size_t D = sizeof(double), W = 64 * (size_t)V;
  const size_t ntj = ((size_t)ny + W - 1) / W;
  const size_t pitch = stats_pitch((size_t)ny, W);
  CHECK(pitch == ntj * W && pitch >= (size_t)ny && pitch - (size_t)ny < W && (pitch * D) % 16 == 0, CTX);
  const StatsCarve c = carve_stats((size_t)nx, pitch, mask, part_doubles);
  CHECK(c.plane_bytes == (size_t)nx * pitch * D && c.plane_bytes % 16 == 0, CTX);
  size_t end = 0;
  int on = 0;
  for (int k = 0; k < kStatsPlanes; ++k) {
    const bool want = (mask & (k < kStatsMomentPlanes ? 1 : 2)) != 0;
    if (!want) { CHECK(c.plane[k] == kNoRange, CTX); continue; }
    CHECK(c.plane[k] != kNoRange && c.plane[k] % 16 == 0 && c.plane[k] >= end && c.plane[k] + c.plane_bytes <= c.total, CTX);   // aligned, behind the one before it, inside
    CHECK(c.plane[k] == (size_t)on * c.plane_bytes, CTX);                                                                   // consecutive, in slot order
    end = c.plane[k] + c.plane_bytes;
    ++on;
  }
  CHECK(on == ((mask & 1) ? kStatsMomentPlanes : 0) + ((mask & 2) ? kStatsPlanes - kStatsMomentPlanes : 0), CTX);
  CHECK(c.planes_total == end && c.part % 16 == 0 && c.part >= end && c.sum % 16 == 0 && c.sum >= c.part + part_doubles * D, CTX);
  CHECK(c.total == c.sum + 2 * D, CTX);
  // the vectors of the first and of the last lane that takes part, in the first and in the last row: lane l of tile t holds the
  // columns j0 = 1 + t W + l V .. j0 + V - 1 at [(i - 1) pitch + (j0 - 1)]; k_stats leaves lanes with j0 > ny, k_stats_summary keeps all
  for (int i : {1, nx}) {
    for (size_t j0 : {(size_t)1, (size_t)(1 + ((size_t)ny - 1) / V * V), (size_t)(1 + (ntj - 1) * W + 63 * V)}) {
      const size_t at = ((size_t)i - 1) * pitch + (j0 - 1);
      CHECK((at * D) % 16 == 0 && at + V <= (size_t)i * pitch && (at + V) * D <= c.plane_bytes, CTX);
    }
  }
#undef CTX
}

int main() {
  const int sizes[12] = {3, 4, 7, 17, 33, 64, 127, 128, 129, 300, 513, 1100};
  long n = 0;
  for (int nx : sizes)
    for (int ny : sizes)
      for (int mask = 1; mask <= 3; ++mask)
        for (int esz : {8, 4}) {
          check_stats(nx, ny, mask, esz, 2, (size_t)((nx + 1) / 2 * ((ny + 127) / 128) + 3) / 4 * 2 + 1);
          ++n;
        }
  for (int mask = 1; mask <= 3; ++mask) { check_stats(4096, 4096, mask, 8, 2, 4097); check_stats(16384, 16384, mask, 4, 2, 1); n += 2; }
  {
    const StatsCarve c = carve_stats(4096, stats_pitch(4096, 128), 3, 4097);
    CHECK(c.plane_bytes == (size_t)4096 * 4096 * 8 && c.planes_total == 13 * c.plane_bytes && c.plane[12] == 12 * c.plane_bytes, "4096^2, both groups");
    const StatsCarve e = carve_stats(64, stats_pitch(129, 128), 2, 9);
    CHECK(e.plane_bytes == (size_t)64 * 256 * 8 && e.plane[9] == 0 && e.plane[12] == 3 * e.plane_bytes && e.plane[0] == kNoRange, "64 x 129, the envelope alone");
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld layouts ok\n", n);
  return 0;
}
