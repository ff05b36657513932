// Stand-alone check (host compiler, no HIP) of what vof_regrid decides on the host before anything reaches the device
// (runtime/regrid_check.h): regrid_factors finds the factors and the direction of every pair of grids that stand in integer ratios of
// at most VOF_REGRID_MAX_FACTOR and refuses the others, with a message -- checked against a search over all factor pairs --;
// regrid_check refuses every argument include/vof2d.h lists and passes what it allows.
// Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <cstdio>
#include <initializer_list>
#include <limits>

#include "runtime/regrid_check.h"

using namespace vof;

static int failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

// the same answer by search: is there (rx, ry) in [1, MAX]^2 with dst = r * src (dir +1) or src = r * dst (dir -1)?
static bool by_search(int snx, int sny, int dnx, int dny, RegridFactors* f) {
  for (int rx = 1; rx <= VOF_REGRID_MAX_FACTOR; ++rx)
    for (int ry = 1; ry <= VOF_REGRID_MAX_FACTOR; ++ry) {
      const bool up = (long)snx * rx == dnx && (long)sny * ry == dny, down = (long)dnx * rx == snx && (long)dny * ry == sny;
      if (up || down) {
        *f = RegridFactors{rx, ry, rx == 1 && ry == 1 ? 0 : (up ? 1 : -1)};
        return true;
      }
    }
  return false;
}

int main() {
  long n = 0;
  // ---- the factors: every pair of small grids, and the pairs of the tests
  const int sizes[] = {3, 4, 5, 6, 8, 9, 11, 12, 16, 17, 24, 32, 33, 34, 48, 51, 64, 66, 96, 128, 132, 136, 256, 272, 384, 512, 528, 544, 2048};
  for (int snx : sizes) for (int sny : sizes) for (int dnx : sizes) for (int dny : sizes) {
    RegridFactors want{0, 0, 0}, got{-1, -1, -9};
    const bool ok = by_search(snx, sny, dnx, dny, &want);
    const char* const msg = regrid_factors(snx, sny, dnx, dny, &got);
    CHECK(ok == (msg == nullptr), "%d x %d -> %d x %d: %s", snx, sny, dnx, dny, msg ? msg : "allowed");
    if (ok && !msg) CHECK(got.rx == want.rx && got.ry == want.ry && got.dir == want.dir, "%d x %d -> %d x %d: (%d, %d, %d)", snx, sny, dnx, dny, got.rx, got.ry, got.dir);
    if (msg) CHECK(got.rx == -1 && got.ry == -1 && got.dir == -9, "a refusal leaves *f alone");
    ++n;
  }
  RegridFactors f{0, 0, 0};
  CHECK(regrid_factors(33, 17, 66, 51, &f) == nullptr && f.rx == 2 && f.ry == 3 && f.dir == 1, "refine (2, 3)");
  CHECK(regrid_factors(33, 17, 132, 136, &f) == nullptr && f.rx == 4 && f.ry == 8 && f.dir == 1, "refine (4, 8)");
  CHECK(regrid_factors(128, 128, 384, 128, &f) == nullptr && f.rx == 3 && f.ry == 1 && f.dir == 1, "refine along i only");
  CHECK(regrid_factors(128, 128, 32, 16, &f) == nullptr && f.rx == 4 && f.ry == 8 && f.dir == -1, "coarsen (4, 8)");
  CHECK(regrid_factors(33, 17, 11, 17, &f) == nullptr && f.rx == 3 && f.ry == 1 && f.dir == -1, "coarsen along i only");
  CHECK(regrid_factors(33, 17, 33, 17, &f) == nullptr && f.rx == 1 && f.ry == 1 && f.dir == 0, "the same grid");
  CHECK(regrid_factors(64, 64, 1024, 1024, &f) == nullptr && f.rx == 16, "the largest factor");
  CHECK(regrid_factors(64, 64, 1088, 64, &f) != nullptr && regrid_factors(1088, 64, 64, 64, &f) != nullptr, "a factor of 17");
  CHECK(regrid_factors(64, 64, 128, 32, &f) != nullptr && regrid_factors(64, 64, 32, 128, &f) != nullptr, "refined one way, coarsened the other");
  CHECK(regrid_factors(64, 64, 96, 64, &f) != nullptr && regrid_factors(96, 64, 64, 64, &f) != nullptr && regrid_factors(33, 17, 66, 50, &f) != nullptr, "no integer ratio");
  CHECK(regrid_factors(0, 64, 64, 64, &f) != nullptr && regrid_factors(64, 64, 64, -3, &f) != nullptr, "an extent < 1 (no division by it)");
  const int big = std::numeric_limits<int>::max();
  CHECK(regrid_factors(big, big, big, big, &f) == nullptr && f.dir == 0, "the largest grid onto itself");
  CHECK(regrid_factors(1, 1, big, big, &f) != nullptr && regrid_factors(big, 1, 1, big, &f) != nullptr, "the ends of the type");
  n += 14;

  // ---- the arguments
  const double L = 0.1, nan = std::numeric_limits<double>::quiet_NaN();
  CHECK(regrid_check(64, 64, L, L, 128, 128, L, L, VOF_REGRID_PLIC, 1e-6, &f) == nullptr && f.rx == 2 && f.ry == 2 && f.dir == 1, "a refinement with PLIC");
  CHECK(regrid_check(64, 64, L, L, 128, 128, L, L, 0, 1e-6, &f) == nullptr, "... without");
  for (int flags : {2, 3, 4, -1, 1 << 30}) CHECK(regrid_check(64, 64, L, L, 128, 128, L, L, flags, 1e-6, &f) != nullptr, "flags %d", flags);
  CHECK(regrid_check(64, 64, L, L, 128, 128, L * (1 + 1e-15), L, 0, 0.0, &f) != nullptr, "Lx differs in the last bits");
  CHECK(regrid_check(64, 64, L, L, 128, 128, L, 0.2, 0, 0.0, &f) != nullptr, "Ly differs");
  CHECK(regrid_check(64, 64, nan, L, 128, 128, nan, L, 0, 0.0, &f) != nullptr, "a NaN is equal to nothing");
  for (double eps : {-1e-300, 0.5, 1.0, nan}) {
    CHECK(regrid_check(64, 64, L, L, 128, 128, L, L, VOF_REGRID_PLIC, eps, &f) != nullptr, "eps %g with PLIC", eps);
    CHECK(regrid_check(64, 64, L, L, 128, 128, L, L, 0, eps, &f) == nullptr, "eps %g is not looked at without", eps);
  }
  for (double eps : {0.0, 1e-6, 0.4999}) CHECK(regrid_check(64, 64, L, L, 128, 128, L, L, VOF_REGRID_PLIC, eps, &f) == nullptr, "eps %g", eps);
  CHECK(regrid_check(64, 64, L, L, 128, 32, L, L, 0, 0.0, &f) != nullptr && regrid_check(64, 64, L, L, 1088, 64, L, L, 0, 0.0, &f) != nullptr, "the ratio is checked");
  n += 22;

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld regrid checks ok\n", n);
  return 0;
}
