// Stand-alone check (host compiler, no HIP) of runtime/rows.h and of the tile geometry in vof2d_device.h.
// Exit status 0 and "ok" on success; the first failing check is printed otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "runtime/rows.h"
#include "vof2d_device.h"

using namespace vof;

static int failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

static void cover(std::vector<int>& n, RowRange r, int base) {
  for (int i = r.first; i <= r.last; ++i) {
    if (i - base < 0 || i - base >= (int)n.size()) { ++failures; std::printf("FAIL row %d outside the stored rows\n", i); return; }
    n[i - base] += 1;
  }
}
static void cover(std::vector<int>& n, const PartRows& p, int base) { cover(n, p.band_lo, base); cover(n, p.band_hi, base); cover(n, p.body, base); }
static bool same(RowRange a, RowRange b) { return (a.empty() && b.empty()) || (a.first == b.first && a.last == b.last); }

// What the runtime computed before rows.h existed (transport_part, tm5_tm), written out: ranges {band_lo, band_hi, body}.
static PartRows parts_before(int row_lo, int row_hi, int own_lo, int own_hi, int nx, int iters, int part) {
  const int W = iters + 8;
  const int ilo = row_lo + 1 > 1 ? row_lo + 1 : 1, ihi = row_hi - 1 < nx ? row_hi - 1 : nx;
  const int lo = own_lo > ilo ? own_lo : ilo, hi = own_hi < ihi ? own_hi : ihi;
  const bool band_lo = row_lo != 0, band_hi = row_hi != nx + 1;
  const int in_lo = band_lo ? lo + W : lo, in_hi = band_hi ? hi - W : hi;
  const bool split = in_lo <= in_hi && (band_lo || band_hi);
  PartRows r{{1, 0}, {1, 0}, {1, 0}};
  if (part == 0 || !split) {
    if (part == 2 && (band_lo || band_hi)) return r;
    if (part == 1 && !(band_lo || band_hi)) return r;
    r.body = {lo, hi};
  } else if (part == 1) {
    if (band_lo) r.band_lo = {lo, in_lo - 1};
    if (band_hi) r.band_hi = {in_hi + 1, hi};
  } else {
    r.body = {in_lo, in_hi};
  }
  return r;
}

static void check_rows() {
  static_assert(VOF_HALO_ROWS(10) == 18, "halo rows");
  const int iters_of[3] = {5, 10, 20};
  for (int it = 0; it < 3; ++it) {
    const int iters = iters_of[it], W = VOF_HALO_ROWS(iters);
    for (int walls = 0; walls < 4; ++walls) {
      const bool wall_lo = walls & 1, wall_hi = walls & 2;
      for (int height = (W < 18 ? W : 18); height <= 3 * W + 1; ++height) {
        const int row_lo = wall_lo ? 0 : 100, own_lo = wall_lo ? 1 : row_lo + W, own_hi = own_lo + height - 1;
        const int nx = wall_hi ? own_hi : own_hi + 300, row_hi = wall_hi ? nx + 1 : own_hi + W;
        const StripRows s = strip_rows(row_lo, row_hi, own_lo, own_hi, nx, iters);
        CHECK(s.owned.first == own_lo && s.owned.last == own_hi, "owned %d..%d", s.owned.first, s.owned.last);
        CHECK(s.has_bands == !(wall_lo && wall_hi), "walls %d", walls);
        const int nbands = (wall_lo ? 0 : 1) + (wall_hi ? 0 : 1);
        CHECK(s.meet == (nbands > 0 && height <= nbands * W), "walls %d height %d W %d", walls, height, W);
        std::vector<int> n(row_hi - row_lo + 1, 0);
        // bands plus rest cover each owned row exactly once (where the bands meet there are neither: all is one range)
        if (s.meet) {
          CHECK(s.band_lo.empty() && s.band_hi.empty() && s.rest.empty(), "walls %d height %d", walls, height);
        } else {
          cover(n, s.band_lo, row_lo); cover(n, s.band_hi, row_lo); cover(n, s.rest, row_lo);
          for (int i = row_lo; i <= row_hi; ++i) CHECK(n[i - row_lo] == (i >= own_lo && i <= own_hi ? 1 : 0), "row %d walls %d height %d", i, walls, height);
          // bands are W rows, next to the interior edges only
          CHECK(s.band_lo.rows() == (wall_lo ? 0 : W) && s.band_hi.rows() == (wall_hi ? 0 : W), "walls %d height %d", walls, height);
          CHECK(wall_lo || s.band_lo.first == own_lo, "lower band"); CHECK(wall_hi || s.band_hi.last == own_hi, "upper band");
        }
        // parts "bands" and "rest" together are part "all": every owned row once
        const PartRows all = part_rows(s, kAllOwned), bands = part_rows(s, kEdgeBands), rest = part_rows(s, kRest);
        CHECK(all.band_lo.empty() && all.band_hi.empty() && same(all.body, s.owned), "part all");
        std::vector<int> m(row_hi - row_lo + 1, 0);
        cover(m, bands, row_lo); cover(m, rest, row_lo);
        for (int i = row_lo; i <= row_hi; ++i) CHECK(m[i - row_lo] == (i >= own_lo && i <= own_hi ? 1 : 0), "parts: row %d walls %d height %d", i, walls, height);
        // a full domain has no bands: everything is rest; meeting bands: everything is bands
        if (!s.has_bands) CHECK(bands.empty() && same(rest.body, s.owned), "full domain");
        if (s.meet) CHECK(rest.empty() && same(bands.body, s.owned) && bands.band_lo.empty() && bands.band_hi.empty(), "meeting bands");
        // ... and each part is what the runtime launched before
        for (int part = 0; part < 3; ++part) {
          const PartRows a = part_rows(s, part), b = parts_before(row_lo, row_hi, own_lo, own_hi, nx, iters, part);
          CHECK(same(a.band_lo, b.band_lo) && same(a.band_hi, b.band_hi) && same(a.body, b.body), "part %d walls %d height %d iters %d", part, walls, height, iters);
        }
      }
    }
  }
}

// Tile counts at ny = k * stride and k * stride + 1 against the formulas the launch wrappers carried, written out.
template <typename G>
static void check_family(const char* name, int stride, int (*before)(int)) {
  CHECK(G::STRIDE == stride, "%s stride %d", name, G::STRIDE);
  CHECK(G::W == 128 && G::W - 2 * G::H == G::STRIDE, "%s", name);
  for (int k = 1; k <= 80; ++k)
    for (int ny = k * stride; ny <= k * stride + 1; ++ny) {
      CHECK(G::tiles(ny) == before(ny), "%s ny %d: %d tiles, %d before", name, ny, G::tiles(ny), before(ny));
      CHECK(G::tiles(ny) == (ny == k * stride ? k : k + 1), "%s ny %d", name, ny);
    }
  for (int ny = 3; ny <= 1000; ++ny) CHECK(G::tiles(ny) == before(ny), "%s ny %d", name, ny);
}
template <int TS, bool SQ>
static int tb_before(int ny) {
  const int VV = 2, Wt = 64 * VV;
  const bool sq = SQ;
  const int Ht = ((TS - 1 + (sq ? 1 : 0) + VV - 1) / VV) * VV, ST = Wt - 2 * Ht;
  return (ny + ST - 1) / ST;
}
static void check_geometry() {
  check_family<MomentumGeom<2>>("momentum", 124, [](int ny) { const int Wt = 64 * 2, Ht = 2, ST = Wt - 2 * Ht; return (ny + ST - 1) / ST; });
  check_family<TransportGeom<2>>("transport / fct_y", 112, [](int ny) { const int W = 64 * 2; return (ny + (W - 2 * 8) - 1) / (W - 2 * 8); });
  check_family<TmGeom<2>>("tm", 112, [](int ny) { const int ST = 64 * 2 - 2 * 8; return (ny + ST - 1) / ST; });
  check_family<JacobiTbGeom<2, 5, true>>("jacobi_tb<5> square", 116, tb_before<5, true>);
  check_family<JacobiTbGeom<2, 5, false>>("jacobi_tb<5> general", 120, tb_before<5, false>);
  check_family<JacobiTbGeom<2, 2, true>>("jacobi_tb<2> square", 124, tb_before<2, true>);
  check_family<JacobiTbGeom<2, 2, false>>("jacobi_tb<2> general", 124, tb_before<2, false>);
  check_family<JacobiPairGeom<2, 5>>("jacobi_pair<5>", 108, [](int ny) { const int VV = 2, ST = 64 * VV - 2 * (((2 * 5 + VV - 1) / VV) * VV); return (ny + ST - 1) / ST; });
}

int main() {
  check_rows();
  check_geometry();
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
