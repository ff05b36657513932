// Stand-alone check (host compiler, no HIP) of what vof_depths lays out on the host: the chunk rule (depths_chunk_rows,
// runtime/rows.h) against the cells-per-wave rule written out below, the partial counts and launch sizes (depths_geom) against
// the expressions kernels/depths.h indexes with, and the arena (carve_depths, runtime/carve.h): every range aligned, in
// order, disjoint, inside the total, and the integer range zeroed in front of a pass exactly top[rows] and the two words.
// Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <cstdio>

#include "runtime/carve.h"
#include "runtime/rows.h"

using namespace vof;

static int failures = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

static const int W = 128;   // columns of a wave tile (vof2d_device.h: V = 2)

// the cells-per-wave rule as runtime/launches.h has it (chunk_rows), with 2 and 32
static int rule(long rows, int ntiles) {
  long R = rows * ntiles / 4096;
  if (R < 2) R = 2;
  if (R > 32) R = 32;
  long P = 1;
  while (P * 2 <= R) P *= 2;
  return (int)(P < 2 ? 2 : P);
}

static void check_handle(int nx, int ny, size_t esz, int row_lo, int row_hi, int own_lo, int own_hi) {
  const char* const fmt = "%dx%d esz %zu rows %d..%d own %d..%d";
#define CTX fmt, nx, ny, esz, row_lo, row_hi, own_lo, own_hi
  const int ntj = (ny + W - 1) / W;   // (the same for both precisions: V = 2 elements per lane whatever their size)
  const int ilo = row_lo + 1 > 1 ? row_lo + 1 : 1, ihi = row_hi - 1 < nx ? row_hi - 1 : nx;
  const int lo = own_lo > ilo ? own_lo : ilo, hi = own_hi < ihi ? own_hi : ihi;
  const int rows = hi < lo ? 0 : hi - lo + 1;
  const ReportedRows rep = reported_rows(row_lo, row_hi, own_lo, own_hi, nx, ny, ntj);
  // ---- the chunk rule: on the computable rows, whatever the handle owns of them; a power of two in [2, 32]
  const int R = depths_chunk_rows(row_lo, row_hi, nx, ntj);
  CHECK(R == rule(ihi - ilo + 1, ntj) && R >= 2 && R <= 32 && (R & (R - 1)) == 0, CTX);
  CHECK(cells_per_wave_rows(ihi - ilo + 1, ntj, 2, 16) == (R > 16 ? 16 : R), CTX);   // (the diagnostics' rule differs in the cap alone)
  // ---- the partial counts and the launches
  const DepthsGeom dg = depths_geom(rep, R);
  const int chunks = (rows + R - 1) / R;
  CHECK(dg.R == R && dg.chunks == chunks && dg.row_partials == (int64_t)rows * ntj && dg.col_partials == (int64_t)chunks * ny, CTX);
  CHECK(dg.blocks == (unsigned)(((long)chunks * ntj + 3) / 4) && (dg.blocks == 0) == (rows == 0), CTX);
  CHECK((long)dg.blocks * 4 >= (long)chunks * ntj && (long)(dg.blocks ? dg.blocks - 1 : 0) * 4 < (long)chunks * ntj + (rows == 0), CTX);
  CHECK((long)dg.row_blocks * 256 >= rows && (long)dg.col_blocks * 256 >= ny && dg.col_blocks >= 1, CTX);
  CHECK((rows == 0) == (dg.row_blocks == 0), CTX);
  // the last wave's last indices stay inside the partials (k_depths: r * ntj + tj, ch * ny + j - 1)
  if (rows) {
    CHECK((int64_t)(rows - 1) * ntj + (ntj - 1) == dg.row_partials - 1, CTX);
    CHECK((int64_t)((rows - 1) / R) * ny + (ny - 1) == dg.col_partials - 1, CTX);
    CHECK((ntj - 1) * W + 1 <= ny && ntj * W >= ny, CTX);
  }
  // ---- the arena
  const DepthsCarve c = carve_depths((size_t)rows, (size_t)ny, (size_t)dg.row_partials, (size_t)dg.col_partials);
  const size_t D = sizeof(double);
  CHECK(c.rowpart == 0 && c.colpart == (size_t)dg.row_partials * D && c.depth_i == c.colpart + (size_t)dg.col_partials * D, CTX);
  CHECK(c.depth_j == c.depth_i + (size_t)rows * D && c.sum == c.depth_j + (size_t)ny * D && c.top == c.sum + 8 * D, CTX);
  CHECK(c.top_bytes == ((size_t)rows + 2) * sizeof(int) && c.total == c.top + c.top_bytes, CTX);
  CHECK(c.colpart % 8 == 0 && c.depth_i % 8 == 0 && c.depth_j % 8 == 0 && c.sum % 8 == 0 && c.top % 4 == 0, CTX);
#undef CTX
}

int main() {
  const int sizes[9] = {3, 4, 17, 33, 64, 130, 260, 516, 1100};
  const int Wh = VOF_HALO_ROWS(10);
  long handles = 0;
  // the rule itself at the sizes the tests and the profiles name
  CHECK(depths_chunk_rows(0, 34, 33, 1) == 2 && depths_chunk_rows(0, 1101, 1100, 2) == 2 && depths_chunk_rows(0, 2049, 2048, 16) == 8 &&
        depths_chunk_rows(0, 4097, 4096, 32) == 32 && depths_chunk_rows(0, 8193, 8192, 64) == 32 && depths_chunk_rows(0, 1025, 1024, 8) == 2,
        "the chunk lengths of the named grids");
  for (int nx : sizes)
    for (int ny : sizes)
      for (size_t esz : {(size_t)8, (size_t)4}) {
        check_handle(nx, ny, esz, 0, nx + 1, 1, nx);
        ++handles;
        for (int n = 2; n <= 3; ++n)   // strips with halo rows, as the tests cut them
          for (int k = 0; k < n; ++k) {
            const int b0 = (int)((double)k * nx / n + 0.5), b1 = (int)((double)(k + 1) * nx / n + 0.5);
            const int row_lo = b0 + 1 - Wh > 0 ? b0 + 1 - Wh : 0, row_hi = b1 + Wh < nx + 1 ? b1 + Wh : nx + 1;
            if (row_hi - row_lo < 2) continue;
            check_handle(nx, ny, esz, row_lo, row_hi, b0 + 1, b1);
            ++handles;
          }
        // no owned row left inside the computable rows: above them, below them, an empty range to begin with
        check_handle(nx, ny, esz, 0, 2, 2, 3);
        check_handle(nx, ny, esz, nx - 1, nx + 1, nx - 2, nx - 1);
        check_handle(nx, ny, esz, 0, nx + 1, 2, 1);
        handles += 3;
      }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld handles ok\n", handles);
  return 0;
}
