// Stand-alone check (host compiler, no HIP) of what vof_frame lays out on the host: the frame geometry (frame_geom,
// runtime/rows.h) -- pw, ph, the chunk rule, the launch sizes -- against the expressions written out below, every index
// k_frame_cols, k_frame_fold and k_frame_paint form (kernels/frames.h) against the ranges they index, and the arena
// (carve_frame, runtime/carve.h): every range aligned, in order, disjoint, inside the total, the results consecutive.
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

static void check_frame(int nx, int ny, int bx, int by) {
  const char* const fmt = "%dx%d block %dx%d";
#define CTX fmt, nx, ny, bx, by
  const int ntj = (ny + W - 1) / W;
  const FrameGeom f = frame_geom(nx, ny, ntj, W, bx, by);
  // ---- blocks beyond the grid count as the grid; the picture
  const int ex = bx < nx ? bx : nx, ey = by < ny ? by : ny;
  CHECK(f.bx == ex && f.by == ey, CTX);
  CHECK(f.pw == (nx + ex - 1) / ex && f.ph == (ny + ey - 1) / ey && f.pw >= 1 && f.ph >= 1, CTX);
  CHECK((long)(f.pw - 1) * ex < nx && (long)f.pw * ex >= nx && (long)(f.ph - 1) * ey < ny && (long)f.ph * ey >= ny, CTX);   // the last pixel has a cell, no cell is left out
  if (bx >= nx) CHECK(f.pw == 1, CTX);
  if (by >= ny) CHECK(f.ph == 1, CTX);
  CHECK(f.pixels == (int64_t)f.pw * f.ph && f.pixel_blocks == (unsigned)((f.pixels + 255) / 256 < 256 ? (f.pixels + 255) / 256 : 256) && f.pixel_blocks >= 1, CTX);
  // ---- the chunk rule: whole pixel rows, K of them
  const int len = rule(nx, ntj);
  const int K = len / ex > 1 ? len / ex : 1;
  CHECK(f.K == K && f.R == K * ex && f.R % ex == 0 && f.chunks == (f.pw + K - 1) / K, CTX);
  CHECK((long)(f.chunks - 1) * f.R < nx && (long)f.chunks * f.R >= nx, CTX);             // the last chunk has a row, every row a chunk
  CHECK(f.cols_blocks == (unsigned)(((long)f.chunks * ntj + 3) / 4) && (long)f.cols_blocks * 4 >= (long)f.chunks * ntj, CTX);
  // a wave past the last chunk starts past nx: it returns (cell_tile of kernels/cells.h)
  CHECK(1 + (long)f.chunks * f.R > nx, CTX);
  // ---- what k_frame_cols indexes: the pixel row of a chunk's first and last row, the last lane's vector in the padded row
  for (int ch = 0; ch < f.chunks; ch += (f.chunks > 64 ? f.chunks / 7 + 1 : 1)) {
    const int ra = 1 + ch * f.R, rb = ra + f.R - 1 < nx ? ra + f.R - 1 : nx;
    CHECK((ra - 1) / ex == ch * K && (rb - 1) / ex < f.pw && (ra - 1) % ex == 0, CTX);
  }
  CHECK(f.cpitch == ntj * W && f.cpitch >= ny && f.cpitch % 2 == 0 && f.col_partials == (int64_t)f.pw * f.cpitch, CTX);
  const int j0_last = 1 + (ntj - 1) * W + 63 * 2;
  CHECK((int64_t)(f.pw - 1) * f.cpitch + (j0_last - 1) + 1 == f.col_partials - 1, CTX);
  // ---- k_frame_fold: the columns and rows of the last pixel
  CHECK((f.ph - 1) * ey < ny && (f.pw - 1) * ex < nx, CTX);
  // ---- the arena, with and without the means of F beside the quantity's
  for (int beside = 0; beside < 2; ++beside) {
    const size_t fp = beside ? (size_t)f.col_partials : 0, fx = beside ? (size_t)f.pixels : 0;
    const FrameCarve c = carve_frame((size_t)f.col_partials, (size_t)f.pixels, fp, fx);
    const size_t D = sizeof(double);
    CHECK(c.colq == 0 && c.colF == (size_t)f.col_partials * D && c.colF % 16 == 0 && c.mF == c.colF + fp * D && c.mF % 8 == 0, CTX);
    CHECK(c.words == c.mF + fx * D && c.words % 8 == 0 && c.words_bytes == 32, CTX);
    CHECK(c.means == c.words + c.words_bytes && c.sum == c.means + (size_t)f.pixels * D && c.rgb == c.sum + 8 * D, CTX);
    CHECK(c.rgb_bytes == (size_t)f.pixels * 3 && c.total == c.rgb + c.rgb_bytes, CTX);
  }
#undef CTX
}

int main() {
  const int sizes[10] = {3, 4, 7, 17, 33, 128, 129, 131, 300, 1100};
  const int blocks[8] = {1, 2, 3, 4, 7, 8, 16, 100};
  long frames = 0;
  for (int nx : sizes)
    for (int ny : sizes) {
      for (int bx : blocks)
        for (int by : blocks) { check_frame(nx, ny, bx, by); ++frames; }
      check_frame(nx, ny, nx + 5, 1); check_frame(nx, ny, 1, ny + 5); check_frame(nx, ny, nx, ny); check_frame(nx, ny, 0x7fffffff, 0x7fffffff);
      frames += 4;
    }
  // the grids the profiles name: 32-row lengths, 4 pixel rows of 8 or 8 of 4 a chunk
  {
    const FrameGeom f = frame_geom(4096, 4096, 32, W, 8, 8);
    CHECK(f.pw == 512 && f.ph == 512 && f.K == 4 && f.R == 32 && f.chunks == 128 && f.cols_blocks == 1024, "4096^2 at 8 x 8");
    const FrameGeom g = frame_geom(4096, 4096, 32, W, 4, 4);
    CHECK(g.pw == 1024 && g.K == 8 && g.R == 32 && g.chunks == 128, "4096^2 at 4 x 4");
    const FrameGeom s = frame_geom(7, 131, 2, W, 1, 1);
    CHECK(s.R == 2 && s.chunks == 4 && s.pw == 7 && s.ph == 131 && s.cpitch == 256, "7 x 131 at 1 x 1: three chunks and a remainder");
    check_frame(4096, 4096, 8, 8); check_frame(8192, 8192, 8, 8); check_frame(8192, 8192, 1, 1);
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld frames ok\n", frames);
  return 0;
}
