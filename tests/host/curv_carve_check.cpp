// tests/host/curv_carve_check.cpp -- the arena of vof_curvature and vof_interface (carve_cell_rows of runtime/carve.h, plain C++): the ranges
// are consecutive, aligned, do not overlap and hold what the launches of runtime/cell_rows.h write there, over grids and chunk lengths.
#include <stdio.h>

#include "runtime/carve.h"
#include "runtime/rows.h"

using namespace vof;

#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      printf("FAILED %s: ", #cond);               \
      printf(__VA_ARGS__);                        \
      printf("\n");                               \
      return 1;                                   \
    }                                             \
  } while (0)

int main() {
  const int widths[][2] = {{10, 16}, {2, 4}};   // CVP_N, CVS_N of kernels/curvature.h; kIfacePart, IFS_N of kernels/interface.h
  const int grids[][2] = {{3, 3}, {3, 129}, {33, 17}, {24, 40}, {48, 80}, {31, 129}, {200, 200}, {4096, 4096}, {3277, 513}};
  for (const auto& gr : grids) {
    const int nx = gr[0], ny = gr[1], ntj = (ny + 127) / 128;
    const ReportedRows rep = reported_rows(0, nx + 1, 1, nx, nx, ny, ntj);
    const int R = cells_per_wave_rows(nx, ntj, 4, 32);
    const size_t entries = (size_t)rep.entries(), blocks = rep.blocks(R);
    for (const auto& w : widths) {
      const int kPart = w[0], kSum = w[1];
      const CellRowsCarve c = carve_cell_rows(entries, blocks * kPart, kSum);
      CHECK(c.cnt == 0 && c.part >= (entries + 1) * sizeof(int) && c.part % sizeof(double) == 0, "%d x %d: part at %zu", nx, ny, c.part);
      CHECK(c.part - (entries + 1) * sizeof(int) < sizeof(double), "%d x %d: a gap in front of the partials", nx, ny);
      CHECK(c.sum == c.part + blocks * kPart * sizeof(double), "%d x %d: sum at %zu", nx, ny, c.sum);
      CHECK(c.total == c.sum + kSum * sizeof(double), "%d x %d: total %zu", nx, ny, c.total);
    }
    CHECK(blocks * 4 >= (size_t)((nx + R - 1) / R) * ntj, "%d x %d: a wave without a block", nx, ny);
  }
  printf("ok\n");
  return 0;
}
