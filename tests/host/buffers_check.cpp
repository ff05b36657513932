// Stand-alone check (host compiler, no HIP) of the cells a handle reports (ReportedRows, runtime/rows.h) and of the arenas of
// the verbs (runtime/carve.h) against what the runtime computed before they existed: diag_rows_of, iface_entries, blob_cells
// and the blocks of their launches; the offsets and totals of iface_prepare (now cell_rows_prepare), blobs_prepare, cg_prepare and mg_prepare,
// written out below.  Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <cstdio>
#include <vector>

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

// the constants of the kernels (kernels/cg.h, diag.h, interface.h) and of the layout (vof2d_device.h: V = 2)
static const int kCgPart = 3, CG_NSCAL = 16, kIfacePart = 2, IFS_N = 4, kDiagPart = 10, W = 128;

struct Handle {   // what vof_create derives from the description
  int nx, ny, row_lo, row_hi, own_lo, own_hi, ilo, ihi, ntj;
  size_t esz, pitch, field_elems;
};
static size_t pitch_of(int ny, size_t esz) {
  const size_t align = 128 / esz, col0 = align - 1, maxcol = (size_t)ny + W + 16;
  return ((col0 + maxcol + 1 + align - 1) / align) * align;
}
static Handle handle(int nx, int ny, size_t esz, int row_lo, int row_hi, int own_lo, int own_hi) {
  Handle h{nx, ny, row_lo, row_hi, own_lo, own_hi, row_lo + 1 > 1 ? row_lo + 1 : 1, row_hi - 1 < nx ? row_hi - 1 : nx, (ny + W - 1) / W, esz, 0, 0};
  h.pitch = pitch_of(ny, esz);
  h.field_elems = (size_t)(row_hi - row_lo + 1) * h.pitch + 128 / esz;
  return h;
}
// runtime/launches.h
static int chunk_rows(const Handle& h, int ntiles, int rmin, int rmax) {
  const long rows = h.ihi - h.ilo + 1;
  long R = rows * ntiles / 4096;
  if (R < rmin) R = rmin;
  if (R > rmax) R = rmax;
  long P = 1;
  while (P * 2 <= R) P *= 2;
  return (int)(P < rmin ? rmin : P);
}
static unsigned blocks_rows(int rows, int ntiles, int R) {
  const long waves = (long)((rows + R - 1) / R) * ntiles;
  return (unsigned)((waves + 3) / 4);
}

static void check_handle(const Handle& h, bool whole) {
  const char* const fmt = "%dx%d esz %zu rows %d..%d own %d..%d";
#define CTX fmt, h.nx, h.ny, h.esz, h.row_lo, h.row_hi, h.own_lo, h.own_hi
  // ---- the reported cells, as diag_rows_of, diag_blocks, iface_blocks, iface_entries, blob_cells and diag_launch had them
  const int lo = h.own_lo > h.ilo ? h.own_lo : h.ilo, hi = h.own_hi < h.ihi ? h.own_hi : h.ihi;
  const int diag_chunk = chunk_rows(h, h.ntj, 2, 16), iface_chunk = chunk_rows(h, h.ntj, 4, 32);
  const unsigned diag_blocks = hi < lo ? 0u : blocks_rows(hi - lo + 1, h.ntj, diag_chunk);
  const unsigned iface_blocks = hi < lo ? 0u : blocks_rows(hi - lo + 1, h.ntj, iface_chunk);
  const int64_t entries = hi < lo ? 0 : (int64_t)(hi - lo + 1) * h.ntj;
  const int64_t cells = hi < lo ? 0 : (int64_t)(hi - lo + 1) * h.ny;
  const double diag_cells = hi < lo ? 0.0 : (double)(hi - lo + 1) * (double)h.ny;
  const ReportedRows rep = reported_rows(h.row_lo, h.row_hi, h.own_lo, h.own_hi, h.nx, h.ny, h.ntj);
  CHECK(rep.range.first == lo && rep.range.last == hi, CTX);   // (what the launches get as g.ilo, g.ihi: also where there are no rows)
  CHECK(rep.rows() == (hi < lo ? 0 : hi - lo + 1) && rep.cells() == cells && rep.entries() == entries, CTX);
  CHECK((double)rep.cells() == diag_cells, CTX);
  CHECK(rep.blocks(diag_chunk) == diag_blocks && rep.blocks(iface_chunk) == iface_blocks, CTX);
  for (int it = 0; it <= 20; it += 5)
    CHECK(strip_rows(h.row_lo, h.row_hi, h.own_lo, h.own_hi, h.nx, it).owned.first == lo && strip_rows(h.row_lo, h.row_hi, h.own_lo, h.own_hi, h.nx, it).owned.last == hi, CTX);

  // ---- cell_rows_prepare with the widths of vof_interface: ints, then doubles
  {
    const size_t ints = ((size_t)entries + 2) & ~(size_t)1, dbl = (size_t)iface_blocks * kIfacePart + IFS_N;
    const CellRowsCarve c = carve_cell_rows((size_t)rep.entries(), (size_t)rep.blocks(iface_chunk) * kIfacePart, IFS_N);
    CHECK(c.cnt == 0 && c.part == ints * sizeof(int) && c.total == ints * sizeof(int) + dbl * sizeof(double), CTX);
    CHECK(c.part % 8 == 0 && c.part >= ((size_t)entries + 1) * sizeof(int), CTX);
    CHECK(c.sum == c.part + (size_t)iface_blocks * kIfacePart * sizeof(double), CTX);   // the summary directly behind the partials
  }
  // ---- blobs_prepare
  {
    const size_t n = (size_t)cells, ints = (2 * n + (size_t)entries + 4) & ~(size_t)1;
    const BlobCarve c = carve_blobs((size_t)rep.cells(), (size_t)rep.entries());
    CHECK(c.lab == 0 && c.idx == n * sizeof(int) && c.cnt == 2 * n * sizeof(int) && c.sum == ints * sizeof(int), CTX);
    CHECK(c.total == ints * sizeof(int) + 8 * sizeof(double) && c.sum % 8 == 0, CTX);
    CHECK(c.sum >= c.cnt + ((size_t)entries + 2) * sizeof(int), CTX);   // the counts and the two ints of k_blob_stats fit in front of the doubles
  }
  // ---- diag_prepare (one range: nothing to cut; the count of partials)
  CHECK((size_t)rep.blocks(diag_chunk) * kDiagPart + 1 == (size_t)diag_blocks * kDiagPart + 1, CTX);
  if (!whole) return;
  // ---- cg_prepare
  const size_t fbytes = h.field_elems * h.esz;
  {
    const size_t nblocks = blocks_rows(h.ihi - h.ilo + 1, h.ntj, 1), pbytes = (nblocks * kCgPart + CG_NSCAL) * sizeof(double);
    const CgCarve c = carve_cg(fbytes, nblocks * kCgPart, CG_NSCAL);
    for (size_t k = 0; k < 4; ++k) CHECK(c.fld[k] == k * fbytes && c.fld[k] % 128 == 0, CTX);
    CHECK(c.fields_total == 4 * fbytes && c.part_total == pbytes && c.sc == nblocks * kCgPart * sizeof(double) && c.sc % 8 == 0, CTX);
  }
  // ---- mg_prepare
  {
    std::vector<size_t> bytes{fbytes};
    const size_t align = 128 / h.esz;
    size_t total = 0;
    for (int nx = h.nx, ny = h.ny; !(nx % 2 || ny % 2 || nx / 2 < 4 || ny / 2 < 4);) {
      nx /= 2; ny /= 2;
      bytes.push_back(((size_t)(nx + 2) * pitch_of(ny, h.esz) + align) * h.esz);
      total += 3 * bytes.back();
    }
    if (bytes.size() > 1) {
      total += 4 * bytes[1] + CG_NSCAL * sizeof(double);
      const MgCarve c = carve_mg(bytes, CG_NSCAL);
      size_t at = 0;
      for (size_t l = 1; l < bytes.size(); ++l) {
        CHECK(c.level[l][0] == at && c.level[l][1] == at + bytes[l] && c.level[l][2] == at + 2 * bytes[l] && at % 128 == 0 && bytes[l] % 128 == 0, CTX);
        at += 3 * bytes[l];
      }
      for (size_t k = 0; k < 4; ++k) { CHECK(c.cgw[k] == at && at % 128 == 0, CTX); at += bytes[1]; }
      CHECK(c.sc == at && c.sc % 8 == 0 && c.total == total && c.total == at + CG_NSCAL * sizeof(double), CTX);
    }
  }
#undef CTX
}

static void check_carve() {
  Carve a;
  CHECK(a.take(5) == 0 && a.take(3) == 5 && a.ints(1) == 8 && a.doubles(2) == 16 && a.total == 32, "consecutive, aligned up");
  CHECK(a.ints(3) == 32 && a.doubles(1) == 48 && a.take(0, 128) == 128 && a.total == 128, "the padding of an odd count of ints");
}

int main() {
  const int sizes[8] = {3, 4, 17, 33, 64, 130, 260, 516};
  const int Wh = VOF_HALO_ROWS(10);
  long handles = 0;
  check_carve();
  for (int nx : sizes)
    for (int ny : sizes)
      for (size_t esz : {(size_t)8, (size_t)4}) {
        check_handle(handle(nx, ny, esz, 0, nx + 1, 1, nx), true);
        ++handles;
        for (int n = 2; n <= 3; ++n)   // strips with halo rows, as the tests cut them
          for (int k = 0; k < n; ++k) {
            const int b0 = (int)((double)k * nx / n + 0.5), b1 = (int)((double)(k + 1) * nx / n + 0.5);
            const int row_lo = b0 + 1 - Wh > 0 ? b0 + 1 - Wh : 0, row_hi = b1 + Wh < nx + 1 ? b1 + Wh : nx + 1;
            if (row_hi - row_lo < 2) continue;
            check_handle(handle(nx, ny, esz, row_lo, row_hi, b0 + 1, b1), false);
            ++handles;
          }
        // no owned row left inside the computable rows: above them, below them, an empty range to begin with
        check_handle(handle(nx, ny, esz, 0, 2, 2, 3), false);
        check_handle(handle(nx, ny, esz, nx - 1, nx + 1, nx - 2, nx - 1), false);
        check_handle(handle(nx, ny, esz, 0, nx + 1, 2, 1), false);
        handles += 3;
      }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("%ld handles ok\n", handles);
  return 0;
}
