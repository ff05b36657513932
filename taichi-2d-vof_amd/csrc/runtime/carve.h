// runtime/carve.h -- one allocation cut into consecutive, aligned ranges; the arenas of the verbs cut that way
//
// Plain C++ (no HIP): runtime/buffers.h includes it, the CPU tests compile it on its own.  All figures are bytes.
#pragma once
#include <stddef.h>

#include <array>
#include <vector>

namespace vof {

struct Carve {
  size_t total = 0;
  size_t take(size_t bytes, size_t align = 1) {   // the offset of the range
    const size_t at = (total + align - 1) / align * align;
    total = at + bytes;
    return at;
  }
  size_t ints(size_t n) { return take(n * sizeof(int)); }
  size_t doubles(size_t n) { return take(n * sizeof(double), sizeof(double)); }
};

// vof_solve_p_cg, two allocations: r, two direction arrays (ping-pong), q in the fields' layout; one partial per block, then the scalars
struct CgCarve { size_t fld[4], fields_total, sc, part_total; };
inline CgCarve carve_cg(size_t field_bytes, size_t part_doubles, size_t scalars) {
  CgCarve c;
  Carve fields, part;
  for (size_t& f : c.fld) f = fields.take(field_bytes);
  part.doubles(part_doubles);
  c.sc = part.doubles(scalars);
  c.fields_total = fields.total; c.part_total = part.total;
  return c;
}

// vof_solve_p_mg: e (two), f of every level >= 1; r, two directions, q of the coarsest-level solve, sized for level 1; its scalars.
// level_bytes[l] is one array of level l (entry 0, the grid, has none here); at least two levels.
struct MgCarve { std::vector<std::array<size_t, 3>> level; size_t cgw[4], sc, total; };
inline MgCarve carve_mg(const std::vector<size_t>& level_bytes, size_t scalars) {
  MgCarve c{std::vector<std::array<size_t, 3>>(level_bytes.size()), {}, 0, 0};
  Carve a;
  for (size_t l = 1; l < level_bytes.size(); ++l)
    for (size_t& at : c.level[l]) at = a.take(level_bytes[l]);
  for (size_t& w : c.cgw) w = a.take(level_bytes[1]);
  c.sc = a.doubles(scalars);
  c.total = a.total;
  return c;
}

// vof_interface, vof_curvature (runtime/cell_rows.h): the count of every (row, column tile) and one spare int; the block partials; the summary
struct CellRowsCarve { size_t cnt, part, sum, total; };
inline CellRowsCarve carve_cell_rows(size_t entries, size_t part_doubles, size_t summary_doubles) {
  Carve a;
  const size_t cnt = a.ints(entries + 1), part = a.doubles(part_doubles), sum = a.doubles(summary_doubles);
  return {cnt, part, sum, a.total};
}

// vof_blobs: parent, then label, of every cell; the blob index of every root; the root count of every (row, column tile),
// two ints of k_blob_stats and one spare; 8 doubles (the summary, the total of a scan)
struct BlobCarve { size_t lab, idx, cnt, sum, total; };
inline BlobCarve carve_blobs(size_t cells, size_t entries) {
  Carve a;
  const size_t lab = a.ints(cells), idx = a.ints(cells), cnt = a.ints(entries + 3), sum = a.doubles(8);
  return {lab, idx, cnt, sum, a.total};
}

// vof_depths: the partials per (row, tile) and per (chunk, column); depth_i, depth_j and the summary; top of every row and the two
// integer words of the fronts behind it (zeroed as one range)
struct DepthsCarve { size_t rowpart, colpart, depth_i, depth_j, sum, top, top_bytes, total; };
inline DepthsCarve carve_depths(size_t rows, size_t ny, size_t row_partials, size_t col_partials) {
  Carve a;
  DepthsCarve c;
  c.rowpart = a.doubles(row_partials); c.colpart = a.doubles(col_partials);
  c.depth_i = a.doubles(rows); c.depth_j = a.doubles(ny); c.sum = a.doubles(8);
  c.top_bytes = (rows + 2) * sizeof(int);
  c.top = a.ints(rows + 2);
  c.total = a.total;
  return c;
}

// vof_frame: the column partials of the quantity and, where the contour needs them beside it (f_partials, f_pixels: 0 otherwise),
// of F; the means of F; the integer words (zeroed as one range in front of a pass); then what a call copies out, consecutive:
// the means, the summary, three bytes a pixel
struct FrameCarve { size_t colq, colF, mF, words, words_bytes, means, sum, rgb, rgb_bytes, total; };
inline FrameCarve carve_frame(size_t col_partials, size_t pixels, size_t f_partials, size_t f_pixels) {
  Carve a;
  FrameCarve c;
  c.colq = a.take(col_partials * sizeof(double), 16); c.colF = a.take(f_partials * sizeof(double), 16);
  c.mF = a.doubles(f_pixels);
  c.words_bytes = 4 * sizeof(unsigned long long);
  c.words = a.take(c.words_bytes, sizeof(unsigned long long));
  c.means = a.doubles(pixels); c.sum = a.doubles(8);
  c.rgb_bytes = pixels * 3;
  c.rgb = a.take(c.rgb_bytes);
  c.total = a.total;
  return c;
}

// vof_stats_*: one plane of doubles per accumulator of the groups chosen by `mask` (bit 0: the nine moments, bit 1: the four of the
// envelope), in slot order; a plane is `rows` rows of `pitch` doubles, the pitch a whole number of wave tiles so that a lane's columns
// are one aligned 16-byte vector and no lane of a launch leaves its row.  A plane of a group that is off has no range (kNoRange).
// Behind the planes: the block partials of k_stats_summary, its two results.
constexpr int kStatsPlanes = 13, kStatsMomentPlanes = 9;
constexpr size_t kNoRange = ~(size_t)0;
inline size_t stats_pitch(size_t ny, size_t tile_cols) { return (ny + tile_cols - 1) / tile_cols * tile_cols; }
struct StatsCarve { size_t plane[kStatsPlanes], plane_bytes, planes_total, part, sum, total; };
inline StatsCarve carve_stats(size_t rows, size_t pitch, int mask, size_t part_doubles) {
  Carve a;
  StatsCarve c;
  c.plane_bytes = rows * pitch * sizeof(double);
  for (int k = 0; k < kStatsPlanes; ++k) c.plane[k] = (mask & (k < kStatsMomentPlanes ? 1 : 2)) ? a.take(c.plane_bytes, 16) : kNoRange;
  c.planes_total = a.total;
  c.part = a.take(part_doubles * sizeof(double), 16);
  c.sum = a.take(2 * sizeof(double), 16);
  c.total = a.total;
  return c;
}

}  // namespace vof
