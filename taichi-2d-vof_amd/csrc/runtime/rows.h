// runtime/rows.h -- the rows of a strip: what it owns, the bands at its interior edges, the rest, and which of them
// a launch of one part gets
//
// Plain C++ (no HIP): the host runtime includes it through schedule.h, the CPU tests compile it on its own.
#pragma once
#include <stdint.h>

#include "../../../include/vof2d.h"

namespace vof {

struct RowRange {
  int first, last;   // inclusive; last < first: no rows
  bool empty() const { return last < first; }
  int rows() const { return empty() ? 0 : last - first + 1; }
};
constexpr RowRange kNoRows{1, 0};

// A handle stores rows row_lo .. row_hi of the global rows 0 .. nx + 1 and owns own_lo .. own_hi of them.  It computes
// the interior rows it has a neighbour row for on both sides; an edge of the strip that is not a wall of the domain
// is an interior edge, and the W = VOF_HALO_ROWS owned rows next to it are what the neighbour's halo receives: a band.
struct StripRows {
  RowRange owned;              // the owned rows inside the computable rows
  RowRange band_lo, band_hi;   // the W-row bands (none at a wall; none where the bands meet)
  RowRange rest;               // the owned rows between the bands (none where the bands meet)
  bool has_bands;              // the strip has an interior edge
  bool meet;                   // the bands leave no row between them: the strip is not split, all of it counts as bands
};
inline StripRows strip_rows(int row_lo, int row_hi, int own_lo, int own_hi, int nx, int jacobi_iters) {
  const int W = VOF_HALO_ROWS(jacobi_iters);
  const int ilo = row_lo + 1 > 1 ? row_lo + 1 : 1, ihi = row_hi - 1 < nx ? row_hi - 1 : nx;
  const bool edge_lo = row_lo != 0, edge_hi = row_hi != nx + 1;
  StripRows s{{own_lo > ilo ? own_lo : ilo, own_hi < ihi ? own_hi : ihi}, kNoRows, kNoRows, kNoRows, edge_lo || edge_hi, false};
  const int in_lo = edge_lo ? s.owned.first + W : s.owned.first, in_hi = edge_hi ? s.owned.last - W : s.owned.last;
  s.meet = s.has_bands && in_lo > in_hi;
  if (s.meet) return s;
  if (edge_lo) s.band_lo = {s.owned.first, in_lo - 1};
  if (edge_hi) s.band_hi = {in_hi + 1, s.owned.last};
  s.rest = {in_lo, in_hi};
  return s;
}

// The cells a handle reports (vof_diagnostics, vof_interface, vof_blobs): its owned rows inside what it can compute (row
// own_hi + 1 of u is read: a strip stores it as a halo row, a full domain as the wall's ghost row), ny columns in ntj tiles
struct ReportedRows {
  RowRange range;
  int ny, ntj;
  int rows() const { return range.rows(); }
  int64_t cells() const { return (int64_t)rows() * ny; }
  int64_t entries() const { return (int64_t)rows() * ntj; }   // one per (row, column tile)
  unsigned blocks(int R) const { return (unsigned)(((long)((rows() + R - 1) / R) * ntj + 3) / 4); }   // chunks of R rows, four waves a block
};
inline ReportedRows reported_rows(int row_lo, int row_hi, int own_lo, int own_hi, int nx, int ny, int ntj) {
  return {strip_rows(row_lo, row_hi, own_lo, own_hi, nx, 0).owned, ny, ntj};   // (the owned rows do not depend on the halo width)
}

// The cells-per-wave rule of the chunk lengths (chunk_rows of runtime/launches.h, plain: ~4096 waves, a power of two between rmin
// and rmax) on `rows` rows of `ntiles` tiles
inline int cells_per_wave_rows(long rows, int ntiles, int rmin, int rmax) {
  long R = rows * ntiles / 4096;
  if (R < rmin) R = rmin;
  if (R > rmax) R = rmax;
  long P = 1;
  while (P * 2 <= R) P *= 2;
  return (int)(P < rmin ? rmin : P);
}

// vof_depths (kernels/depths.h): the chunk length -- the rule above with 2 and 32 on the rows the handle can compute,
// max(1, row_lo + 1) .. min(nx, row_hi - 1), whatever it owns of them -- and what a launch on the reported rows leaves
// behind: one partial per (row, tile) and per (chunk, column)
inline int depths_chunk_rows(int row_lo, int row_hi, int nx, int ntj) {
  const int ilo = row_lo + 1 > 1 ? row_lo + 1 : 1, ihi = row_hi - 1 < nx ? row_hi - 1 : nx;
  return cells_per_wave_rows(ihi - ilo + 1, ntj, 2, 32);
}
struct DepthsGeom {
  int R, chunks;
  int64_t row_partials, col_partials;
  unsigned blocks;                   // of k_depths: four waves a block (0: nothing to launch)
  unsigned row_blocks, col_blocks;   // of k_depths_fold: 256 rows, 256 columns a block
};
inline DepthsGeom depths_geom(const ReportedRows& rep, int R) {
  const int chunks = (rep.rows() + R - 1) / R;
  return {R, chunks, rep.entries(), (int64_t)chunks * rep.ny, rep.blocks(R), (unsigned)((rep.rows() + 255) / 256), (unsigned)((rep.ny + 255) / 256)};
}

// vof_frame (kernels/frames.h) on a whole domain: pixel (a, b) covers bx x by cells, the last pixel row / column what is left.
// Blocks larger than the grid count as the grid (one pixel that way either way; no product of theirs overflows).  A wave of
// k_frame_cols marches K whole pixel rows: the cells-per-wave rule with 2 and 32 gives a length, K = max(1, length / bx) pixel
// rows of it make a chunk of R = K bx rows (the last chunk ends at nx).  It leaves one partial per (pixel row, column), the
// columns padded to whole tiles of `tile` = 64 V columns so that every lane stores its V partials as one vector: cpitch doubles
// a pixel row.  k_frame_fold and k_frame_paint: one lane per pixel, 256 a block, at most kFramePixelBlocks blocks striding over the pixels.
constexpr unsigned kFramePixelBlocks = 256;
struct FrameGeom {
  int bx, by;       // as used: min(bx, nx), min(by, ny)
  int pw, ph;       // ceil(nx / bx), ceil(ny / by)
  int K, R, chunks;
  int cpitch;
  int64_t col_partials;   // pw * cpitch
  int64_t pixels;         // pw * ph
  unsigned cols_blocks;   // of k_frame_cols: four waves a block
  unsigned pixel_blocks;  // of k_frame_fold and k_frame_paint
};
inline FrameGeom frame_geom(int nx, int ny, int ntj, int tile, int bx, int by) {
  FrameGeom f;
  f.bx = bx < nx ? bx : nx; f.by = by < ny ? by : ny;
  f.pw = (nx + f.bx - 1) / f.bx; f.ph = (ny + f.by - 1) / f.by;
  const int len = cells_per_wave_rows(nx, ntj, 2, 32);
  f.K = len / f.bx > 1 ? len / f.bx : 1;
  f.R = f.K * f.bx;
  f.chunks = (f.pw + f.K - 1) / f.K;
  f.cpitch = ntj * tile;
  f.col_partials = (int64_t)f.pw * f.cpitch;
  f.pixels = (int64_t)f.pw * f.ph;
  f.cols_blocks = (unsigned)(((long)f.chunks * ntj + 3) / 4);
  f.pixel_blocks = (f.pixels + 255) / 256 < (int64_t)kFramePixelBlocks ? (unsigned)((f.pixels + 255) / 256) : kFramePixelBlocks;
  return f;
}

// The kernels that end a step on a strip run on all owned rows at once, or on the bands first (the exchange waits for
// them alone) and on the rest beside the exchange.
enum StripPart { kAllOwned = 0, kEdgeBands = 1, kRest = 2 };
// What the launch of one part gets: the two bands (short chunks, both in one launch) and / or one body range (chunks
// of the usual length).  A full domain has no bands: everything is "rest".  Where the bands meet there is no rest:
// everything is "bands", as one body range.  A part with nothing in it gets no launch.
struct PartRows {
  RowRange band_lo, band_hi, body;
  bool empty() const { return band_lo.empty() && band_hi.empty() && body.empty(); }
};
inline PartRows part_rows(const StripRows& s, int part) {
  const bool split = s.has_bands && !s.meet;
  if (part == kAllOwned || !split) {
    const bool mine = part == kAllOwned || (part == kEdgeBands) == s.has_bands;
    return {kNoRows, kNoRows, mine ? s.owned : kNoRows};
  }
  if (part == kEdgeBands) return {s.band_lo, s.band_hi, kNoRows};
  return {kNoRows, kNoRows, s.rest};
}

}  // namespace vof
