// kernels/row_segments.h -- the rows of a k_tm or k_transport launch: up to four row ranges ("segments"), each cut in chunks of
// its own length, handed out in order; which chunk of which segment a pair (a wave) takes, and how many the launch needs
//
// Plain C++ (no HIP): the kernels' entries (kernels/fused_tm.h, kernels/transport.h) and the host's chunk count
// (runtime/launches.h) read the one mapping below, and tests/host/row_segments_check.cpp compiles it on its own.  The functions are constexpr, which
// is also what lets device code call them.
#pragma once

namespace vof {

constexpr int kRowMaxSegments = 4;

// rows [first, last] (last < first: none) in chunks of R rows, the last one ragged; nch = the number of those chunks
struct RowSeg { int first, last, R, nch; };
// By value in the kernel's arguments.  A full domain: the body and up to three tail segments of shorter chunks
// (L::tm_chunk_rows); a strip's two edge bands: two segments of one chunk length -- in k_transport the bands in short chunks
// and then the body: three; everything else: one segment.
struct RowSegments {
  RowSeg s[kRowMaxSegments];
};
struct RowChunk {
  int ma, mb;   // the chunk's rows; mb < ma: the chunk index lies behind the last segment
  constexpr bool none() const { return mb < ma; }
};

constexpr int row_seg_chunks(int first, int last, int R) { return last >= first ? (last - first + R) / R : 0; }
constexpr RowSeg row_seg(int first, int last, int R) { return RowSeg{first, last, R < 1 ? 1 : R, row_seg_chunks(first, last, R < 1 ? 1 : R)}; }
constexpr RowSeg kRowNoSeg{1, 0, 1, 0};
constexpr RowSegments row_segments(RowSeg a, RowSeg b = kRowNoSeg, RowSeg c = kRowNoSeg, RowSeg d = kRowNoSeg) { return RowSegments{{a, b, c, d}}; }

// chunks of all segments: the launch needs this many pairs (waves) per tile column
constexpr int row_chunks(const RowSegments& sg) {
  int n = 0;
  for (int k = 0; k < kRowMaxSegments; ++k) n += sg.s[k].nch;
  return n;
}
// segments that hold rows
constexpr int row_used_segments(const RowSegments& sg) {
  int n = 0;
  for (int k = 0; k < kRowMaxSegments; ++k) n += sg.s[k].nch > 0 ? 1 : 0;
  return n;
}
// Chunk `ch` of the launch, counted through the segments in order: its rows [ma, mb]; false: ch lies behind the last segment.
// A compare chain on launch-uniform values, shaped for k_tm's entry: the first segment -- nearly all pairs -- costs what the one
// range cost before, the others are looked up on the cold side of one branch, and the results leave through references (with the
// rows returned as a struct, or the chain in front of the branch, the register allocator keeps the kernel's arguments in VGPR
// lanes for the whole kernel instead of reloading them where they are used: 87 -> 1500 v_readlane in k_tm<double>).
constexpr bool row_chunk_rows_of(const RowSegments& sg, int ch, int& ma, int& mb) {
  int R = sg.s[0].R, lim = sg.s[0].last;
  ma = sg.s[0].first + ch * R;
  if (ch < 0 || ma > lim) {   // behind the first segment (an empty one has last < first)
    int k = ch - sg.s[0].nch;
    bool found = false;
    for (int q = 1; q < kRowMaxSegments; ++q) {
      if (!found && k >= 0 && k < sg.s[q].nch) { R = sg.s[q].R; ma = sg.s[q].first + k * R; lim = sg.s[q].last; found = true; }
      k -= sg.s[q].nch;
    }
    if (!found) return false;
  }
  mb = ma + R - 1 < lim ? ma + R - 1 : lim;
  return true;
}
constexpr RowChunk row_chunk(const RowSegments& sg, int ch) {
  int ma = 1, mb = 0;
  return row_chunk_rows_of(sg, ch, ma, mb) ? RowChunk{ma, mb} : RowChunk{1, 0};
}

}  // namespace vof
