// Stand-alone check (host compiler, no HIP) of kernels/row_segments.h: the chunk index -> (segment, chunk, rows) mapping the
// entries of k_tm and k_transport read, and the chunk count their launches compute from the same header.
// Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/row_segments.h"
#include "vof2d_device.h"

using namespace vof;

static int failures = 0;
static long checks = 0;
#define CHECK(cond, ...)                                            \
  do {                                                              \
    ++checks;                                                       \
    if (!(cond)) {                                                  \
      if (failures++ < 20) { std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } \
    }                                                               \
  } while (0)

// What k_tm's entry computed before the segments, written out: rows [first, last] and [first2, last2] in chunks of R.
static RowChunk chunk_before(int ch, int R, int first, int last, int first2, int last2) {
  int ma = first + ch * R, lim = last;
  if (ma > last) {
    const int n1 = last >= first ? (last - first + R) / R : 0;
    ma = first2 + (ch - n1) * R;
    lim = last2;
    if (last2 < first2 || ma > last2) return RowChunk{1, 0};
  }
  return RowChunk{ma, ma + R - 1 < lim ? ma + R - 1 : lim};
}
static int chunks_before(int R, int first, int last, int first2, int last2) {
  return ((last - first + R) / R) + (last2 >= first2 ? (last2 - first2 + R) / R : 0);
}

// Every row of `want` (0 / 1 per row, rows 0 .. size - 1) lies in exactly one chunk of the launch, every chunk inside its
// segment and no longer than the segment's length, the chunks of the launch in ascending order within a segment, nothing
// behind the last chunk; and for every tile column alike (a pair is chunk * ntf + tile: the launch's pair count).
static void check_layout(const RowSegments& sg, const std::vector<int>& want, int ntf, const char* what) {
  const int n = row_chunks(sg);
  int sum = 0, used = 0;
  for (int k = 0; k < kRowMaxSegments; ++k) {
    const RowSeg& s = sg.s[k];
    CHECK(s.R >= 1, "%s: segment %d R %d", what, k, s.R);
    CHECK(s.nch == row_seg_chunks(s.first, s.last, s.R), "%s: segment %d", what, k);
    CHECK((s.nch == 0) == (s.last < s.first), "%s: segment %d: %d chunks of rows %d..%d", what, k, s.nch, s.first, s.last);
    sum += s.nch;
    used += s.nch > 0;
  }
  CHECK(sum == n && used == row_used_segments(sg), "%s: %d chunks, %d segments", what, n, used);
  std::vector<int> got(want.size(), 0);
  int seg = 0, left = sg.s[0].nch, prev_mb = -1;
  for (int ch = 0; ch < n; ++ch) {
    while (left == 0 && seg + 1 < kRowMaxSegments) { left = sg.s[++seg].nch; prev_mb = -1; }
    --left;
    const RowChunk c = row_chunk(sg, ch);
    CHECK(!c.none(), "%s: chunk %d of %d is empty", what, ch, n);
    if (c.none()) continue;
    const RowSeg& s = sg.s[seg];
    CHECK(c.ma >= s.first && c.mb <= s.last && c.mb - c.ma + 1 <= s.R, "%s: chunk %d rows %d..%d, segment %d rows %d..%d R %d", what, ch, c.ma, c.mb, seg, s.first, s.last, s.R);
    CHECK(c.mb - c.ma + 1 == s.R || c.mb == s.last, "%s: chunk %d is short inside its segment", what, ch);
    CHECK(prev_mb < 0 || c.ma == prev_mb + 1, "%s: chunk %d starts at %d behind %d", what, ch, c.ma, prev_mb);
    prev_mb = c.mb;
    for (int i = c.ma; i <= c.mb; ++i) {
      CHECK(i >= 0 && i < (int)got.size(), "%s: row %d", what, i);
      if (i >= 0 && i < (int)got.size()) got[i] += 1;
    }
  }
  for (size_t i = 0; i < want.size(); ++i) CHECK(got[i] == want[i], "%s: row %d in %d chunks, expected %d", what, (int)i, got[i], want[i]);
  CHECK(row_chunk(sg, n).none() && row_chunk(sg, n + 1).none() && row_chunk(sg, n + 1000).none() && row_chunk(sg, -1).none(), "%s: chunks behind the last", what);
  // pairs: ch = pair / ntf, tile = pair % ntf -- every (row, tile column) once over the launch's n * ntf pairs
  std::vector<int> cells(want.size() * (size_t)ntf, 0);
  const long pairs = (long)n * ntf;
  for (long pair = 0; pair < pairs; ++pair) {
    const RowChunk c = row_chunk(sg, (int)(pair / ntf));
    for (int i = c.ma; i <= c.mb; ++i)
      if (i >= 0 && i < (int)want.size()) cells[(size_t)i * ntf + (size_t)(pair % ntf)] += 1;
  }
  for (size_t i = 0; i < want.size(); ++i)
    for (int tj = 0; tj < ntf; ++tj) CHECK(cells[i * ntf + tj] == want[i], "%s: row %d tile %d", what, (int)i, tj);
}

// one to four segments that tile [first, last]: cut points from a small set that includes empty segments and segments of
// 1, 2 and 3 rows; chunk lengths from 1 up to longer than the segment
static void check_tilings() {
  const int lens[] = {1, 2, 3, 5, 12, 16, 52, 200};
  const int grids[][2] = {{1, 1}, {1, 2}, {1, 3}, {1, 17}, {1, 97}, {1, 160}, {19, 131}, {3073, 3301}};
  for (const auto& gr : grids) {
    const int first = gr[0], last = gr[1], rows = last - first + 1;
    std::vector<int> cuts;   // a cut c: the next segment starts at first + c
    for (int c : {0, 1, 2, 3, rows / 3, rows / 2, rows - 3, rows - 2, rows - 1, rows})
      if (c >= 0 && c <= rows) cuts.push_back(c);
    std::vector<int> want(last + 2, 0);
    for (int i = first; i <= last; ++i) want[i] = 1;
    for (int ntf : {1, 3}) {
      for (int c1 : cuts)
        for (int c2 : cuts)
          for (int c3 : cuts) {
            if (c1 > c2 || c2 > c3) continue;
            if (ntf == 3 && (c1 + c2 + c3) % 3 != 0) continue;   // (a third of them with more than one tile column)
            for (int l0 : lens)
              for (int l1 : {1, 3, 7, 26})
                for (int l2 : {1, 2, 13}) {
                  const int l3 = l0 > 3 ? l0 / 4 : 1;
                  const RowSegments sg = row_segments(row_seg(first, first + c1 - 1, l0), row_seg(first + c1, first + c2 - 1, l1),
                                                    row_seg(first + c2, first + c3 - 1, l2), row_seg(first + c3, last, l3));
                  check_layout(sg, want, ntf, "tiling");
                }
          }
    }
  }
  // fewer than four segments given: the others hold nothing
  for (int R : lens) {
    std::vector<int> want(252, 0);
    for (int i = 1; i <= 250; ++i) want[i] = 1;
    const RowSegments one = row_segments(row_seg(1, 250, R));
    check_layout(one, want, 2, "one segment");
    CHECK(row_used_segments(one) == 1 && row_chunks(one) == (250 + R - 1) / R, "one segment of %d-row chunks", R);
    check_layout(row_segments(row_seg(1, 100, R), row_seg(101, 250, 7)), want, 2, "two segments");
    check_layout(row_segments(row_seg(1, 100, R), row_seg(101, 249, 7), row_seg(250, 250, 3)), want, 2, "a last segment of one row");
  }
  CHECK(row_chunks(row_segments(row_seg(5, 4, 3))) == 0 && row_chunk(row_segments(row_seg(5, 4, 3)), 0).none(), "no rows at all");
  CHECK(row_seg(1, 10, 0).R == 1 && row_seg(1, 10, -4).nch == 10, "a chunk length below one row counts as one");
}

// the two bands of a strip in one launch: two segments of one chunk length against the expressions they replaced
static void check_two_bands() {
  for (int R : {1, 2, 5, 6, 7, 18, 19, 40})
    for (int rows1 = 0; rows1 <= 20; ++rows1)
      for (int rows2 = 0; rows2 <= 20; ++rows2)
        for (int gap : {0, 1, 500}) {
          const int first = 117, last = first + rows1 - 1, first2 = rows2 ? last + 1 + gap : 1, last2 = rows2 ? first2 + rows2 - 1 : 0;
          if (rows1 == 0) continue;   // (the launch wrapper puts a lone band first: the first range always holds rows)
          const RowSegments sg = row_segments(row_seg(first, last, R), row_seg(first2, last2, R));
          const int n = chunks_before(R, first, last, first2, last2);
          CHECK(row_chunks(sg) == n, "bands %d + %d rows, R %d: %d chunks, %d before", rows1, rows2, R, row_chunks(sg), n);
          for (int ch = 0; ch <= n + 2; ++ch) {
            const RowChunk a = row_chunk(sg, ch), b = chunk_before(ch, R, first, last, first2, last2);
            CHECK((a.none() && b.none()) || (a.ma == b.ma && a.mb == b.mb), "bands %d + %d rows, R %d, chunk %d: %d..%d, before %d..%d", rows1, rows2, R, ch, a.ma, a.mb, b.ma, b.mb);
          }
          std::vector<int> want(last2 > last ? last2 + 2 : last + 2, 0);
          for (int i = first; i <= last; ++i) want[i] += 1;
          for (int i = first2; i <= last2; ++i) want[i] += 1;
          check_layout(sg, want, TmGeom<2>::tiles(250), "two bands");
        }
  // one range, as every other launch passed it: [first, last] with the second range absent (1, 0)
  for (int R : {1, 16, 37, 52, 64})
    for (int last : {1, 2, 15, 16, 17, 160, 4096}) {
      const RowSegments sg = row_segments(row_seg(1, last, R));
      const int n = chunks_before(R, 1, last, 1, 0);
      CHECK(row_chunks(sg) == n, "rows 1..%d R %d", last, R);
      for (int ch = 0; ch <= n + 1; ++ch) {
        const RowChunk a = row_chunk(sg, ch), b = chunk_before(ch, R, 1, last, 1, 0);
        CHECK((a.none() && b.none()) || (a.ma == b.ma && a.mb == b.mb), "rows 1..%d R %d chunk %d", last, R, ch);
      }
    }
}

// What k_transport's entry computed before it took segments, written out: up to three ranges [first[k], last[k]] (last < first: none)
// in chunks of R[k], the chunks counted through the ranges in order (cumulative chunk counts).
static RowChunk three_ranges_before(int ch, const int (&first)[3], const int (&last)[3], const int (&R)[3]) {
  int k = 0, cbase = 0;
  for (; k < 3; ++k) {
    const int n = last[k] >= first[k] ? (last[k] - first[k] + R[k]) / R[k] : 0;
    if (ch < cbase + n) break;
    cbase += n;
  }
  if (k == 3) return RowChunk{1, 0};
  const int ra = first[k] + (ch - cbase) * R[k];
  return RowChunk{ra, ra + R[k] - 1 < last[k] ? ra + R[k] - 1 : last[k]};
}
static void check_three(const char* what, int lo_first, int lo_last, int hi_first, int hi_last, int body_first, int body_last, int Rb, int R) {
  // the order of the launch: the lower band, the upper band, the body (the neighbours wait for the bands)
  const int first[3] = {lo_first, hi_first, body_first}, last[3] = {lo_last, hi_last, body_last}, len[3] = {Rb, Rb, R};
  const RowSegments sg = row_segments(row_seg(lo_first, lo_last, Rb), row_seg(hi_first, hi_last, Rb), row_seg(body_first, body_last, R));
  int n = 0;
  for (int k = 0; k < 3; ++k) n += last[k] >= first[k] ? (last[k] - first[k] + len[k]) / len[k] : 0;
  CHECK(row_chunks(sg) == n, "%s: %d chunks, %d before", what, row_chunks(sg), n);
  for (int ch = 0; ch <= n; ++ch) {   // every chunk index from 0 to one past the last
    const RowChunk a = row_chunk(sg, ch), b = three_ranges_before(ch, first, last, len);
    CHECK((a.none() && b.none()) || (a.ma == b.ma && a.mb == b.mb), "%s, chunk %d: %d..%d, before %d..%d", what, ch, a.ma, a.mb, b.ma, b.mb);
    CHECK(a.none() == (ch == n), "%s, chunk %d of %d", what, ch, n);
  }
}
// the ranges k_transport took as RowRanges: a strip's two edge bands in short chunks and its body, in one launch
static void check_three_ranges() {
  check_three("both bands and a body, three chunk lengths apart", 101, 110, 191, 200, 111, 190, 4, 16);
  {  // (the bands and the body with different lengths each: the segments carry their own)
    const int first[3] = {101, 191, 111}, last[3] = {110, 200, 190}, len[3] = {4, 3, 16};
    const RowSegments sg = row_segments(row_seg(101, 110, 4), row_seg(191, 200, 3), row_seg(111, 190, 16));
    const int n = 3 + 4 + 5;
    CHECK(row_chunks(sg) == n, "three lengths: %d chunks", row_chunks(sg));
    for (int ch = 0; ch <= n; ++ch) {
      const RowChunk a = row_chunk(sg, ch), b = three_ranges_before(ch, first, last, len);
      CHECK((a.none() && b.none()) || (a.ma == b.ma && a.mb == b.mb), "three lengths, chunk %d: %d..%d, before %d..%d", ch, a.ma, a.mb, b.ma, b.mb);
    }
  }
  check_three("the first strip: no lower band", 1, 0, 91, 100, 1, 90, 4, 16);
  check_three("the last strip: no upper band", 101, 110, 1, 0, 111, 200, 4, 16);
  check_three("no band at all", 1, 0, 1, 0, 1, 200, 4, 16);
  check_three("bands of 10 rows in 4-row chunks: a ragged last chunk", 13, 22, 25, 34, 23, 24, 4, 16);
  check_three("a body of one row", 13, 22, 24, 33, 23, 23, 4, 16);
  check_three("the bands alone", 13, 22, 25, 34, 1, 0, 4, 16);
  for (int Rb : {1, 3, 4, 10, 11})
    for (int R : {1, 2, 16})
      for (int body : {0, 1, 2, 17, 32}) {
        check_three("bands and body, every length", 13, 22, 23 + body, 32 + body, 23, 22 + body, Rb, R);
        check_three("upper band and body, every length", 1, 0, 23 + body, 32 + body, 23, 22 + body, Rb, R);
      }
}

int main() {
  check_tilings();
  check_two_bands();
  check_three_ranges();
  if (failures) { std::printf("%d of %ld checks failed\n", failures, checks); return 1; }
  std::printf("%ld checks\nok\n", checks);
  return 0;
}
