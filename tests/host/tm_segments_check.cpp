// Stand-alone check (host compiler, no HIP) of kernels/tm_segments.h: the pair index -> (segment, chunk, rows) mapping k_tm's
// entry reads, and the pair count its launch computes from the same header.
// Exit status 0 and "ok" on success; the first failing checks are printed otherwise.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/tm_segments.h"
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
static TmChunk chunk_before(int ch, int R, int first, int last, int first2, int last2) {
  int ma = first + ch * R, lim = last;
  if (ma > last) {
    const int n1 = last >= first ? (last - first + R) / R : 0;
    ma = first2 + (ch - n1) * R;
    lim = last2;
    if (last2 < first2 || ma > last2) return TmChunk{1, 0};
  }
  return TmChunk{ma, ma + R - 1 < lim ? ma + R - 1 : lim};
}
static int chunks_before(int R, int first, int last, int first2, int last2) {
  return ((last - first + R) / R) + (last2 >= first2 ? (last2 - first2 + R) / R : 0);
}

// Every row of `want` (0 / 1 per row, rows 0 .. size - 1) lies in exactly one chunk of the launch, every chunk inside its
// segment and no longer than the segment's length, the chunks of the launch in ascending order within a segment, nothing
// behind the last chunk; and for every tile column alike (a pair is chunk * ntf + tile: the launch's pair count).
static void check_layout(const TmSegments& sg, const std::vector<int>& want, int ntf, const char* what) {
  const int n = tm_chunks(sg);
  int sum = 0, used = 0;
  for (int k = 0; k < kTmMaxSegments; ++k) {
    const TmSeg& s = sg.s[k];
    CHECK(s.R >= 1, "%s: segment %d R %d", what, k, s.R);
    CHECK(s.nch == tm_seg_chunks(s.first, s.last, s.R), "%s: segment %d", what, k);
    CHECK((s.nch == 0) == (s.last < s.first), "%s: segment %d: %d chunks of rows %d..%d", what, k, s.nch, s.first, s.last);
    sum += s.nch;
    used += s.nch > 0;
  }
  CHECK(sum == n && used == tm_used_segments(sg), "%s: %d chunks, %d segments", what, n, used);
  std::vector<int> got(want.size(), 0);
  int seg = 0, left = sg.s[0].nch, prev_mb = -1;
  for (int ch = 0; ch < n; ++ch) {
    while (left == 0 && seg + 1 < kTmMaxSegments) { left = sg.s[++seg].nch; prev_mb = -1; }
    --left;
    const TmChunk c = tm_chunk(sg, ch);
    CHECK(!c.none(), "%s: chunk %d of %d is empty", what, ch, n);
    if (c.none()) continue;
    const TmSeg& s = sg.s[seg];
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
  CHECK(tm_chunk(sg, n).none() && tm_chunk(sg, n + 1).none() && tm_chunk(sg, n + 1000).none() && tm_chunk(sg, -1).none(), "%s: chunks behind the last", what);
  // pairs: ch = pair / ntf, tile = pair % ntf -- every (row, tile column) once over the launch's n * ntf pairs
  std::vector<int> cells(want.size() * (size_t)ntf, 0);
  const long pairs = (long)n * ntf;
  for (long pair = 0; pair < pairs; ++pair) {
    const TmChunk c = tm_chunk(sg, (int)(pair / ntf));
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
                  const TmSegments sg = tm_segments(tm_seg(first, first + c1 - 1, l0), tm_seg(first + c1, first + c2 - 1, l1),
                                                    tm_seg(first + c2, first + c3 - 1, l2), tm_seg(first + c3, last, l3));
                  check_layout(sg, want, ntf, "tiling");
                }
          }
    }
  }
  // fewer than four segments given: the others hold nothing
  for (int R : lens) {
    std::vector<int> want(252, 0);
    for (int i = 1; i <= 250; ++i) want[i] = 1;
    const TmSegments one = tm_segments(tm_seg(1, 250, R));
    check_layout(one, want, 2, "one segment");
    CHECK(tm_used_segments(one) == 1 && tm_chunks(one) == (250 + R - 1) / R, "one segment of %d-row chunks", R);
    check_layout(tm_segments(tm_seg(1, 100, R), tm_seg(101, 250, 7)), want, 2, "two segments");
    check_layout(tm_segments(tm_seg(1, 100, R), tm_seg(101, 249, 7), tm_seg(250, 250, 3)), want, 2, "a last segment of one row");
  }
  CHECK(tm_chunks(tm_segments(tm_seg(5, 4, 3))) == 0 && tm_chunk(tm_segments(tm_seg(5, 4, 3)), 0).none(), "no rows at all");
  CHECK(tm_seg(1, 10, 0).R == 1 && tm_seg(1, 10, -4).nch == 10, "a chunk length below one row counts as one");
}

// the two bands of a strip in one launch: two segments of one chunk length against the expressions they replaced
static void check_two_bands() {
  for (int R : {1, 2, 5, 6, 7, 18, 19, 40})
    for (int rows1 = 0; rows1 <= 20; ++rows1)
      for (int rows2 = 0; rows2 <= 20; ++rows2)
        for (int gap : {0, 1, 500}) {
          const int first = 117, last = first + rows1 - 1, first2 = rows2 ? last + 1 + gap : 1, last2 = rows2 ? first2 + rows2 - 1 : 0;
          if (rows1 == 0) continue;   // (the launch wrapper puts a lone band first: the first range always holds rows)
          const TmSegments sg = tm_segments(tm_seg(first, last, R), tm_seg(first2, last2, R));
          const int n = chunks_before(R, first, last, first2, last2);
          CHECK(tm_chunks(sg) == n, "bands %d + %d rows, R %d: %d chunks, %d before", rows1, rows2, R, tm_chunks(sg), n);
          for (int ch = 0; ch <= n + 2; ++ch) {
            const TmChunk a = tm_chunk(sg, ch), b = chunk_before(ch, R, first, last, first2, last2);
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
      const TmSegments sg = tm_segments(tm_seg(1, last, R));
      const int n = chunks_before(R, 1, last, 1, 0);
      CHECK(tm_chunks(sg) == n, "rows 1..%d R %d", last, R);
      for (int ch = 0; ch <= n + 1; ++ch) {
        const TmChunk a = tm_chunk(sg, ch), b = chunk_before(ch, R, 1, last, 1, 0);
        CHECK((a.none() && b.none()) || (a.ma == b.ma && a.mb == b.mb), "rows 1..%d R %d chunk %d", last, R, ch);
      }
    }
}

int main() {
  check_tilings();
  check_two_bands();
  if (failures) { std::printf("%d of %ld checks failed\n", failures, checks); return 1; }
  std::printf("%ld checks\nok\n", checks);
  return 0;
}
