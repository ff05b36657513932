// step_groups of runtime/groups.h, the loop of every vof_step_<verb>, on the host: the trace of its calls for every nsteps in
// 0..13 and every `every` in 1..5, and a failure injected at each position of that trace in turn.
#include <stdint.h>
#include <stdio.h>

#include <utility>
#include <vector>

#include "runtime/groups.h"

namespace {

enum Kind { kSteps, kAfter };
using Trace = std::vector<std::pair<Kind, int64_t>>;

// what the loop owes: [steps(every), after(r)] * (nsteps / every), then steps(nsteps % every) iff that is not 0
Trace expected(int64_t nsteps, int64_t every) {
  Trace t;
  for (int64_t r = 0; r < nsteps / every; ++r) {
    t.push_back({kSteps, every});
    t.push_back({kAfter, r});
  }
  if (nsteps % every) t.push_back({kSteps, nsteps % every});
  return t;
}

// the loop with call number fail_at (-1: none) returning `code`; the trace includes the failing call
int run(int64_t nsteps, int64_t every, long fail_at, int code, Trace& got) {
  auto note = [&](Kind k, int64_t v) {
    got.push_back({k, v});
    return (long)got.size() - 1 == fail_at ? code : 0;
  };
  return vof::step_groups(nsteps, every, [&](int64_t n) { return note(kSteps, n); }, [&](int64_t r) { return note(kAfter, r); });
}

}  // namespace

int main() {
  int bad = 0;
  for (int64_t nsteps = 0; nsteps <= 13; ++nsteps)
    for (int64_t every = 1; every <= 5; ++every) {
      const Trace want = expected(nsteps, every);
      Trace got;
      if (run(nsteps, every, -1, 0, got) != 0 || got != want) {
        printf("nsteps %lld every %lld: wrong trace or return\n", (long long)nsteps, (long long)every);
        ++bad;
      }
      for (long at = 0; at < (long)want.size(); ++at) {
        const int code = -(int)(at % 4) - 1;   // (the library's codes are negative)
        Trace cut;
        const int rc = run(nsteps, every, at, code, cut);
        if (rc != code || cut != Trace(want.begin(), want.begin() + at + 1)) {
          printf("nsteps %lld every %lld, failure at call %ld: returned %d, %zu calls\n", (long long)nsteps, (long long)every, at, rc, cut.size());
          ++bad;
        }
      }
    }
  if (bad) return 1;
  printf("ok\n");
  return 0;
}
