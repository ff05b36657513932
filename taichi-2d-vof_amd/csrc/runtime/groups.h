// runtime/groups.h -- the loop of every vof_step_<verb>: steps in groups, something behind every group, the remainder
//
// Plain C++ (no HIP): runtime/step.h includes it, the CPU tests compile it on its own.
#pragma once
#include <stdint.h>

namespace vof {

// nsteps steps in groups of `every` (>= 1): steps(every), after(r) for r = 0 .. nsteps / every - 1, then steps(nsteps % every) if that
// is not 0.  The first non-zero return of either ends the loop and is returned; nothing is called after it.
template <class Steps, class After>
int step_groups(int64_t nsteps, int64_t every, Steps&& steps, After&& after) {
  for (int64_t r = 0; r < nsteps / every; ++r) {
    if (const int rc = steps(every)) return rc;
    if (const int rc = after(r)) return rc;
  }
  return nsteps % every ? steps(nsteps % every) : 0;
}

}  // namespace vof
