// kernels/residual_rule.h -- the residual of a criterion from the two norms of a check: ONE statement of the rule, for the
// host (vof_residual_value, include/vof2d.h) and for the device (k_mg_step_record, kernels/mg.h)
#pragma once
#include <hip/hip_runtime.h>

#include "../../../include/vof2d.h"

namespace vof {

__host__ __device__ inline double residual_rule(double max_update, double max_p, int criterion) {
  if (!(max_update < __builtin_huge_val())) return __builtin_huge_val();   /* inf or NaN: diverged */
  if (criterion == VOF_RESID_ABS) return max_update;
  /* a finite update over a tiny (or zero) max|p_new| must not read as "diverged": the quotient is
   * clamped to the largest finite double, so only a non-finite UPDATE ever returns +inf */
  const double q = max_update / (max_p > VOF_RESID_TINY ? max_p : VOF_RESID_TINY);
  return q < __builtin_huge_val() ? q : __DBL_MAX__;
}

}  // namespace vof
