// csrc/gmm_dist.h -- the Mahalanobis sum of scoring mode 0 (CodebookBasic::_scoreOpt, asr/gaussian/codebookBasic.cc:431-554), one definition
// for k_gmm.hip (k_gmm_exact) and k_fsa.hip (k_fsa_nearest): fp32, d ascending, (mu - x)^2 * iv, no FMA, starting from pi + det.
#pragma once
#include <hip/hip_runtime.h>

namespace dsr {

__device__ __forceinline__ float gmm_dist_exact(float dist, const float* rv, const float* cv, const float* xr, int n)
{
#pragma unroll
  for (int d = 0; d < n; d++) { const float diff = __fsub_rn(rv[d], xr[d]); dist = __fadd_rn(dist, __fmul_rn(__fmul_rn(diff, diff), cv[d])); }
  return dist;
}

}  // namespace dsr
