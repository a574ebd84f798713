// csrc/mfma64.h -- the fp64 MFMA helpers of the kernels that run complex GEMMs on v_mfma_f64_16x16x4_f64 (k_doa.hip, k_sph.hip,
// k_wpe_tiled.hip).
//
// v_mfma_f64_16x16x4_f64 lane map: lane l holds A[l & 15][k = l >> 4] and B[k = l >> 4][l & 15]; result register q of lane l is
// C[(l >> 4) + 4 q][l & 15] (not the fp32 map; tools/probes/probe_f64_mfma.hip checks it with asymmetric integer data).
#pragma once
#include <hip/hip_runtime.h>

namespace dsr {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ d4 mfma64(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
// (cr + i ci) += (ar + i ai) (br + i bi) over one k-step of 4
__device__ __forceinline__ void cmfma(double ar, double ai, double br, double bi, d4& cr, d4& ci)
{
  cr = mfma64(ar, br, cr); cr = mfma64(-ai, bi, cr); ci = mfma64(ar, bi, ci); ci = mfma64(ai, br, ci);
}

}  // namespace dsr
