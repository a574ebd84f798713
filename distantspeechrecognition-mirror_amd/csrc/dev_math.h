// csrc/dev_math.h -- the small device helpers that several kernel units share: complex fp64 arithmetic on double2, the clamp of a frame count,
// the 64-lane sum and the two wavefront LDS syncs.  Every expression is the one the units had; a unit whose helper differs in rounding keeps it
// (mk_wsum in k_mk.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace dsr {

__device__ __forceinline__ double2 z2() { return make_double2(0.0, 0.0); }
__device__ __forceinline__ double2 cj(double2 a) { return make_double2(a.x, -a.y); }
__device__ __forceinline__ double abs2(double2 a) { return a.x * a.x + a.y * a.y; }
__device__ __forceinline__ double2 cmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 cmul_conj(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ double2 conj_mul(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x); }    // conj(a) b
__device__ __forceinline__ double2 shfl2(double2 a, int src) { return make_double2(__shfl(a.x, src), __shfl(a.y, src)); }

// gsl_complex_div (GSL complex/math.c): scale by 1/|b| first -- restated so that the last bit does not depend on a runtime's __divdc3
__host__ __device__ __forceinline__ double2 gsl_div(double2 a, double2 b)
{ const double s = 1.0 / hypot(b.x, b.y); const double sbr = s * b.x, sbi = s * b.y; return make_double2((a.x * sbr + a.y * sbi) * s, (a.y * sbr - a.x * sbi) * s); }

// frames of utterance u: nf[u] clamped to [0, Tmax]; Tmax when there is no count array
__device__ __forceinline__ int clampT(const int* nf, int u, int Tmax) { int T = nf ? nf[u] : Tmax; return T < 0 ? 0 : (T > Tmax ? Tmax : T); }

// sum over the 64 lanes, butterfly from distance 32 down: every lane ends with the same bits
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// What one wave wrote to LDS becomes readable by its other lanes: LDS runs a wave's accesses in order, the compiler has to keep them so.  Two
// forms, as the kernels were tuned with them: one acquire-release fence before the barrier, or a release fence, the barrier, an acquire fence.
__device__ __forceinline__ void wave_lds_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
__device__ __forceinline__ void wave_sync()
{ __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }

}  // namespace dsr
