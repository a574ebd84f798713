// csrc/fft_lds.h -- the fp64 radix-2 FFT that k_gcc.hip (k_gcc_corr, k_cctde) and k_conv.hip share (DESIGN 4.4j gives the bank layout and
// the LDS budget).  The transform works on any pair of fp64 arrays a workgroup owns: LDS, or a block of global memory for transforms that
// do not fit (the waves of a workgroup share a CU and its L1, and __syncthreads() orders their accesses).
//
// n points, data in re[] / im[], loaded in bit-reversed order by the caller.  Twiddles exp(+2 pi i j / n): tw[0 .. n/2) serves the stages with
// half-span h >= n/4; the stage with half-span h < n/4 reads tw[n/2 + h - 1 + k], k < h.  sgn = -1 conjugates them (forward transform).
#pragma once
#include <hip/hip_runtime.h>

namespace dsr {

__host__ __device__ inline int fft_tw_entries(int n) { return n / 2 + n / 4; }
inline int fft_block(int butterflies) { return butterflies < 64 ? 64 : (butterflies > 256 ? 256 : butterflies); }

#ifdef __HIPCC__
__device__ inline void fft_tw_init(double* twr, double* twi, int n)
{
  for (int j = threadIdx.x; j < n / 2; j += blockDim.x) { double sn, cs; sincospi(2.0 * j / n, &sn, &cs); twr[j] = cs; twi[j] = sn; }
  for (int h = 1; 4 * h < n; h *= 2)
    for (int k = threadIdx.x; k < h; k += blockDim.x) { double sn, cs; sincospi((double) k / h, &sn, &cs); twr[n / 2 + h - 1 + k] = cs; twi[n / 2 + h - 1 + k] = sn; }
}
__device__ inline void fft_run(double* re, double* im, const double* twr, const double* twi, int n, double sgn)
{
  for (int h = 1; h < n; h *= 2) {
    __syncthreads();
    for (int j = threadIdx.x; j < n / 2; j += blockDim.x) {
      const int k = j & (h - 1), i0 = ((j - k) << 1) + k, i1 = i0 + h;
      const int w = 4 * h >= n ? k * (n / (2 * h)) : n / 2 + h - 1 + k;
      const double wr = twr[w], wi = sgn * twi[w];
      const double xr = re[i1], xi = im[i1], tr = xr * wr - xi * wi, ti = xr * wi + xi * wr;
      const double ar = re[i0], ai = im[i0];
      re[i0] = ar + tr; im[i0] = ai + ti; re[i1] = ar - tr; im[i1] = ai - ti;
    }
  }
  __syncthreads();
}
__device__ __forceinline__ int brev(int k, int logn) { return (int) (__brev((unsigned) k) >> (32 - logn)); }

// The split step of an inverse real transform of 2n points done as a complex one of n: from the half spectrum's bins A = X[k] and
// Bn = X[n-k], the input Z[k] = (X[k] + conj X[n-k]) + i (X[k] - conj X[n-k]) e^{2 pi i k / 2n} of the complex transform, whose output
// holds the even samples in its real and the odd ones in its imaginary parts (unscaled: the caller divides by 2n).
__device__ __forceinline__ double2 fft_split_inverse(double2 A, double2 Bn, int k, int n)
{
  double2 Bc = Bn; Bc.y = -Bc.y;
  const double ex = A.x + Bc.x, ey = A.y + Bc.y, dx = A.x - Bc.x, dy = A.y - Bc.y;
  double sn, cs; sincospi((double) k / n, &sn, &cs);
  const double ox = dx * cs - dy * sn, oy = dx * sn + dy * cs;
  return make_double2(ex - oy, ey + ox);
}
#endif

}  // namespace dsr
