// csrc/srp_common.h -- what the steered-response-power kernels share: k_doa.hip (linear array) and k_sph.hip (spherical array).
// The fp64 MFMA helpers, the staged-chunk frame energy of calcEnergy (beamformer.cc:3043-3074), the linear estimator's handle and its
// launchers, which the spherical estimator's folded path drives with a table of its own.  Files that include this are built with
// -ffp-contract=off: the energy must stay the reference's float accumulation bit for bit.
#pragma once
#include "common.h"
#include <complex>

struct dsr_doa {
  int nBest = 1, M = 0, C = 0; unsigned sampleRate = 16000;
  std::vector<double> pos;                                   // setArrayGeometry: the x coordinates
  double minTheta = -M_PI / 2, maxTheta = M_PI / 2, widthTheta = 0.1;   // the constructor's setSearchParam() (beamformer.h:531)
  int fbinMin = 1, fbinMax = 0; float threshold = 0.0f;
  // the steering table as built by the first use after construction / setSearchParam (the reference keeps it until then)
  bool tbl = false; unsigned tableGen = 0; int nTheta = 0, tblFbinMax = 0;
  std::vector<double> thetas; std::vector<std::complex<double>> W;   // W [tblFbinMax+1][nTheta][C]
  dsr::DevBuf<double2> dW; bool dDirty = true; int NT = 0, KS = 0;
  dsr::PerStream<dsr::DevBuf<double>> ws;                    // rp when the caller does not ask for it
};

namespace dsr {

typedef double d4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ d4 mfma64(double a, double b, d4 c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
__device__ __forceinline__ void cmfma(double ar, double ai, double br, double bi, d4& cr, d4& ci)
{
  cr = mfma64(ar, br, cr); cr = mfma64(-ai, bi, cr); ci = mfma64(ar, bi, ci); ci = mfma64(ai, br, ci);
}

// calcEnergy (:3043-3074) over nb staged bins f0.. of frame t: rp += g_f |zdotc(X_f, X_f)|^2 in a float.  xs [C][FB][BP] as k_doa_srp stages it.
__device__ __forceinline__ float srp_energy_chunk(const float2* xs, int C, int FB, int BP, int t, int f0, int nb, int M2, float e)
{
  for (int b = 0; b < nb; b++) {
    double s = 0.0;
    for (int c = 0; c < C; c++) { const float2 v = xs[(c * FB + t) * BP + b]; const double a = v.x, q = v.y; s = s + (a * a + q * q); }
    const double g = f0 + b < M2 ? 2.0 : 1.0;
    e = (float) ((double) e + g * (s * s));                 // the imaginary part of x^H x is exactly 0
  }
  return e;
}
// the energy's final division (:3071-3073)
__device__ __forceinline__ float srp_energy_final(float e, int M2, int C) { return e / (float) (2u * (unsigned) M2 * (unsigned) C); }

// k_doa_srp over s's table (uploaded when dirty): rp [U][Tmax][nTheta], energy [U][Tmax], Y (optional) the last unit's bins
void doa_launch_rp(dsr_doa& s, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st);
// k_doa_acc: acc[u][k] += rp of every frame t < nframes[u] with energy >= thr, in frame order
void doa_launch_acc(const double* rp, const float* en, const int* nf, int U, int Tmax, int nUnits, float thr, double* acc, hipStream_t st);

}  // namespace dsr
