// csrc/srp_common.h -- what the steered-response-power kernels share: k_doa.hip (linear array) and k_sph.hip (spherical array).
// The workgroup tiling and the parts of the two SRP kernels that are the same (snapshot staging, the staged-chunk frame energy of calcEnergy,
// beamformer.cc:3043-3074, the response-power accumulation and its epilogue), the N-best insertion of DOAEstimatorSRP*::next and
// _getNBestHypothesesFromACCRP (also the stream operators', csrc/streams_beamformer.cpp), the frequency-range check, the linear estimator's handle (host side: doa.cpp) and its
// launchers, which the spherical estimator's folded path (sph.cpp) drives with a table of its own.  Kernel files that include this are built with
// -ffp-contract=off: the energy must stay the reference's float accumulation bit for bit.
#pragma once
#include "common.h"
#include "mfma64.h"
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

constexpr int FB = 64;                                       // frames per workgroup (16 per wave)
#ifndef DOA_LDS_ROWS
#define DOA_LDS_ROWS 128
#endif
constexpr int LDS_ROWS = DOA_LDS_ROWS;                       // 128: at most 64 KB of staged snapshots (measured: 80 rows, 40 KB, is no faster at 8 channels and a third slower at 64)

// LDS row of one (channel, frame): BC bins, padded by one from 4 bins up so that the 16 frames a read touches fall in distinct banks
__host__ __device__ inline int bin_pitch(int BC) { return BC >= 4 ? BC + 1 : BC; }
inline int bin_chunk(int C)
{
  for (int BC = 16; BC > 1; BC >>= 1) if (C * bin_pitch(BC) <= LDS_ROWS) return BC;   // C * pitch * FB * 8 bytes <= LDS_ROWS / 2 KB
  return 1;
}
// The launch shape of an SRP call, in one place: the uploads, the launches and the queries (dsr_doa_srp_cell, dsr_sph_srp_cell) all take it from here.
inline int srp_tiles(int nUnits) { return (nUnits + 15) / 16; }          // NT: 16-unit row tiles, the last one zero padded
inline int srp_ksteps(int C) { return (C + 3) / 4; }                     // KS: K steps of 4 channels, the last one masked
inline size_t srp_lds_bytes(int C, int BC) { return (size_t) C * FB * bin_pitch(BC) * sizeof(float2); }   // the staged snapshots [C][FB][pitch]
struct SrpCell { int TG, BC, KS; size_t ldsBytes; };                     // k_doa_srp<TG> (k_sph_srp<TG, DT>) staging BC bins a chunk
inline int doa_tile_group(int NT) { return NT >= 4 ? 4 : NT >= 2 ? 2 : 1; }   // k_doa_srp's unit tiles per workgroup
inline SrpCell doa_srp_cell(int nUnits, int C)
{
  const int BC = bin_chunk(C);
  return SrpCell{doa_tile_group(srp_tiles(nUnits)), BC, srp_ksteps(C), srp_lds_bytes(C, BC)};
}

// The N-best of next() (beamformer.cc:3223-3245, modalBeamformer.cc:922-946) and of _getNBestHypothesesFromACCRP (beamformer.cc:2986-3025):
// R descending, I the unit of each rank; an empty rank is rp -10e10, unit -1 (DOA (-pi, -pi)).  Strict >: on a tie the earlier unit wins.
__host__ __device__ __forceinline__ void nbest_reset(double* R, int* I, int nBest)
{
  for (int n = 0; n < nBest; n++) { R[n] = -10e10; I[n] = -1; }
}
__host__ __device__ __forceinline__ void nbest_insert(double* R, int* I, int nBest, double v, int k)
{
  if (!(v > R[nBest - 1])) return;
  for (int n1 = 0; n1 < nBest; n1++)
    if (v > R[n1]) {
      for (int n2 = nBest - 1; n2 > n1; n2--) { R[n2] = R[n2 - 1]; I[n2] = I[n2 - 1]; }
      R[n1] = v; I[n1] = k; return;
    }
}
// _getNBestHypothesesFromACCRP over acc [U][nUnits]: R, I [U][nBest]
inline void final_nbest(const double* acc, int U, int nUnits, int nBest, double* R, int32_t* I)
{
  for (int u = 0; u < U; u++) {
    nbest_reset(R + (size_t) u * nBest, I + (size_t) u * nBest, nBest);
    for (int k = 0; k < nUnits; k++) nbest_insert(R + (size_t) u * nBest, I + (size_t) u * nBest, nBest, acc[(size_t) u * nUnits + k], k);
  }
}

inline void check_range(int fbinMin, int fbinMax, int M, int tblFbinMax)
{
  if (fbinMin < 0 || fbinMin > fbinMax || fbinMax > M / 2)
    throw Error(DSR_E_DIMENSION, "frequency range [%d, %d] outside [0, %d]", fbinMin, fbinMax, M / 2);
  if (fbinMax > tblFbinMax)                                  // the table's bins end at the fbinMax it was built with (:3125-3127)
    throw Error(DSR_E_DIMENSION, "fbinMax %d beyond the steering table built for bins up to %d (setSearchParam rebuilds it)", fbinMax, tblFbinMax);
}

// bins f0 .. f0 + nb - 1 of the workgroup's FB frames from t0 on into xs [C][FB][BP], zero past nb and from frame N on; between two barriers
__device__ __forceinline__ void srp_stage_chunk(float2* xs, const float2* __restrict__ Xu, int C, int Tmax, int F, int BC, int BP, int t0, int N, int f0, int nb)
{
  __syncthreads();
  for (int idx = threadIdx.x; idx < C * FB * BC; idx += 256) {
    const int b = idx % BC, r = idx / BC, t = r % FB, c = r / FB;
    float2 v = make_float2(0.f, 0.f);
    if (b < nb && t0 + t < N) v = Xu[((long) c * Tmax + t0 + t) * F + f0 + b];
    xs[(c * FB + t) * BP + b] = v;
  }
  __syncthreads();
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

// rp += g |c|^2 of a 16-unit tile (cr, ci) at bin f; Y (optional): row yrow gets the last unit's beamformed value when this is its tile
__device__ __forceinline__ void srp_accumulate(d4& rp, const d4& cr, const d4& ci, double g, float2* __restrict__ Y, bool lastTile, int lastRow, int kq,
                                               bool live, long yrow, int F, int f)
{
#pragma unroll
  for (int q = 0; q < 4; q++) rp[q] += g * (cr[q] * cr[q] + ci[q] * ci[q]);
  if (Y && lastTile) {
#pragma unroll
    for (int q = 0; q < 4; q++)
      if (kq + 4 * q == lastRow && live) Y[yrow * F + f] = make_float2((float) cr[q], (float) ci[q]);
  }
}
// rpOut[row][unit] = rp / nbins for the workgroup's TG tiles from th0 on (_calcResponsePower's division, :3184)
template <int TG>
__device__ __forceinline__ void srp_write_rp(const d4 (&rp)[TG], int th0, int NT, int kq, int nUnits, bool live, long row, int fbinMin, int fbinMax,
                                             double* __restrict__ rpOut)
{
  const double nbins = (double) (fbinMax - fbinMin + 1);
#pragma unroll
  for (int tg = 0; tg < TG; tg++) {
    const int th = th0 + tg;
    if (th >= NT) break;
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int r = th * 16 + kq + 4 * q;
      if (r < nUnits && live) rpOut[row * nUnits + r] = rp[tg][q] / nbins;
    }
  }
}

// ---- k_doa.hip ----
// k_doa_srp over s's table (uploaded when dirty): rp [U][Tmax][nTheta], energy [U][Tmax], Y (optional) the last unit's bins
void doa_launch_rp(dsr_doa& s, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st);
// k_doa_acc: acc[u][k] += rp of every frame t < nframes[u] with energy >= thr, in frame order
void doa_launch_acc(const double* rp, const float* en, const int* nf, int U, int Tmax, int nUnits, float thr, double* acc, hipStream_t st);
// k_doa_frame: the energy gate (gated, optional) and the N-best nbRp, nbIdx [U][Tmax][nBest] of every frame t < nframes[u]
void doa_launch_frame(const double* rp, const float* en, const int* nf, int U, int Tmax, int nUnits, int nBest, float thr, double* nbRp, int* nbIdx,
                      int* gated, hipStream_t st);

}  // namespace dsr
