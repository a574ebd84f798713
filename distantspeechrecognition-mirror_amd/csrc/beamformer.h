// csrc/beamformer.h -- what the linear-array subband beamformer's files share: the handle dsr_bf (BfState), the functions through which the host
// side (beamformer.cpp: weight design, the dsr_bf_* entries) reaches the kernels (k_beamform.hip), and what other units read of a beamformer:
// the fused analysis + beamformer entry (filterbank.cpp), the post-filter behind a beamformer (k_postfilter.hip) and the maximum-kurtosis /
// maximum-negentropy estimators (mk_minimize.h).
#pragma once
#include "common.h"
#include <complex>

namespace dsr {

typedef std::complex<double> zc;

struct BfState {
  int M = 0, C = 0, halfBandShift = 0, mode = 0;
  std::vector<zc> wq;      // [M][C]
  std::vector<zc> R;       // [M/2+1][C][C]
  bool haveR = false, haveWq = false, haveMvdr = false, haveB = false;
  std::vector<zc> mvdr;    // [M/2+1][C]
  std::vector<zc> B;       // [M][C][C-1]
  std::vector<zc> wa;      // [M][C-1]
  std::vector<zc> wl;      // [M][C]  B wa as of the last setActiveWeights_f / zeroActiveWeights (SubbandMVDRGSC reads this cached product)
  std::vector<zc> eff;     // [M/2+1][C] weights in use
  DevBuf<float2> d_w;      // [M/2+1][C]
  DevBuf<float2> d_wT;     // [C][M/2+2] the same weights channel-major (the fused analysis + beamformer kernel reads a channel's row coalesced)
  bool dirty = true;
  // SubbandGSCRLS (beamformer.h:213-262): recursive-least-squares adaptation of the active weights
  bool rlsOn = false, rlsAdapt = true, haveP0 = false; double rlsMyu = 0.9, rlsAlpha = -1.0; int rlsQc = 0;
  std::vector<double> rlsDiag;   // [M/2+1] _diagonalWeights (the constructor's sigma2)
  std::vector<zc> rlsP0;         // [M/2+1][C-1][C-1] precision matrices every utterance starts from
  DevBuf<double2> d_wq, d_B, d_P0, d_state; DevBuf<double> d_diag; bool rlsDirty = true;
  // carried adaptation state (dsr_bf_rls_carry): [entry][U x F] precision matrices + active weights as the last call left them; the next call of
  // the same batch shape continues from it -- block streaming, and the reference's "keeps adapting across reset()" (beamformer.cc:1552-1612)
  bool rlsCarry = false, rlsHaveState = false; int rlsStateU = 0; DevBuf<double2> d_carry;
  PerStream<DevBuf<float2>> d_wB;   // blockingMatrixOutput's weights, one image per stream
};

}  // namespace dsr

struct dsr_bf : dsr::BfState {};

namespace dsr {

// ---- beamformer.cpp ----
// the weights k_bf_apply would use, channel-major [C][M/2+2] on the device, for the fused analysis + beamformer kernel (dsr_fb_analysis_beamform, filterbank.cpp, hands them to k_filterbank.hip); null when the output is
// not a fixed linear combination of the channels (SubbandGSCRLS adapting) or when all M bins are computed (halfBandShift)
bool bf_has_fixed_weights(const dsr_bf* s);
const float2* bf_fixed_weights_dev(dsr_bf* s);
// the quiescent vectors [M][C] and blocking matrices [M][C][C-1] calcGSCWeights left, for the maximum-kurtosis estimator (k_mk.hip); false without them
bool bf_gsc_fixed_weights(const dsr_bf* s, int* M, int* C, int* halfBandShift, const zc** wq, const zc** B);

// ---- k_beamform.hip ----
// Y [U][Tmax][F] = sum_c conj(W[f][c]) X[u][c][t][f] with the device weights W [F][C]
void bf_launch_apply(const float* X, const float2* W, int C, int F, int U, int Tmax, float* Y, hipStream_t st);
// the kernel the RLS launch picks for C channels, and where a thread's precision matrix and active weights live
struct RlsPath { int ct, cap, residence; size_t stateBytes, ldsBytes; };
RlsPath rls_path(int C);
// k_gsc_rls over the uploaded wq, B, P0 and diagonal weights of s; sizes the working and the carried state
void bf_launch_rls(BfState& s, const float* X, const int32_t* nframes, int U, int Tmax, float* Y, double* waOut, hipStream_t st);

}  // namespace dsr
