// csrc/sph.h -- what the spherical-array beamformer's two files share: the handle dsr_sph, its limits and kind predicates, and the functions
// through which the host side (sph.cpp: weight design, tables, the dsr_sph_* entries) reaches the kernels (k_sph.hip).
#pragma once
#include "srp_common.h"
#include <complex>

namespace dsr {

constexpr double SSPEED = 343740.0;                          // mm/s (beamformer.h:47)
constexpr int MAX_ORDER = 8;                                 // dim = maxOrder^2 <= 64: four 16-row tiles of the fused kernel
constexpr int MAX_BEAMS = 16;                               // one MFMA row tile
constexpr long MAX_TABLE = 1L << 27;                         // (fbinMax+1) units max(dim, C) complex128 entries: 2 GiB per table copy

}  // namespace dsr

struct dsr_sph {
  typedef std::complex<double> zc;
  int kind = DSR_SPH_EB, nBest = 1, M = 0, C = 0, maxOrder = 1, dim = 1; unsigned sampleRate = 16000; bool normalize = false;
  float sigma2 = 0.0f, wgain = 1.0f;
  double a = 0.0; std::vector<double> thS, phS;              // geometry: radius (mm) and the sensors' (theta_s, phi_s)
  double lookTheta = 0.0, lookPhi = 0.0;
  double minTheta = -M_PI, maxTheta = M_PI, minPhi = -M_PI, maxPhi = M_PI, widthTheta = 0.25, widthPhi = 0.25;  // DOAEstimatorSRPBase (beamformer.cc:2922-2938)
  int fbinMin = 1, fbinMax = 0; float threshold = 0.0f;
  std::vector<zc> B, SH;                                     // B [M/2+1][maxOrder], SH [dim][C] (conj Y at the sensors); empty until the geometry is set
  std::vector<zc> look; bool lookDirty = true;               // look [M/2+1][dim]: bin 0 the DC weights
  bool tbl = false; unsigned tableGen = 0; int nTheta = 0, nPhi = 0, tblFbinMax = 0;
  unsigned settingsGen = 0;                                  // bumped by every geometry / look-direction / sigma2 / gain change
  std::vector<double> uTheta, uPhi; std::vector<zc> W;       // W [tblFbinMax+1][units][dim]
  dsr::DevBuf<double2> dS, dSp, dLook, dWp; bool dSDirty = true, dLookDirty = true, dWDirty = true; int NT = 0, DT = 0, KS = 0;
  dsr_doa fold; unsigned foldGen = ~0u;                      // the folded path's [units][C] table, driven through k_doa_srp
  dsr::PerStream<dsr::DevBuf<double>> ws;
  // the further kinds
  float ratio = 1.0f; int NC = 1; bool lookSet = false;      // HWNC's _ratio; the GSC kinds' number of constraints; setLookDirection called
  std::vector<zc> Bm, wl;                                    // GSC: B [M/2+1][dim][dim-NC] (bin 0 stays zero), wl [M/2+1][dim] = B wa as last set
  std::vector<float> diag; bool fixedTerms = false;          // MOEN: _diagonalWeights [M/2+1], _isTermFixed
  std::vector<zc> fixedW; bool fixedWValid = false;          // MOEN: (A^H A + l I)^+ A^H [M/2+1][C][dim] (bin 0 unused), direction independent
  double beamTheta[dsr::MAX_BEAMS] = {0}, beamPhi[dsr::MAX_BEAMS] = {0}; bool beamSet[dsr::MAX_BEAMS] = {false}; unsigned beamGen = 0;   // beams 1.. (0 is the look direction)
  std::vector<zc> V; int vNB = 0; unsigned vSetGen = ~0u, vBeamGen = ~0u;   // V [NB][M/2+1][C]: y = v^H x
  dsr::DevBuf<double2> dV; int dVLayout = -1; bool dVDirty = true; // device copy, conjugated: layout 0 MFMA [F][KS][64], n > 0 VALU [C][n][F]
};

namespace dsr {

inline bool hwnc(int kind) { return kind == DSR_SPH_HWNC || kind == DSR_SPH_HWNCGSC; }
inline bool gsc_kind(int kind) { return kind == DSR_SPH_GSC || kind == DSR_SPH_HWNCGSC; }
inline bool sensor_kind(int kind) { return kind == DSR_SPH_SPATIALDS || kind == DSR_SPH_MOEN; }   // weights of length C, no transform

inline int units(const dsr_sph& s) { return s.nTheta * s.nPhi; }

// ---- k_sph.hip ----
int sph_beams_path(int NB);                                  // 0 VALU, 1 MFMA, as NB and DSR_SPH_BEAMS_PATH say
int sph_beams_path_for(int NB, int F);                       // the kernel of one call: sph_beams_path unless the VALU kernel's table does not fit
int sph_srp_path(const dsr_sph& s);                          // 0 fused, 1 folded, as the flop count and DSR_SPH_SRP_PATH say
// the launches as the queries report them (dsr_sph_srp_cell, dsr_sph_beams_cell); the launchers switch on the same values
struct SphSrpCell { int path, TG, DT, BC, KS; size_t ldsBytes; };             // path 0: k_sph_srp<TG, DT>; path 1: k_doa_srp<TG> on the folded table, DT 0
struct SphBeamsCell { int kernel, rows, CC, BCT, KS; size_t ldsBytes; };      // kernel 0: k_sph_beams_valu<rows, .>, CC channels staged; 1: k_sph_beams_mfma<BCT>
SphSrpCell sph_fused_cell(const dsr_sph& s);                 // needs the steering table's grid (units)
SphBeamsCell sph_beams_cell(int NB, int C, int F);           // follows DSR_SPH_BEAMS_PATH; DSR_E_DIMENSION where a forced VALU table does not fit
// Y [U][Tmax][F] = w^H (S X) with the weights in s.dLook, Fo (optional) [U][Tmax][F][dim] = S X; uploads S when it moved
void sph_apply(dsr_sph& s, const float* X, const int* nf, int U, int Tmax, float* Y, float* Fo, hipStream_t st);
// Y [U][NB][Tmax][F] = v_b^H X for the beams of s.V, on the kernel of `path`; uploads the vectors in that kernel's layout when they moved
void sph_beams(dsr_sph& s, const float* X, const int* nf, int U, int Tmax, int NB, int path, float* Y, hipStream_t st);
// the fused SRP: rp [U][Tmax][units], energy [U][Tmax], Y (optional) the last unit's bins; uploads S and the steering table when they moved
void sph_srp_fused(dsr_sph& s, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st);
// the gate and the N-best of every frame from rp and the energy
void sph_frame(const dsr_sph& s, const double* rp, const float* en, const int* nf, int U, int Tmax, double* nbRp, int* nbIdx, int* gated, hipStream_t st);

}  // namespace dsr
