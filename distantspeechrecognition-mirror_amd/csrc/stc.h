// csrc/stc.h -- semi-tied covariance (STC) and LDA transform estimation as stc.cpp (accumulator arithmetic, files, host), k_stc.hip (nearest
// Gaussian, statistics, estimation and the transforms on the device) and streams_asr.cpp (the stream operators) share it.
// Replaces STCTransformer / LDATransformer (asr/adapt/transform.cc:1788-1984, "tr") and STCEstimator / LDAEstimator
// (asr/train/estimateAdapt.cc:2203-3036, "eA") for models of one sub-feature (nSubFeat = 1, subFeatLen = dimN).
#pragma once
#include "train.h"
#include <vector>

namespace dsr {

static constexpr int kStcMaxD = 64;                       // the LDS of k_lda_solve: three dimN x dimN matrices of doubles

// what both estimators need to turn (frame, distribution, factor, estimator) items into chunks of one estimator on the device
struct XfBase {
  dsr_gmm* g = nullptr;                                   // the model: its scoring tables find the nearest Gaussian; must outlive the handle
  int D = 0, G = 0, K = 0, nEst = 0;
  DevBuf<float> d_mean, d_ivar;                           // [G][D] copies made at creation: the operands of the statistics
  DevBuf<int> d_frame, d_dist, d_gsel, d_chunk, d_accChunk, d_flag;
  DevBuf<float> d_fac, d_score, d_featScore, d_featSrc;      // the latter two: dsr_*_upload_features
  DevBuf<double> d_part, d_stats;
  bool timing = false; float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};     // nearest, statistics + reduction, eigen-decompositions, rows, apply
  size_t msz() const { return (size_t) D * D; }
  void check_est(int e, const char* who) const { if (e < 0 || e >= nEst) throw Error(DSR_E_INDEX, "%s: estimator %d of %d", who, e, nEst); }
};

// The accumulators live on the host as the reference holds them (estimateAdapt.h: _sumOsq / _regSq, dimN matrices of dimN x dimN each, the
// lower triangle written by accumulation); the device forms one call's sums, the host adds them.
struct StcHandle : XfBase {
  bool cascade = false, mmi = false;
  std::vector<double> count, denCount, totalPr, E;        // [nEst]
  std::vector<unsigned> totalT;
  std::vector<double> sumOsq, regSq;                      // [nEst][D][D][D]
  std::vector<double> A, Ainv;                            // [nEst][D][D]: matrix() and _stcInv
  std::vector<int> status;                                // [nEst] of the last estimate: 0 or DSR_E_CONSISTENCY
  int NCp = 0, PZ = 0;                                    // columns of a statistics row (padded), first R column
  DevBuf<int> d_pq;
  DevBuf<double> d_G, d_Ginv, d_A, d_Ai, d_gamma, d_ev, d_Aall;
  bool aDirty = true;                                     // d_Aall is behind A
  size_t ssz() const { return (size_t) D * D * D; }
};

struct LdaHandle : XfBase {
  int globalRefN = 0;
  std::vector<float> mu0;                                 // [D] Gaussian 0 of the global codebook
  std::vector<double> count;                              // [nEst]
  std::vector<double> within, between, mixture;           // [nEst][D][D]
  std::vector<double> L;                                  // [nEst][D][D] the LDA matrix
  std::vector<double> ev;                                 // [nEst][2 D] of the last estimate: eigenvalues of within, of the whitened between (descending)
  std::vector<int> status;
  DevBuf<float> d_mu0;
  DevBuf<double> d_W, d_B, d_L, d_ev, d_Lall;
  bool lDirty = true;
};

void stc_apply(StcHandle& h, const float* x, long N, int estX, float* out, hipStream_t st);
void lda_apply(LdaHandle& h, const float* x, long N, int estX, int outDim, float* out, hipStream_t st);

}  // namespace dsr

struct dsr_stc : dsr::StcHandle {};
struct dsr_lda : dsr::LdaHandle {};
