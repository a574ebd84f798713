// csrc/fsa.h -- feature-space adaptation (constrained MLLR) as fsa.cpp (accumulator arithmetic, files, host), k_fsa.hip (nearest Gaussian,
// statistics, estimation and the transform on the device) and streams_asr.cpp (the stream operator) share it.
// Replaces FeatureSpaceAdaptationFeature (asr/train/fsa.{h,cc}, "fsa").
#pragma once
#include "train.h"
#include <vector>

namespace dsr {

static constexpr int kFsaMaxD = 80;                       // the LDS of k_fsa_eig / k_fsa_rows, as for MLLR

// The accumulators live on the host as the reference holds them (fsa.h: _count double, _beta float, _z [dimN][dimN + 1], _Gi [dimN] matrices of
// (dimN + 1)^2 with the lower triangle and column 0 written by accumulation); the device forms one call's sums, the host adds them.
struct FsaHandle {
  dsr_gmm* g = nullptr;                                   // the model: its scoring tables find the nearest Gaussian; must outlive the handle
  int D = 0, G = 0, K = 0, maxRef = 0, nAccu = 0, nTran = 0;
  std::vector<unsigned char> on;                          // [K] _dsXA
  unsigned topN = 1; float shift = 1.0f;
  std::vector<double> count; std::vector<float> beta;     // [nAccu]
  std::vector<double> z, Gi;                              // [nAccu][D][D + 1], [nAccu][D][D + 1][D + 1]
  std::vector<double> W;                                  // [nTran][D][D + 1], column 0 the bias
  std::vector<int> status;                                // [nTran] of the last estimate: 0 or DSR_E_CONSISTENCY
  int NCp = 0, PZ = 0;                                    // columns of a statistics row (padded), first z column
  DevBuf<float> d_mean, d_ivar;                           // [G][D] copies made at creation: the operands of the statistics
  DevBuf<int> d_pq, d_frame, d_dist, d_gsel, d_chunk, d_accChunk, d_flag;
  DevBuf<float> d_gamma, d_featScore, d_featSrc;         // the latter two: dsr_fsa_upload_features
  DevBuf<double> d_part, d_stats, d_G, d_z, d_Ginv, d_W, d_beta, d_Wall;
  bool wDirty = true;                                     // d_Wall is behind W
  bool timing = false; float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};     // nearest, statistics + reduction, eig, rows, apply
  size_t zsz() const { return (size_t) D * (D + 1); }
  size_t gsz() const { return (size_t) D * (D + 1) * (D + 1); }
  void check_accu(int a, const char* who) const { if (a < 0 || a >= nAccu) throw Error(DSR_E_INDEX, "%s: Bad accu index: %d should be less then %d.", who, a, nAccu); }
  void check_tran(int t, const char* who) const { if (t < 0 || t >= nTran) throw Error(DSR_E_INDEX, "%s: Bad transformation index: %d should be less then %d.", who, t, nTran); }
};

// x [N][D] -> out [N][D] with W[tranOfRow[n]] (tranOfRow == nullptr: transform 0), FeatureSpaceAdaptationFeature::next (fsa:247-280)
void fsa_apply(FsaHandle& h, const float* x, const int* tranOfRow, long N, float shift, float* out, hipStream_t st);

}  // namespace dsr

struct dsr_fsa : dsr::FsaHandle {};
