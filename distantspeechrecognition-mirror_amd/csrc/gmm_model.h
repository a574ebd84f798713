// csrc/gmm_model.h -- the codebook/distribution set as k_gmm.hip and k_gmm_mfma.hip share it (one definition for both translation units).
#pragma once
#include "common.h"
#include <string>
#include <vector>

namespace dsr {

// what the MFMA scoring path hands from its contraction kernel to its near-tie kernel: owned by the model, ONE PER STREAM (two pipes on two
// HIP streams may score with the same model at the same time; within a stream the two launches are ordered)
struct GmmTieScratch { DevBuf<unsigned long long> list; DevBuf<unsigned> count; DevBuf<unsigned> masks; };

struct GmmModel {
  int K = 0, D = 0, G = 0, maxRef = 0;
  std::vector<int> refN, off;
  std::vector<float> mean, ivar, det, val, scale, pi, count;
  std::vector<std::string> cbNames, dsNames;
  std::vector<uint16_t> regClass;    // [G] first regression class of each Gaussian (CodebookBasic::_regClass[refX][1]); empty: no table
  DevBuf<int> d_off;                 // [K+1]
  DevBuf<float> d_mean, d_ivar;      // [G][Dp]  (rows padded to Dp = multiple of 4)
  DevBuf<float> d_cst;               // [G] pi+det
  DevBuf<float> d_val, d_scale;      // [G], [K]
  int Dp = 0;
  // MFMA operand image (built lazily)
  bool mfmaReady = false; int KP = 0, GT = 0;
  DevBuf<float> d_A;                 // [GT][KP/2][64]
  DevBuf<float> d_bn;                // the same operand, four consecutive steps of a lane side by side
  DevBuf<int> d_tileCb;              // codebook ids per 32-Gaussian tile (uniform refN=16 path)
  // bound on the magnitude of the expanded form's terms: sum |terms| <= 2 (ivMax |x|^2 + muIvMax) + cstMax for every Gaussian of the model
  float ivMax = 0.0f, termMax = 0.0f;
  PerStream<GmmTieScratch> tie;
};

// The trust radius of the expanded form as a multiple of S = 2 ivMax |x|^2 + termMax (k_gmm_mfma.hip header): two computed distances further apart
// than twice the rounding bound (2 dimN + 3) 2^-24 S, plus what the search itself may move a compared value by, keep the order of the exact ones.
// tagValues: how many index values the search writes into the low mantissa bits of the values it compares (0: none).  Such a value is off its
// distance by less than tagValues ulp <= tagValues 2^-23 |d| <= tagValues 2^-23 S; twice that is budgeted (the roundings of the test itself).
// `tuned` is the literal the kernels were measured with: the radius never falls below it, so shapes it covers keep their scores bit for bit.
inline float gmm_trust_radius(int D, float tuned, int tagValues)
{
  const float r = (float) (2.0 * (2 * D + 3) * 0x1p-24 + tagValues * 0x1p-22);
  return r > tuned ? r : tuned;
}

// k_gmm_sp.hip: the software-pipelined MFMA shape for codebooks of four Gaussians
int gmm_sp_frames();
size_t gmm_sp_lds(const GmmModel& m);
bool gmm_sp_has(int S4, int R);
bool gmm_sp_launch(GmmModel& m, int R, const float* x, long N, float* score, unsigned char* argmin, DevBuf<unsigned>& masks, unsigned long long* tieList, unsigned* tieCount, unsigned cap, hipStream_t st);

}  // namespace dsr
