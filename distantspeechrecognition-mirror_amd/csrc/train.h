// csrc/train.h -- the training handle as k_train.hip (accumulation on the device) and train.cpp (updates, accumulator files) share it.
// Replaces CodebookTrain::Accu / DistribTrain::Accu (asr/train/codebookTrain.h, distribTrain.h) for the 1:1 diagonal models of dsr_gmm.
#pragma once
#include "gmm_model.h"
#include <vector>

struct dsr_gmm : dsr::GmmModel {};

namespace dsr {

void gmm_finish(GmmModel& m);                             // k_gmm.hip: offsets, padded device copies, mfmaReady = false

// The accumulators live on the device as one fp64 row per Gaussian: [sumO (D) | sumOsq (D) | count | denCount | distCount | distDenCount].
// Host entries pull the rows, work on them and push them back.
struct TrainAccu {
  GmmModel* g = nullptr;
  double minCount = 5.0;                                   // CodebookTrain::Accu::MinimumCount (cT:458), per handle
  int D = 0, G = 0, NA = 0;                                // NA = 2 D + 4 doubles per Gaussian
  DevBuf<double> d_acc;                                    // [G][NA]
  std::vector<double> h;                                   // host image, valid between pull() and push()
  // scratch of one accumulate call
  DevBuf<int> d_frame, d_dist, d_start, d_cstart; DevBuf<long long> d_gbase, d_chunk, d_pbase; DevBuf<float> d_factor, d_score, d_gamma; DevBuf<double> d_part; DevBuf<int> d_flag;
  DevBuf<float> d_feat;                                    // dsr_train_upload_features
  bool timing = false; float ms[2] = {0.f, 0.f};
  void resize();                                           // after create / split: G rows of zeros
  void pull(); void push();
  double* row(int gi) { return h.data() + (size_t) gi * NA; }
};

// the codebooks List::Iterator(lst, nParts, part) visits (btk/common/mlist.h:155-178): [first, last)
inline void part_range(int K, int nParts, int part, int& first, int& last)
{
  if (nParts < 1 || part < 1 || part > nParts) throw Error(DSR_E_PARAMETER, "bad nParts=%d part=%d", nParts, part);
  const int seg = K / nParts; first = (part - 1) * seg; last = part == nParts ? K : part * seg;
}

void train_accumulate(TrainAccu& t, const float* x, long N, const int* frame, const int* dist, const float* factor, long M, float* score, hipStream_t st);

}  // namespace dsr

struct dsr_train : dsr::TrainAccu {};
