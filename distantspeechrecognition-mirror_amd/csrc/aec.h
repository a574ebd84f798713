// csrc/aec.h -- the echo canceller handle of include/dsr.h section 2d, shared by k_aec.hip (NLMS, Kalman, block, DTD) and k_aec_info.hip (the
// information filter and its square-root form).  k_aec.hip owns the C entries and hands the two information kinds on to dsr::aec_info.
#pragma once
#include "common.h"

struct dsr_aec {
  int kind, M, L, frameMode = 0;
  double delta = 100.0, epsilon = 1.0e-4, threshold = 100.0;                       // cancelVP.i:80-81
  double beta = 0.95, sigma2 = 5.0, sigmau2 = 10e-4, sigmak2 = 5.0, amp = 1.0;     // cancelVP.i:108-109, :140-143
  double engTh = 100.0, smooth = 0.9;                                              // cancelVP.i:241-244 (snrTh is `threshold`, cancelVP.cc:1061)
  double loading = 1.0e-2;                                                         // cancelVP.i:163, :197
};

namespace dsr {
namespace aec_info {
inline bool is_info(const dsr_aec& a) { return a.kind == DSR_AEC_INFO || a.kind == DSR_AEC_SQRT_INFO; }
size_t state_bytes(const dsr_aec& a, int U);
void init_state(const dsr_aec& a, void* state, int U, hipStream_t st);
// state == nullptr: a fresh state in per-stream scratch, discarded
void apply(const dsr_aec& a, const float2* V, const float2* A, const int* nf, int U, int Tmax, int frame0, float2* out, void* state, hipStream_t st);
void read(const dsr_aec& a, const void* state, int U, int what, double* host_out, size_t outDoubles);
}  // namespace aec_info
}  // namespace dsr
