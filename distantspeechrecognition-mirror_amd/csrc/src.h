// csrc/src.h -- what the sample-rate converter (dsr_src_*, include/dsr.h section 6d) shares: the handle dsr_src (SrcState), the dispatch (src_path)
// and the launch.  Host side (the coefficient table, the dsr_src_* entries): csrc/src.cpp; kernels and launch: csrc/src_kernels.hip.
#pragma once
#include "common.h"

namespace dsr {

enum { SRC_FASTEST = 0, SRC_MEDIUM = 1, SRC_BEST = 2, SRC_ZOH = 3, SRC_LINEAR = 4 };

// The carried state the caller owns: [U] SrcCount, then [U][C][hist] floats, the last `hist` input samples of every row (SrcState::hist).
struct SrcCount { int64_t nin, nout; };

struct SrcState {
  unsigned srcRate = 0, dstRate = 0; int method = 0;
  int L = 1, M = 1, K = 0, taps = 0, stride = 0;      // taps = 2K of a sinc method; stride: floats between two rows of the uploaded table
  bool copy = false;                                  // srcRate == dstRate
  std::vector<float> table;                           // [L][stride]: row q holds the taps of phase (q M) mod L, j = -K+1 .. K, the rest of the row zero
  DevBuf<float> d_table; bool uploaded = false;
  int stateU = -1, stateC = -1;                       // the shape dsr_src_state_init saw last
  EventTimes<2> tm;                                   // dsr_src_set_timing: around the launch
  // the samples a row keeps: 2K for a sinc method.  zoh and linear keep ceil(M / L) more: the count floor(b L / M) can hold back an output whose taps
  // were all there (never with a sinc method, whose K L / M is at least 10), and its base lies up to ceil(M / L) samples back
  int hist() const { return copy ? 0 : method <= SRC_BEST ? 2 * K : 2 * K + (M + L - 1) / L; }
};

// the cell a launch takes: where the table is read from, where the input is read from, the outputs of a tile, the launch's dynamic LDS and the pitch
// between the outputs of neighbouring lanes
struct SrcPath { int table, input, run; size_t ldsBytes; int lanePitch; };
SrcPath src_path(const SrcState& s);
void src_launch(SrcState& s, const float* x, const int32_t* nsamp, int U, int C, long inStride, void* state, int flush, float* y, int32_t* nout,
                long outStride, hipStream_t st);

}  // namespace dsr

struct dsr_src : dsr::SrcState {};
