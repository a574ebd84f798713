// csrc/mcc.h -- what the multichannel cross-correlation localiser's files share: the handles dsr_sgb (a search-grid builder) and dsr_mcc (a localiser
// over a built grid), and the function through which the host side (mcc.cpp: the search grids, the dsr_sgb_* / dsr_mcc_* entries) reaches the
// kernels (k_mcc.hip).
#pragma once
#include "common.h"

struct dsr_sgb {
  int kind, C, farField; unsigned fs; float maxTimeDelay = -1.0f, constV = 0.0f;
  std::vector<double> mpos, delays; double hypo[3] = {0.0, 0.0, 0.0};
};

struct dsr_mcc {
  int C, G, D, S; unsigned fs;
  std::vector<int> tau; std::vector<double> pos;      // [G][C], [G][3]
  dsr::DevBuf<int> d_tau, d_tau1; dsr::DevBuf<double> d_pos, d_pos1; bool uploaded = false;
  dsr::EventTimes<4> tm;                              // dsr_mcc_set_timing: around k_mcc_cost, k_mcc_nbest and k_mcc_eig
};

namespace dsr {

// ---- k_mcc.hip ----
// where a launch writes; a null part goes to the stream's scratch (eig, R: not computed)
struct MOut { int32_t* valid; int32_t* index; double* cost; int32_t* tau; double* pos; double* eig; double* costMap; double* R; };
// the three kernels over [U][B] blocks with a grid of G candidates (the localiser's table, or the calculator's single row); throws when the
// sample tile the LDS budget leaves is too short
void mcc_launch(dsr_mcc* m, const float* x, const int32_t* ns, int U, int N, int L, int G, const int* d_tau, const double* d_pos, int maxSource, int normalize,
                MOut o, hipStream_t st);

}  // namespace dsr
