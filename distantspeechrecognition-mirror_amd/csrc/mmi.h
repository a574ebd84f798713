// csrc/mmi.h -- what SubbandMMI's two files share: the handle dsr_mmi with each source's weights, and the launcher through which the host side
// (mmi.cpp: weight design, the dsr_mmi_* entries) reaches the frame loop (k_mmi.hip).
#pragma once
#include "common.h"
#include <complex>

namespace dsr {

typedef std::complex<double> zc;

struct SrcW { std::vector<zc> wq, B, wa, wl, ta; };     // [M][C], [M][C][C-NC], [M][C-NC], [M][C], [M][C]

}  // namespace dsr

struct dsr_mmi {
  int M = 0, C = 0, hbs = 0, target = 0, S = 2, pfType = 0, NC = 1; double alpha = 0.9;
  bool haveW = false, dirty = true;
  bool useMask = false; double avgFactor = -1.0; unsigned fwidth = 1, maskType = 0;
  std::vector<dsr::SrcW> src;
  dsr::DevBuf<double2> d_weff, d_wup, d_mani, d_csd, d_ta;
};

namespace dsr {

// k_mmi.hip: Y [U][Tmax][dsr_mmi_out_bins] from the snapshots X [U][C][Tmax][F] with the weights in m.d_weff, m.d_wup, m.d_mani; sizes the densities and the scratch
void mmi_launch(dsr_mmi& m, const float* X, const int* nf, int U, int Tmax, float* Y, hipStream_t st);

}  // namespace dsr
