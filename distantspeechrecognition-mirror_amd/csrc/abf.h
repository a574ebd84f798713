// csrc/abf.h -- what the adaptive subband beamformers of btk/lib/subbandBeamforming.py share: the handle dsr_abf (AbfState), the dispatch
// (abf_path) and the launch.  Host side (set-up helpers, the dsr_abf_* entries): csrc/abf.cpp; kernels and launch: csrc/abf_kernels.hip.
#pragma once
#include "common.h"
#include <complex>

namespace dsr {

typedef std::complex<double> zc;

// the constructor parameters of SubbandBeamformerGriffithsJim (subbandBeamforming.py:989-1005) and of SubbandBeamformerMVDR / MPDR (:1110-1121, :1188-1198)
struct AbfParams {
  double beta = 0.999, gamma = 0.0005, initDiagLoad = 1.0e10, floorSb = 2.0e7, silThresh = 1.0e10, alpha2 = 0.001; int staticAfter = 1000;
  double diagLoad = 0.001, lambda = 0.99; int end = 20;
};

struct AbfState {
  int kind = 0, M = 0, C = 0, NC = 1;
  AbfParams p;
  std::vector<zc> wq, B, wa;      // [F][C], [F][C][C-NC], [F][C-NC] (the static GSC's active weights)
  bool haveWq = false, haveB = false, dirty = true;
  bool spkr = false;              // Griffiths-Jim: nextSpkr() creates the state (:1092-1104); iterating before it is an error
  // carried state: [entry][U x F] per (utterance, bin) + [U][4] per utterance (frame counter, gamma, average power)
  bool carry = false, haveState = false; int stateU = 0;
  DevBuf<double2> d_wq, d_B, d_weff, d_work, d_carry;
  DevBuf<double> d_utt, d_sig, d_gam; DevBuf<int> d_start;
};

// the cell a launch takes: the compile-time channel count (0: run-time), the capacity of a thread's vectors, where the state lives, the state and
// factor entries (complex fp64) of a thread, the bytes the 64 lanes' state and factor take (what the LDS gate compares) and the launch's dynamic LDS
struct AbfPath { int ct, cap, residence, stateN, factorN; size_t stateBytes, ldsBytes; };
AbfPath abf_path(int kind, int C);
// the frame-power pass, the per-utterance scan and the recursion kernel of s.kind over the uploaded weights; sizes the working and the carried state
void abf_launch(AbfState& s, const float* X, const int32_t* nframes, int U, int Tmax, const float* wp, const int32_t* wpFrames, float* Y, double* wOut,
                hipStream_t st);

}  // namespace dsr

struct dsr_abf : dsr::AbfState {};
