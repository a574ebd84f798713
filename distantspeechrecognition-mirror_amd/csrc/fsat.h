// csrc/fsat.h -- fast speaker-adaptive training as fsat.cpp (the handle, the fast-accumulator file, the update's bookkeeping, the file-driven
// estimate; host) and fsat_kernels.hip (the fold of speaker statistics into the fast accumulators, their addition into the SAT sums, the
// MDL mean solve with the joint variance update; device) share it.  Replaces CodebookFastSAT::FastAccu / GaussDensity::normFastAccu /
// descLen and CodebookSetFastSAT (asr/sat/codebookFastSAT.cc, "cfs"), MDLSATMean and FastSAT (asr/sat/sat.cc:383-587, "sat"),
// SATBase::FastAcc (sat:1028-1104) and SATFast<FastAcc> = FastMeanVarianceSAT (sat.h:803-844) for the model scope of sat.h.
#pragma once
#include "sat.h"

namespace dsr {

constexpr double kFsatSmallCk = 1.0e-06;                  // GaussDensity::Small_ck, cfs:344
constexpr int kFsatJobs = (kSatTileG * (kSatMaxBlock + 1) + 255) / 256;   // outputs a thread of k_fsat_norm owns at the largest block

struct FsatHandle {
  dsr_sat* sat = nullptr;                                 // owned: the slots, their transforms, and the SAT sums mat / vec / scalar / occ / varVec
  int S = 0, D = 0, G = 0;
  double lhoodThreshold = 0.0; bool meanOnly = false;
  std::vector<char> full;                                 // [S]: the slot holds sumO and sumOsq, not counts alone
  DevBuf<double> d_num, d_den;                            // [S][G]: numProb and denProb of every slot
  int fastBlocks = 0;                                     // nblks of the fast accumulators; 0: not allocated (_zeroFastAccs, cfs:688-695)
  DevBuf<double> d_fcount, d_fden, d_fmean, d_fvar, d_fscalar;   // [G], [G], [G][D], [G][D], [G][fastBlocks]
  DevBuf<int> d_flag;                                     // [1]: a scalar became NaN (cfs:407-408)
  int descBlocks = 0; std::vector<uint16_t> descLen;      // [G][descBlocks]: every block starts at 1 (cfs:523-539)
  std::vector<int> recDesc;                               // [G][nBlocks] of the last update: the description lengths it left
  DevBuf<int> d_desc, d_newDesc; DevBuf<float> d_newVar;  // [G][nBlocks] in and out of k_fsat_solve, [G][D]
  float ms[3] = {0.f, 0.f, 0.f};                          // k_fsat_norm, the matrix-only k_sat_mean_acc, k_fsat_solve of their last launch
};

// tables and tiles as sat_tables left them in the SatHandle
void fsat_norm(FsatHandle& f, const SatCall& c, hipStream_t st);
void fsat_add(FsatHandle& f, hipStream_t st);
void fsat_solve(FsatHandle& f, int nSolve, hipStream_t st);
void fsat_take_counts(FsatHandle& f, int s, const dsr_train& t);

}  // namespace dsr

struct dsr_fsat : dsr::FsatHandle {};
