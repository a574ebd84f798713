// csrc/sat.h -- speaker-adaptive training (ML-SAT) as sat.cpp (slot tables, speaker list, updates, the file-driven estimate; host) and
// sat_kernels.hip (mean and variance accumulators, the mean solve; device) share it.  Replaces the ML slice of asr/sat/sat.{h,cc} ("sat":
// SATMean 54-342, SATVariance 686-760, SATBase::MeanAcc 999-1025, SATBase::VarianceAcc 1194-1246, SATBase / SAT<Type> 1763-1855,
// TransformerTreeList::getTree 1884-1896) and SpeakerList (asr/adapt/transform.cc:1989-1998, "tr") for the diagonal 1:1 models of dsr_gmm.
#pragma once
#include "gmm_model.h"
#include <map>
#include <string>
#include <vector>

struct dsr_train;

namespace dsr {

enum { kSatMLLR = 1, kSatAPT = 2 };                       // whose transform() the variance accumulator restates: tr:1777-1784 or tr:1300-1336
enum { kSatMean = 1, kSatVariance = 2 };
constexpr int kSatMaxBlock = 81;                          // two bl^2 fp64 matrices of k_sat_solve fit the LDS (the bound of k_mllr_solve)
constexpr int kSatTileG = 16;                             // Gaussians of one class per workgroup of k_sat_mean_acc: the rows of one MFMA tile
constexpr int kSatColGroup = 256;                         // columns per workgroup: 4 waves x 4 tiles x 16

// the decision of SATMean::update for one (Gaussian, block)
enum { kSatLeft = 0, kSatUpdated = 1, kSatKeptOld = 2, kSatZeroed = 3, kSatFlagged = 4, kSatNaN = 5 };
struct SatRecord { int kept, decision; double auxOld, auxNew; };

// TransformMatrix of one (slot, class): nBlocks matrices bl x bl and the offsets of all blocks (tr:1339-1363, 1746-1768)
struct SatXform { int kind = 0, nBlocks = 0, bSize = 0; std::vector<double> A, b; };

struct SatHandle {
  dsr_train* tr = nullptr; GmmModel* g = nullptr;
  int S = 0, D = 0, G = 0, nParts = 1, part = 1, nBlocks = 0, bl = 0, aptSub = 1;
  double threshold = 10.0;                                // UpdateThreshhold (sat:1768)
  std::vector<std::map<unsigned, SatXform>> slot;         // [S]: class -> transform
  std::vector<SatRecord> rec;                             // [G][nBlocks] of the last mean update
  std::vector<double> sol;                                // [G][D] of the last mean update: the solved means in double (0 where none)
  std::vector<int> status;                                // [G] of the last mean update: 0, DSR_E_CONSISTENCY or DSR_E_NUMERIC
  bool keepTrn = false; int trnSlots = 0;
  DevBuf<double> d_c, d_sumO, d_sumOsq;                   // [S][G], [S][G][D], [S][G][D]
  DevBuf<double> d_macc, d_mocc, d_vvec, d_vocc;          // [G][nBlocks][bl^2 + bl + 1], [G], [G][D], [G]
  DevBuf<int> d_has;                                      // [G]: _checkBlocks has run (a non-zero count was seen)
  DevBuf<double> d_A, d_b, d_sol; DevBuf<int> d_kind, d_bsz;    // [slots][classes]...: the tables of one accumulate call
  DevBuf<int> d_gidx, d_tile, d_pq, d_cls, d_solve; DevBuf<float> d_mean, d_ivar, d_newMean, d_trn; DevBuf<SatRecord> d_rec;
  bool timing = false; float ms[3] = {0.f, 0.f, 0.f};     // k_sat_mean_acc, k_sat_var_acc, k_sat_solve of their last launch
  size_t stride() const { return (size_t) bl * bl + bl + 1; }
};

// what one accumulate call hands the kernels: the Gaussians [g0, g1) sorted by class and cut into tiles, and the table sizes
struct SatCall { int nSlots, NC, nB, bl, g0, g1, nTiles, PZ, NCp; };

void sat_mean_acc(SatHandle& h, const SatCall& c, bool matOnly, hipStream_t st);   // matOnly: FastSAT::accumulate, mat and occ alone
void sat_var_acc(SatHandle& h, const SatCall& c, hipStream_t st);
void sat_solve(SatHandle& h, int nSolve, hipStream_t st);

std::vector<std::string> read_speaker_list(const char* fileName);      // tr:1989-1998

// sat.cpp, as fsat.cpp uses them on the SatHandle it owns.
// sat_tables: the transformer of every (slot, class of a Gaussian in [g0, g1)) checked (tr:2165-2173) and uploaded with the class of every
// Gaussian; gidx / tile: the Gaussians sorted by class and cut into tiles of kSatTileG that do not cross a class
void sat_tables(SatHandle& h, int nSlots, int g0, int g1, SatCall& c, std::vector<int>& gidx, std::vector<int>& tile, hipStream_t st);
void sat_accumulate(SatHandle& h, int what, bool matOnly, int nSlots, hipStream_t st);
void sat_read_params(SatHandle& h, int s, const std::string& fileName);
void sat_part_gaussians(const SatHandle& h, int& g0, int& g1);

}  // namespace dsr

struct dsr_sat : dsr::SatHandle {};
