// csrc/adapt.h -- MLLR speaker adaptation as adapt.cpp (parameter trees, host) and k_mllr.hip (statistics, solves, mean transforms, device)
// share it.  Replaces the MLLR branch of asr/adapt/transform.{h,cc} ("tr": ParamBase, MLLRParam, ParamTree, MLLRTransformer, TransformerTree)
// and asr/train/estimateAdapt.{h,cc} ("eA": GaussListTrain, MLLREstimatorAdapt, EstimatorTree, EstimatorTreeMLLR).
#pragma once
#include "gmm_model.h"
#include <map>
#include <string>
#include <vector>

namespace dsr {

bool isAncestor(unsigned ancestor, unsigned child);      // tr:133-145

// the symbols of a speaker parameter file, shared with apt.cpp: ParamBase::_symMap (tr:203-208), _getSymbol (tr:219-242), _getAdaptType (tr:244-267)
enum Symbol { SymRegClass = 0, SymRAPT, SymSLAPT, SymMLLR, SymSTC, SymLDA, SymBias, SymEndClass, SymAdaptType, SymEOF, SymNull };
extern const char* kSymMap[];
Symbol getSymbol(FILE* fp);
int getAdaptType(FILE* fp);                              // 0 RAPT, 1 SLAPT, 2 MLLR

// MLLRParam (tr:556-650): the size x size matrix and the bias (W's last column), both double
struct MLLRParam {
  unsigned regClass = 0; int size = 0;
  std::vector<double> matrix, bias;
  void assign(int D, const double* W);                    // operator=(const gsl_matrix*) tr:622-650, W [D][D + 1]
};

enum { kAdaptUnspecified = 0, kAdaptMLLR = 3 };          // AdaptationType: only MLLR is implemented

// ParamTree (tr:789-950) of MLLR parameters
struct ParamTree {
  std::map<unsigned, MLLRParam> map; int type = kAdaptUnspecified;
  void clear() { type = kAdaptUnspecified; map.clear(); }
  bool hasIndex(unsigned rc) const { return map.count(rc) != 0; }
  MLLRParam& find(unsigned rc, bool useAncestor);         // tr:835-860
  MLLRParam& findMLLR(unsigned rc, bool useAncestor);     // tr:898-925
  void read(const char* fileName);                        // tr:927-950
  void write(const char* fileName) const;                 // tr:824-833
};

}  // namespace dsr

struct dsr_param_tree : dsr::ParamTree {};

namespace dsr {

// one step of LeafIterator::estimate (eA:3105-3133): estimate at `node` and store under leaf and node, or copy from the nearest ancestor
struct MllrStep { int speaker, node, leaf, copy; };

struct MllrHandle {
  int S = 0, D = 0, G = 0;
  std::vector<float> origMean, ivar;                      // [G][D] CodebookAdapt::_origRV and the inverse variances
  std::vector<uint16_t> regClass;                         // [G]; empty: the model had no table (every class is 0)
  std::vector<dsr_param_tree> tree;                           // [S]
  std::vector<int> status;                                // [S] of the last estimate: 0 or DSR_E_CONSISTENCY
  std::vector<MllrStep> plan;                             // of the last estimate
  // the regression tree of the last estimate
  std::vector<unsigned> leaves, nodes;                    // ascending
  std::vector<double> ttl;                                // [S][nodes]
  int NCp = 0, PZ = 0;                                    // columns of a statistics row (padded), first z column
  DevBuf<float> d_mean, d_ivar;                           // [G][D]
  DevBuf<double> d_c, d_sumO;                             // [S][G], [S][G][D]
  DevBuf<int> d_gidx, d_chunk, d_pq, d_leafChunk, d_nodeLeafStart, d_nodeLeaf, d_solve, d_flag, d_map;
  DevBuf<double> d_part, d_partTtl, d_stats, d_ttl, d_W, d_Wtab;
  DevBuf<float> d_out;
  bool timing = false; float ms[3] = {0.f, 0.f, 0.f};     // statistics + reduction, solve, apply
};

}  // namespace dsr

struct dsr_mllr : dsr::MllrHandle {};
struct dsr_train;

namespace dsr {
// count - denCount and sumO of a trainer's accumulator rows into device arrays c [G], sumO [G][D] (k_mllr_take); dsr_apt_set_stats shares it
void take_stats(const dsr_train& t, int G, int D, double* c, double* sumO);
// the same with sumOsq [G][D] (or NULL); dsr_sat_set_stats uses it
void take_stats_sq(const dsr_train& t, int G, int D, double* c, double* sumO, double* sumOsq);
}  // namespace dsr
