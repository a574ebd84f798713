// csrc/apt.h -- all-pass transform (APT) speaker adaptation as apt.cpp (parameters, their text files, the line search; host) and apt_kernels.hip
// (series, transform matrices, likelihoods, mean transforms; device) share it.  Replaces the one-parameter slice of asr/adapt/transform.{h,cc}
// ("tr": LaurentSeries, APTParamBase, RAPTParam, SLAPTParam, ParamTree::findAPT, BLTTransformer, SLAPTTransformer) and of
// asr/train/estimateAdapt.{h,cc} ("eA": EstimatorBase::bracket / brentsMethod, BLTEstimatorAdapt, SLAPTEstimatorAdapt with one parameter).
#pragma once
#include "gmm_model.h"
#include <map>
#include <vector>

namespace dsr {

enum { kAptUnspecified = 0, kAptRAPT = 1, kAptSLAPT = 2 };             // AdaptationType + 1, as kAdaptMLLR = 3 (adapt.h)
enum { kAptBiasNone = 0, kAptBiasCepstra = 1, kAptBiasAll = 2 };        // BiasType (eA:49-63)

constexpr int kAptSeriesLen = 150;                        // DefaultSeriesLength (transform.h:83): coefficients -149 .. 149
constexpr int kAptColumns = 50;                           // SLAPTTransformer::NoColumns (tr:1638)
constexpr int kAptMaxParams = 32;                         // all-pass parameters of one SLAPT transformer the kernel takes
constexpr int kAptMaxSub = 48;                            // subFeatLen: the transform matrix of k_apt_lhood sits in LDS

// APTParamBase (tr:410-441): _conf in double, the bias a NaturalVector of floats
struct AptParam {
  unsigned regClass = 0;
  std::vector<double> conf; std::vector<float> bias;
};

// the ParamTree (tr:789-950) of one speaker slot, of RAPTParam or of SLAPTParam
struct AptParams {
  std::map<unsigned, AptParam> map; int type = kAptUnspecified;
  void clear() { type = kAptUnspecified; map.clear(); }
  bool hasIndex(unsigned rc) const { return map.count(rc) != 0; }
  AptParam& findAPT(unsigned rc, int typ, bool useAncestor);           // tr:862-896
  void read(const char* fileName);                                     // tr:927-950 with ParamBase::param / _readParams (tr:339-407)
  void write(const char* fileName) const;                              // tr:824-833 with ParamBase::write (tr:365-372)
};

// EstimatorBase::bracket + brentsMethod (eA:109-240) for one (slot, node), fed the values it has asked for so far.
//   kind      kAptRAPT: b = 0, a = 0.1, range +-0.899 (eA:252-255, 1659-1665); kAptSLAPT: a = -0.05, b = 0, range +-100 (eA:821-826, 1544-1548)
//   lhood     calcLogLhood of the points the search evaluated so far, in its order
// -> kSearchNeeds: *point is the next point to evaluate; kSearchDone: *point = alpha / xmin; kSearchFailed: bracket met a NaN or Brent's
// method ran MaxItns iterations.  points (or NULL) receives the points evaluated so far.
enum { kSearchNeeds = 0, kSearchDone = 1, kSearchFailed = 2 };
constexpr int kSearchEvalCap = 400;                       // bracket's loop has no count of its own: more evaluations than this fail the search
int apt_line_search(int kind, const std::vector<double>& lhood, double* point, std::vector<double>* points);

}  // namespace dsr

struct dsr_apt_params : dsr::AptParams {};

namespace dsr {

struct AptStep { int speaker, node, leaf; };              // LeafIterator::estimate (eA:3105-3133): `leaf` was estimated at `node`

struct AptTrace { std::vector<double> point, lhood; std::vector<float> bias; };       // of one (slot, node): bias [evaluations][bSize]

struct AptHandle {
  int S = 0, D = 0, G = 0, kind = kAptSLAPT, L = 0, nSub = 0, biasType = kAptBiasNone, bSize = 0, paramN = 1;
  std::vector<float> origMean, ivar;                      // [G][D]
  std::vector<uint16_t> regClass;                         // [G]; empty: the model had no table
  std::vector<dsr_apt_params> store;                      // [S]
  std::vector<int> status;                                // [S] of the last estimate
  std::vector<AptStep> plan;
  std::vector<unsigned> leaves, nodes;                    // of the last estimate, ascending
  std::vector<double> ttl;                                // [S][nodes]
  std::map<std::pair<int, unsigned>, AptTrace> trace;     // (slot, node) of the last estimate
  int rounds = 0;
  DevBuf<float> d_mean, d_ivar, d_bias, d_tabBias, d_out;
  DevBuf<double> d_c, d_sumO, d_ecoef, d_conf, d_A, d_lhood;
  DevBuf<int> d_nPar, d_trial, d_gidx, d_nodeStart, d_map, d_tabBsz;
  bool timing = false; float ms[3] = {0.f, 0.f, 0.f};     // series + matrices, likelihoods (both summed over the rounds), apply
};

}  // namespace dsr

struct dsr_apt : dsr::AptHandle {};
