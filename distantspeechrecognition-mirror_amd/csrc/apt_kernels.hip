// csrc/apt_kernels.hip -- all-pass transform (APT) speaker adaptation for a batch of speakers: the bilinear transform (BLT) and the sine-log
// all-pass transform (SLAPT) of the cepstral means, their one-parameter estimation, and the transformed means, on the device.
//
// Replaces LaurentSeries / CauchyProduct / multAdd / shift (asr/adapt/transform.cc:39-101, "tr"), APTTransformerBase::_calcTransMatrix and
// transform (tr:1212-1242, 1295-1337), BLTTransformer::bilinear (tr:1404-1414), SLAPTTransformer::_calcSequence (tr:1640-1650, 1716-1741),
// EstimatorAdapt::_calcBias / _calcMixLhood (asr/train/estimateAdapt.cc:1574-1620, "eA"), BLTEstimatorAdapt::calcLogLhood / estimate
// (eA:1638-1690), APTEstimatorAdaptBase::_accumLogLhood / estimate (eA:1851-1884, 1898-1929) with one parameter, LeafIterator::estimate
// (eA:3105-3133) and TransformerTree::transform (tr:2149-2163), which work on one speaker and one Gaussian at a time, for S speakers at once.
//
//   k_apt_matrix   workgroup per trial point: the Laurent series Q(z) (299 doubles) of the point, its powers Q^2 .. Q^(L-1) by Cauchy
//                  products, and the L x L matrix read off them.  Three or four series sit in LDS; a thread owns one output coefficient and
//                  sums its products for j ascending over the reference's [lower, upper], so the matrix is the reference's bit for bit.
//   k_apt_lhood    workgroup per trial point, over the Gaussians of the node's class set: _calcBias (numerator and denominator in fp64, one
//                  partial per slice of Gaussians, the slices added in order), then the sum of _calcMixLhood (each Gaussian's value as the
//                  reference computes it, added over a fixed tree) divided by the counts.  No floating-point atomics.
//   k_apt_apply    thread per (speaker, Gaussian, component): float(sum_m A[n][m] double(mu[m])), m ascending, then the float bias.
// The line search (apt.cpp) runs on the host, one per (speaker, node); every round launches the first two kernels once for all the
// searches that are still running, each at its own trial point.  This translation unit is compiled with -ffp-contract=off.
#include "launch.h"
#include "adapt.h"
#include "apt.h"
#include "train.h"
#include <algorithm>
#include <cmath>
#include <cstring>
#include <set>

namespace dsr {

static constexpr int kLast = kAptSeriesLen - 1;           // LaurentSeries::last()
static constexpr int kSeries = 2 * kAptSeriesLen - 1;     // coefficients of a series
static constexpr int kMatrixThreads = 320;                // >= kSeries: one thread per coefficient
static constexpr int kLhoodThreads = 256;

// CauchyProduct (tr:85-101) for output coefficient i: every lane walks j = -last .. last so that s1[j] is one LDS address per step
__device__ __forceinline__ double apt_cauchy(const double* s1, const double* s2, int i)
{
  const int lower = max(-kLast, i - kLast), upper = min(kLast, i + kLast);
  double sum = 0.0;
  for (int j = -kLast; j <= kLast; j++)
    if (j >= lower && j <= upper) sum = __dadd_rn(sum, __dmul_rn(s1[j], s2[i - j]));
  return sum;
}

// conf [trial][kAptMaxParams], nPar [trial]; A [trial][L][L]
__global__ __launch_bounds__(kMatrixThreads) void k_apt_matrix(int rapt, int L, const double* __restrict__ conf, const int* __restrict__ nPar,
                                                               const double* __restrict__ ecoef, double* __restrict__ A)
{
  __shared__ double buf[4][kSeries];
  const int t = blockIdx.x, tid = threadIdx.x, i = tid - kLast;
  const bool on = tid < kSeries;
  double* Q = buf[0] + kLast; double* prev = buf[1] + kLast; double* cur = buf[2] + kLast; double* F = buf[3] + kLast;
  const double* p = conf + (long) t * kAptMaxParams;
  if (rapt) {                                             // BLTTransformer::bilinear (tr:1404-1414)
    if (on) Q[i] = 0.0;
    __syncthreads();
    if (tid == 0) {
      const double mu = p[0];
      Q[0] = -mu; Q[1] = __dsub_rn(1.0, __dmul_rn(mu, mu));
      for (int k = 2; k < kAptSeriesLen; k++) Q[k] = __dmul_rn(mu, Q[k - 1]);
    }
    __syncthreads();
  } else {                                                // SLAPTTransformer::_calcSequence (tr:1716-1741)
    if (on) { F[i] = 0.0; Q[i] = 0.0; }
    __syncthreads();
    if (tid == 0) {
      const int nP = nPar[t];
      for (int k = 1; k <= nP; k++) { F[k] = __dmul_rn(M_PI_2, p[k - 1]); F[-k] = __dmul_rn(-M_PI_2, p[k - 1]); }
    }
    __syncthreads();
    if (on) {                                             // multAdd (tr:69-76) of columns 0 (the unit sample) and 1
      Q[i] = __dadd_rn(Q[i], __dmul_rn(ecoef[0], i == 0 ? 1.0 : 0.0));
      Q[i] = __dadd_rn(Q[i], __dmul_rn(ecoef[1], F[i]));
      prev[i] = F[i];
    }
    __syncthreads();
    for (int c = 2; c < kAptColumns; c++) {
      if (on) { const double v = apt_cauchy(F, prev, i); cur[i] = v; Q[i] = __dadd_rn(Q[i], __dmul_rn(ecoef[c], v)); }
      __syncthreads();
      double* sw = prev; prev = cur; cur = sw;
    }
    double moved = 0.0;                                   // shift (tr:78-83): element -last stays as it was
    if (on && i > -kLast) moved = Q[i - 1];
    __syncthreads();
    if (on && i > -kLast) Q[i] = moved;
    __syncthreads();
  }
  // _calcTransMatrix (tr:1212-1242): column 0 is the unit sample sequence, column m comes from Q^m
  double* out = A + (long) t * L * L;
  if (tid < L) out[(long) tid * L] = tid == 0 ? 1.0 : 0.0;
  const double* pw = Q;
  for (int m = 1; m < L; m++) {
    if (m >= 2) {
      const double* last = m == 2 ? Q : prev;
      if (on) cur[i] = apt_cauchy(Q, last, i);
      __syncthreads();
      double* sw = prev; prev = cur; cur = sw; pw = prev;
    }
    if (tid < L) {
      double el = __dadd_rn(pw[tid], pw[-tid]);
      if (tid == 0) el = el / 2.0;
      out[(long) tid * L + m] = el;
    }
  }
}

// trial [2 t] = { speaker, node }; gidx [nodeStart[node] .. nodeStart[node + 1]) the node's Gaussians in model order; A [trial][L][L];
// lhood [trial], bias [trial][bSize]
__global__ __launch_bounds__(kLhoodThreads) void k_apt_lhood(int L, int D, int G, int bSize, const int* __restrict__ trial, const int* __restrict__ gidx,
                                                             const int* __restrict__ nodeStart, const float* __restrict__ mean,
                                                             const float* __restrict__ ivar, const double* __restrict__ cnt,
                                                             const double* __restrict__ sumO, const double* __restrict__ A, double* __restrict__ lhood,
                                                             float* __restrict__ bias)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* sA = reinterpret_cast<double*>(smem);           // [L][L]
  double* red = sA + L * L;                               // [2][kLhoodThreads]
  float* sBias = reinterpret_cast<float*>(red + 2 * kLhoodThreads);      // [D]
  const int t = blockIdx.x, tid = threadIdx.x, s = trial[2 * t], node = trial[2 * t + 1];
  const int g0 = nodeStart[node], nG = nodeStart[node + 1] - g0;
  for (int e = tid; e < L * L; e += kLhoodThreads) sA[e] = A[(long) t * L * L + e];
  __syncthreads();
  const double* cs = cnt + (long) s * G;
  if (bSize > 0) {                                        // _calcBias (eA:1574-1601): thread (component n, slice p of the Gaussians)
    const int P = kLhoodThreads / bSize, n = tid % bSize, p = tid / bSize;
    double num = 0.0, den = 0.0;
    if (p < P) {
      const int isub = n / L; const double* a = sA + (n - isub * L) * L;
      for (int j = p; j < nG; j += P) {
        const int g = gidx[g0 + j]; const float ck = (float) cs[g];
        if (ck == 0.0f) continue;
        const float* mu = mean + (long) g * D + isub * L;
        double tr = 0.0;
        for (int m = 0; m < L; m++) tr = __dadd_rn(tr, __dmul_rn(a[m], (double) mu[m]));
        const float iv = ivar[(long) g * D + n];
        num = __dadd_rn(num, __dmul_rn(__dsub_rn(sumO[((long) s * G + g) * D + n], (double) __fmul_rn(ck, (float) tr)), (double) iv));
        den = __dadd_rn(den, (double) __fmul_rn(ck, iv));
      }
      red[tid] = num; red[kLhoodThreads + tid] = den;
    }
    __syncthreads();
    if (tid < bSize) {
      num = 0.0; den = 0.0;
      for (int q = 0; q < P; q++) { num = __dadd_rn(num, red[q * bSize + tid]); den = __dadd_rn(den, red[kLhoodThreads + q * bSize + tid]); }
      const float b = __fdiv_rn((float) num, (float) den);
      sBias[tid] = b; bias[(long) t * bSize + tid] = b;
    }
    __syncthreads();
  }
  double sum = 0.0, nCounts = 0.0;                        // _calcMixLhood (eA:1603-1620): a thread per Gaussian
  for (int j = tid; j < nG; j += kLhoodThreads) {
    const int g = gidx[g0 + j]; const float ck = (float) cs[g];
    if (ck == 0.0f) continue;
    const float* mu = mean + (long) g * D; const float* iv = ivar + (long) g * D; const double* so = sumO + ((long) s * G + g) * D;
    const double half = __dmul_rn(0.5, (double) ck);
    double mix = 0.0;
    for (int k = 0; k < D; k++) {
      const int isub = k / L; const double* a = sA + (k - isub * L) * L; const float* x = mu + isub * L;
      double tr = 0.0;
      for (int m = 0; m < L; m++) tr = __dadd_rn(tr, __dmul_rn(a[m], (double) x[m]));
      float trn = (float) tr;
      if (k < bSize) trn = __fadd_rn(trn, sBias[k]);
      mix = __dadd_rn(mix, __dmul_rn(__dmul_rn(__dsub_rn(so[k], __dmul_rn(half, (double) trn)), (double) trn), (double) iv[k]));
    }
    sum = __dadd_rn(sum, mix); nCounts = __dadd_rn(nCounts, (double) ck);
  }
  red[tid] = sum; red[kLhoodThreads + tid] = nCounts;
  __syncthreads();
  for (int w = kLhoodThreads / 2; w > 0; w >>= 1) {
    if (tid < w) { red[tid] = __dadd_rn(red[tid], red[tid + w]); red[kLhoodThreads + tid] = __dadd_rn(red[kLhoodThreads + tid], red[kLhoodThreads + tid + w]); }
    __syncthreads();
  }
  if (tid == 0) lhood[t] = red[0] / red[kLhoodThreads];
}

// map [sp][g]: the table of Gaussian g; tabA [.][L][L], tabBias [.][D], tabBsz [.] (the entries of the bias that are added)
__global__ __launch_bounds__(256) void k_apt_apply(int L, int D, int G, const float* __restrict__ mean, const int* __restrict__ map,
                                                   const double* __restrict__ tabA, const float* __restrict__ tabBias, const int* __restrict__ tabBsz,
                                                   float* __restrict__ out)
{
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long) G * D) return;
  const int sp = blockIdx.y, g = (int) (idx / D), k = (int) (idx - (long) g * D), isub = k / L, n = k - isub * L;
  const int tab = map[(long) sp * G + g];
  const double* a = tabA + ((long) tab * L + n) * L;
  const float* mu = mean + (long) g * D + isub * L;
  double tr = 0.0;
  for (int m = 0; m < L; m++) tr = __dadd_rn(tr, __dmul_rn(a[m], (double) mu[m]));
  float v = (float) tr;
  if (k < tabBsz[tab]) v = __fadd_rn(v, tabBias[(long) tab * D + k]);
  out[((long) sp * G + g) * D + k] = v;
}

namespace {

void check_slot(const AptHandle& h, int s) { if (s < 0 || s >= h.S) throw Error(DSR_E_INDEX, "speaker %d of %d", s, h.S); }

int node_index(const AptHandle& h, unsigned node)
{
  std::vector<unsigned>::const_iterator it = std::lower_bound(h.nodes.begin(), h.nodes.end(), node);
  if (it == h.nodes.end() || *it != node) throw Error(DSR_E_KEY, "Could not find node %d.", node);
  return (int) (it - h.nodes.begin());
}

// BaseTree::node(idx, useAncestor = true) over the classes of a slot's parameters (tr:2030-2049)
unsigned tree_node(const AptParams& t, unsigned rc)
{
  if (rc == 0) throw Error(DSR_E_INDEX, "Regression class index must be >= 1");
  unsigned idx = rc;
  if (t.hasIndex(idx)) return idx;
  while (idx > 1) { idx /= 2; if (t.hasIndex(idx)) return idx; }
  throw Error(DSR_E_KEY, "Could not find node %d.", idx);
}

// what RAPTParam::transformer / SLAPTParam::transformer (tr:461-471, 521-527) can be made from here
void check_transformer(const AptHandle& h, int type, const AptParam& p)
{
  if (type == kAptRAPT) {
    if (p.conf.size() != 1) throw Error(DSR_E_PARAMETER, "%d RAPT parameters: only the bilinear transform (one parameter) is implemented", (int) p.conf.size());
    if (!(fabs(p.conf[0]) < 1.0)) throw Error(DSR_E_PARAMETER, "Mu value (%g) is not < 1.0", p.conf[0]);
  } else if (p.conf.empty() || p.conf.size() > (size_t) kAptMaxParams)
    throw Error(DSR_E_PARAMETER, "%d SLAPT parameters: 1 .. %d are implemented", (int) p.conf.size(), kAptMaxParams);
  const int b = (int) p.bias.size();
  if (b != 0 && b != h.L && b != h.D) throw Error(DSR_E_CONSISTENCY, "Bias size %d is incompatible with feature length %d.", b, h.L);
}

// k_apt_matrix for n parameter vectors: conf [n][kAptMaxParams], nPar [n] -> h.d_A [n][L][L]
void run_matrix(AptHandle& h, int rapt, const std::vector<double>& conf, const std::vector<int>& nPar, hipStream_t st)
{
  const int n = (int) nPar.size();
  h.d_conf.upload(conf, st); h.d_nPar.upload(nPar, st); h.d_A.reserve((size_t) n * h.L * h.L);
  ScopedTimer tm(h.timing, st);
  launch(k_apt_matrix, dim3(n), dim3(kMatrixThreads), 0, st, rapt, h.L, h.d_conf.p, h.d_nPar.p, h.d_ecoef.p, h.d_A.p);
  h.ms[0] += tm.stop();
}

struct SearchState { int s, nodeIdx, state; double point; AptTrace tr; };

void apt_estimate(AptHandle& h, double threshold, hipStream_t st)
{
  const int D = h.D, G = h.G, S = h.S, L = h.L, bSize = h.bSize;
  if (h.paramN != 1) throw Error(DSR_E_PARAMETER, "estimation of %d all-pass parameters: only the one-parameter line search is implemented", h.paramN);
  // EstimatorTree: the classes of the Gaussians are the leaves, their ancestors the internal nodes
  if (h.regClass.empty()) throw Error(DSR_E_INDEX, "Regression class index must be >= 1");
  std::set<unsigned> leafSet, nodeSet;
  for (int g = 0; g < G; g++) { if (h.regClass[g] == 0) throw Error(DSR_E_INDEX, "Regression class index must be >= 1"); leafSet.insert(h.regClass[g]); }
  for (std::set<unsigned>::iterator it = leafSet.begin(); it != leafSet.end(); ++it) for (unsigned a = *it; a > 0; a /= 2) nodeSet.insert(a);
  std::vector<unsigned> leaves(leafSet.begin(), leafSet.end()), nodes(nodeSet.begin(), nodeSet.end());
  const int NL = (int) leaves.size(), NN = (int) nodes.size();
  std::vector<int> gidx, nodeStart(NN + 1, 0);            // GaussListTrain (eA:68-76): model order
  for (int k = 0; k < NN; k++) {
    for (int g = 0; g < G; g++) if (isAncestor(nodes[k], h.regClass[g])) gidx.push_back(g);
    nodeStart[k + 1] = (int) gidx.size();
  }
  // what estimate finds stored (eA:1671-1673, 1900-1913), checked for every slot before anything changes
  std::vector<AptParams> fresh(S);
  for (int s = 0; s < S; s++) {
    fresh[s].map = h.store[s].map; fresh[s].type = h.store[s].type;
    for (int l = 0; l < NL; l++) {
      const AptParam& p = fresh[s].findAPT(leaves[l], h.kind, true);
      if (h.kind == kAptRAPT && p.conf.size() > 1) throw Error(DSR_E_CONSISTENCY, " No. of all-pass parameters (%d) is incorrect.", (int) p.conf.size());
      if (h.kind == kAptSLAPT && !p.bias.empty() && (int) p.bias.size() != bSize)
        throw Error(DSR_E_DIMENSION, "Feature lengths (%d vs. %d) do not match.", (int) p.bias.size(), bSize);
    }
  }
  // EstimatorAdapt::ttlFrames (eA:1565-1572): a double sum in model order, on the host
  std::vector<double> c((size_t) S * G);
  DSR_HIP(hipStreamSynchronize(st));
  DSR_HIP(hipMemcpy(c.data(), h.d_c.p, c.size() * sizeof(double), hipMemcpyDeviceToHost));
  std::vector<double> ttl((size_t) S * NN, 0.0);
  for (int s = 0; s < S; s++) for (int k = 0; k < NN; k++) {
    double t = 0.0; for (int j = nodeStart[k]; j < nodeStart[k + 1]; j++) t += c[(size_t) s * G + gidx[j]];
    ttl[(size_t) s * NN + k] = t;
  }
  h.leaves.swap(leaves); h.nodes.swap(nodes); h.ttl.swap(ttl);
  // LeafIterator::estimate (eA:3105-3133) for a tree that is not MLLR: no copying; the back-off node is estimated for the leaf's class
  h.plan.clear(); h.trace.clear(); h.rounds = 0; h.ms[0] = h.ms[1] = 0.f;
  std::vector<SearchState> search; std::map<std::pair<int, int>, int> searchOf; std::vector<int> stepSearch;
  const double thr = (double) (float) threshold;          // EstimateThreshold is a float
  for (int s = 0; s < S; s++) for (int l = 0; l < NL; l++) {
    const unsigned leaf = h.leaves[l]; unsigned rc;
    for (rc = leaf; rc > 0; rc /= 2) if (h.ttl[(size_t) s * NN + node_index(h, rc)] > thr) break;
    if (rc == 0) rc = 1;
    const int k = node_index(h, rc);
    std::map<std::pair<int, int>, int>::iterator it = searchOf.find(std::make_pair(s, k));
    if (it == searchOf.end()) {                           // the search does not start from what is stored: one per (slot, node)
      it = searchOf.insert(std::make_pair(std::make_pair(s, k), (int) search.size())).first;
      SearchState ss; ss.s = s; ss.nodeIdx = k; ss.point = 0.0;
      ss.state = apt_line_search(h.kind, ss.tr.lhood, &ss.point, nullptr);
      search.push_back(ss);
    }
    h.plan.push_back(AptStep{s, (int) rc, (int) leaf}); stepSearch.push_back(it->second);
  }
  h.d_gidx.upload(gidx, st); h.d_nodeStart.upload(nodeStart, st);
  const size_t lds = ((size_t) L * L + 2 * kLhoodThreads) * sizeof(double) + (size_t) D * sizeof(float);
  std::vector<int> active, trial, nPar; std::vector<double> conf, lh; std::vector<float> bias;
  for (;;) {
    active.clear();
    for (size_t i = 0; i < search.size(); i++) if (search[i].state == kSearchNeeds) active.push_back((int) i);
    if (active.empty()) break;
    const int nA = (int) active.size();
    conf.assign((size_t) nA * kAptMaxParams, 0.0); nPar.assign(nA, 1); trial.resize((size_t) 2 * nA);
    for (int a = 0; a < nA; a++) {
      const SearchState& ss = search[active[a]];
      conf[(size_t) a * kAptMaxParams] = ss.point; trial[2 * a] = ss.s; trial[2 * a + 1] = ss.nodeIdx;
    }
    run_matrix(h, h.kind == kAptRAPT, conf, nPar, st);
    h.d_trial.upload(trial, st); h.d_lhood.reserve(nA); h.d_bias.reserve((size_t) nA * std::max(bSize, 1));
    {
      ScopedTimer tm(h.timing, st);
      launch(k_apt_lhood, dim3(nA), dim3(kLhoodThreads), lds, st, L, D, G, bSize, h.d_trial.p, h.d_gidx.p, h.d_nodeStart.p, h.d_mean.p, h.d_ivar.p,
                          h.d_c.p, h.d_sumO.p, h.d_A.p, h.d_lhood.p, h.d_bias.p);
      h.ms[1] += tm.stop();
    }
    lh.resize(nA); bias.resize((size_t) nA * bSize);
    DSR_HIP(hipMemcpyAsync(lh.data(), h.d_lhood.p, nA * sizeof(double), hipMemcpyDeviceToHost, st));
    if (bSize) DSR_HIP(hipMemcpyAsync(bias.data(), h.d_bias.p, bias.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    DSR_HIP(hipStreamSynchronize(st));
    for (int a = 0; a < nA; a++) {
      SearchState& ss = search[active[a]];
      ss.tr.point.push_back(ss.point); ss.tr.lhood.push_back(lh[a]);
      ss.tr.bias.insert(ss.tr.bias.end(), bias.begin() + (size_t) a * bSize, bias.begin() + (size_t) (a + 1) * bSize);
      ss.state = apt_line_search(h.kind, ss.tr.lhood, &ss.point, nullptr);
    }
    h.rounds++;
  }
  h.status.assign(S, 0);
  for (size_t i = 0; i < search.size(); i++) {
    if (search[i].state != kSearchDone) h.status[search[i].s] = DSR_E_CONSISTENCY;
    h.trace[std::make_pair(search[i].s, h.nodes[search[i].nodeIdx])] = search[i].tr;
  }
  for (size_t i = 0; i < h.plan.size(); i++) {
    const AptStep& p = h.plan[i]; if (h.status[p.speaker]) continue;
    const SearchState& ss = search[stepSearch[i]]; const AptTrace& tr = ss.tr;
    // the bias is _calcBias under the matrix the estimator holds last: BLT recomputes it at alpha (eA:1667-1668) -- a point the search
    // evaluated, and the kernel gives the same bits for the same point --, SLAPT keeps the series of the last trial point (eA:1926)
    size_t e = tr.point.size() - 1;
    if (h.kind == kAptRAPT) while (e > 0 && memcmp(&tr.point[e], &ss.point, sizeof(double)) != 0) e--;
    AptParam& par = fresh[p.speaker].findAPT((unsigned) p.leaf, h.kind, true);
    par.conf.assign(1, ss.point); par.bias.assign(tr.bias.begin() + e * bSize, tr.bias.begin() + (e + 1) * bSize);
  }
  int bad = -1, nBad = 0;
  for (int s = 0; s < S; s++) { if (h.status[s]) { if (bad < 0) bad = s; nBad++; continue; } h.store[s].map.swap(fresh[s].map); h.store[s].type = fresh[s].type; }
  if (nBad) throw Error(DSR_E_CONSISTENCY, "the line search of %d speaker(s), the first %d, met a likelihood that is not a number or did not converge", nBad, bad);
}

// the tables and per-Gaussian indices of speakers [s0, s1): one table per class of a speaker's parameters that a Gaussian uses
void run_apply(AptHandle& h, int s0, int s1, float* out, hipStream_t st)
{
  const int D = h.D, G = h.G;
  std::vector<int> map((size_t) (s1 - s0) * G, 0), nPar, bsz; std::vector<double> conf; std::vector<float> tabBias; int rapt = -1;
  for (int s = s0; s < s1; s++) {
    const AptParams& t = h.store[s]; std::map<unsigned, int> at;
    for (int g = 0; g < G; g++) {
      const unsigned node = tree_node(t, h.regClass.empty() ? 0u : h.regClass[g]);
      std::map<unsigned, int>::iterator it = at.find(node);
      if (it == at.end()) {
        const AptParam& p = t.map.find(node)->second;
        check_transformer(h, t.type, p);
        if (rapt >= 0 && rapt != (t.type == kAptRAPT)) throw Error(DSR_E_CONSISTENCY, "speaker %d holds parameters of another adaptation type", s);
        rapt = t.type == kAptRAPT;
        it = at.insert(std::make_pair(node, (int) nPar.size())).first;
        nPar.push_back((int) p.conf.size()); bsz.push_back((int) p.bias.size());
        conf.resize(conf.size() + kAptMaxParams, 0.0); std::copy(p.conf.begin(), p.conf.end(), conf.end() - kAptMaxParams);
        tabBias.resize(tabBias.size() + D, 0.0f); std::copy(p.bias.begin(), p.bias.end(), tabBias.end() - D);
      }
      map[(size_t) (s - s0) * G + g] = it->second;
    }
  }
  const float keep = h.ms[0];
  run_matrix(h, rapt == 1, conf, nPar, st);
  h.ms[0] = keep;                                         // ms[0] is the estimate's
  h.d_map.upload(map, st); h.d_tabBias.upload(tabBias, st); h.d_tabBsz.upload(bsz, st);
  h.ms[2] = 0.f; ScopedTimer tm(h.timing, st);
  launch(k_apt_apply, dim3(cdiv((long) G * D, 256), s1 - s0), dim3(256), 0, st, h.L, D, G, h.d_mean.p, h.d_map.p, h.d_A.p, h.d_tabBias.p, h.d_tabBsz.p, out);
  h.ms[2] += tm.stop();
}

// the means, inverse variances and classes the handle works on ([G][subFeatLen nSubFeat]), zeroed statistics, eCoefficients (tr:1640-1650)
void init_handle(AptHandle& h, int S, int kind, int L, int nSub, int biasType, const std::vector<float>& mean, const std::vector<float>& ivar,
                 const std::vector<uint16_t>& regClass)
{
  h.S = S; h.D = L * nSub; h.G = (int) (mean.size() / h.D); h.kind = kind; h.L = L; h.nSub = nSub; h.biasType = biasType;
  h.bSize = biasType == kAptBiasNone ? 0 : biasType == kAptBiasCepstra ? L : h.D;                      // eA:1553-1563
  h.origMean = mean; h.ivar = ivar; h.regClass = regClass;
  h.store.resize(S); h.status.assign(S, 0);
  h.d_mean.upload(h.origMean); h.d_ivar.upload(h.ivar);
  std::vector<double> e(kAptColumns); e[0] = e[1] = 1.0;
  for (int i = 2; i < kAptColumns; i++) e[i] = e[i - 1] / i;
  h.d_ecoef.upload(e);
  h.d_c.reserve((size_t) S * h.G); h.d_sumO.reserve((size_t) S * h.G * h.D);
  DSR_HIP(hipMemset(h.d_c.p, 0, (size_t) S * h.G * sizeof(double))); DSR_HIP(hipMemset(h.d_sumO.p, 0, (size_t) S * h.G * h.D * sizeof(double)));
}

void check_shape(int kind, int subFeatLen, int nSubFeat)
{
  if (kind != kAptRAPT && kind != kAptSLAPT) throw Error(DSR_E_PARAMETER, "adaptation type %d: 1 (RAPT: the bilinear transform) or 2 (SLAPT)", kind);
  if (nSubFeat < 1 || nSubFeat > 3) throw Error(DSR_E_PARAMETER, "%d sub-features: NaturalIndex holds 1 .. 3", nSubFeat);
  if (subFeatLen < 1 || subFeatLen > kAptMaxSub) throw Error(DSR_E_DIMENSION, "subFeatLen = %d: the all-pass transforms are built for 1 .. %d", subFeatLen, kAptMaxSub);
}

void check_target(const AptHandle& h, const dsr_gmm* g)
{
  if (!g) throw Error(DSR_E_PARAMETER, "null argument");
  if (g->G != h.G || g->D != h.D) throw Error(DSR_E_DIMENSION, "model of %d Gaussians x %d for transforms of %d x %d", g->G, g->D, h.G, h.D);
}

}  // namespace
}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_apt_create(const dsr_gmm* g, int S, int kind, int subFeatLen, int nSubFeat, int biasType, dsr_apt** out)
{
  return guard([&] {
    if (!g || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (S < 1 || S > 65535) throw Error(DSR_E_PARAMETER, "%d speaker slots", S);
    check_shape(kind, subFeatLen, nSubFeat);
    if (biasType < kAptBiasNone || biasType > kAptBiasAll) throw Error(DSR_E_TYPE, "Unrecognized bias type %d", biasType);
    if (subFeatLen * nSubFeat != g->D) throw Error(DSR_E_DIMENSION, "%d sub-features of %d for a model of dimN = %d (extended means are not implemented)", nSubFeat, subFeatLen, g->D);
    require_device();
    dsr_apt* h = new dsr_apt();
    try { init_handle(*h, S, kind, subFeatLen, nSubFeat, biasType, g->mean, g->ivar, g->regClass); } catch (...) { delete h; throw; }
    *out = h;
  });
}
void dsr_apt_destroy(dsr_apt* h) { delete h; }
int dsr_apt_num_speakers(const dsr_apt* h) { return h ? h->S : 0; }

dsr_status dsr_apt_set_param_n(dsr_apt* h, int paramN)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    if (paramN != 1) throw Error(DSR_E_PARAMETER, "estimation of %d all-pass parameters: only the one-parameter line search is implemented", paramN);
    h->paramN = paramN;
  });
}

dsr_status dsr_apt_set_stats(dsr_apt* h, int s, dsr_train* t)
{
  return guard([&] {
    if (!h || !t) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    take_stats(*t, h->G, h->D, h->d_c.p + (size_t) s * h->G, h->d_sumO.p + (size_t) s * h->G * h->D);
  });
}

dsr_status dsr_apt_set_stats_arrays(dsr_apt* h, int s, const double* c, const double* sumO)
{
  return guard([&] {
    if (!h || !c || !sumO) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(h->d_c.p + (size_t) s * h->G, c, (size_t) h->G * sizeof(double), hipMemcpyHostToDevice));
    DSR_HIP(hipMemcpy(h->d_sumO.p + (size_t) s * h->G * h->D, sumO, (size_t) h->G * h->D * sizeof(double), hipMemcpyHostToDevice));
  });
}

dsr_apt_params* dsr_apt_store(dsr_apt* h, int s) { return (h && s >= 0 && s < h->S) ? &h->store[s] : nullptr; }

dsr_status dsr_apt_set_params(dsr_apt* h, int s, unsigned rc, int nConf, const double* conf, int nBias, const float* bias)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    const dsr_status st = dsr_apt_params_set(&h->store[s], rc, h->kind, nConf, conf, nBias, bias); if (st) throw Error(st, "%s", dsr_last_error());
  });
}

dsr_status dsr_apt_get_params(const dsr_apt* h, int s, unsigned rc, int* nConf, double* conf, int* nBias, float* bias)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    std::map<unsigned, AptParam>::const_iterator it = h->store[s].map.find(rc);
    if (it == h->store[s].map.end()) throw Error(DSR_E_INDEX, "Could not find parameters for regression class %d.", rc);
    if (nConf) *nConf = (int) it->second.conf.size();
    if (nBias) *nBias = (int) it->second.bias.size();
    if (conf) std::copy(it->second.conf.begin(), it->second.conf.end(), conf);
    if (bias) std::copy(it->second.bias.begin(), it->second.bias.end(), bias);
  });
}

dsr_status dsr_apt_estimate(dsr_apt* h, double threshold, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); apt_estimate(*h, threshold, (hipStream_t) stream); }); }

int dsr_apt_speaker_status(const dsr_apt* h, int s) { return (h && s >= 0 && s < h->S) ? h->status[s] : DSR_E_INDEX; }
int dsr_apt_rounds(const dsr_apt* h) { return h ? h->rounds : 0; }

dsr_status dsr_apt_get_plan(const dsr_apt* h, int* n, int32_t* steps)
{
  return guard([&] {
    if (!h || !n) throw Error(DSR_E_PARAMETER, "null argument");
    *n = (int) h->plan.size();
    if (steps) for (size_t i = 0; i < h->plan.size(); i++) { steps[3 * i] = h->plan[i].speaker; steps[3 * i + 1] = h->plan[i].node; steps[3 * i + 2] = h->plan[i].leaf; }
  });
}

dsr_status dsr_apt_get_nodes(const dsr_apt* h, int* n, uint32_t* nodes, int32_t* isLeaf)
{
  return guard([&] {
    if (!h || !n) throw Error(DSR_E_PARAMETER, "null argument");
    *n = (int) h->nodes.size();
    for (size_t k = 0; k < h->nodes.size(); k++) {
      if (nodes) nodes[k] = h->nodes[k];
      if (isLeaf) isLeaf[k] = std::binary_search(h->leaves.begin(), h->leaves.end(), h->nodes[k]) ? 1 : 0;
    }
  });
}

dsr_status dsr_apt_ttl_frames(const dsr_apt* h, int s, unsigned node, double* ttl)
{
  return guard([&] {
    if (!h || !ttl) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    *ttl = h->ttl[(size_t) s * h->nodes.size() + node_index(*h, node)];
  });
}

dsr_status dsr_apt_get_trace(const dsr_apt* h, int s, unsigned node, int* n, double* points, double* lhood, float* bias)
{
  return guard([&] {
    if (!h || !n) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    std::map<std::pair<int, unsigned>, AptTrace>::const_iterator it = h->trace.find(std::make_pair(s, node));
    if (it == h->trace.end()) throw Error(DSR_E_KEY, "Could not find node %d.", node);
    const AptTrace& t = it->second;
    *n = (int) t.point.size();
    if (points) std::copy(t.point.begin(), t.point.end(), points);
    if (lhood) std::copy(t.lhood.begin(), t.lhood.end(), lhood);
    if (bias) std::copy(t.bias.begin(), t.bias.end(), bias);
  });
}

dsr_status dsr_apt_get_matrix(dsr_apt* h, int s, unsigned rc, double* A)
{
  return guard([&] {
    if (!h || !A) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    const AptParams& t = h->store[s];
    const AptParam& p = t.map.find(tree_node(t, rc))->second;
    check_transformer(*h, t.type, p);
    std::vector<double> conf(kAptMaxParams, 0.0); std::copy(p.conf.begin(), p.conf.end(), conf.begin());
    const float keep = h->ms[0];
    run_matrix(*h, t.type == kAptRAPT, conf, std::vector<int>(1, (int) p.conf.size()), nullptr);
    h->ms[0] = keep;
    DSR_HIP(hipMemcpy(A, h->d_A.p, (size_t) h->L * h->L * sizeof(double), hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_apt_transform_rows(int kind, int subFeatLen, int nSubFeat, int nConf, const double* conf, int nBias, const float* bias,
                                  const float* rows, int N, double* A, float* out)
{
  return guard([&] {
    if (nConf < 0 || nBias < 0 || N < 0 || (nConf && !conf) || (nBias && !bias) || (N && (!rows || !out))) throw Error(DSR_E_PARAMETER, "null argument");
    check_shape(kind, subFeatLen, nSubFeat);
    require_device();
    const int D = subFeatLen * nSubFeat, G = std::max(N, 1);
    std::vector<float> mean((size_t) G * D, 0.0f); if (N) std::copy(rows, rows + (size_t) N * D, mean.begin());
    dsr_apt h; init_handle(h, 1, kind, subFeatLen, nSubFeat, kAptBiasNone, mean, std::vector<float>(), std::vector<uint16_t>((size_t) G, 1));
    AptParam& p = h.store[0].findAPT(1, kind, true);
    p.conf.assign(conf, conf + nConf); p.bias.assign(bias, bias + nBias);
    h.d_out.reserve((size_t) G * D);
    run_apply(h, 0, 1, h.d_out.p, nullptr);               // checks the parameters, makes the matrix, transforms the rows
    DSR_HIP(hipDeviceSynchronize());
    if (A) DSR_HIP(hipMemcpy(A, h.d_A.p, (size_t) subFeatLen * subFeatLen * sizeof(double), hipMemcpyDeviceToHost));
    if (N) DSR_HIP(hipMemcpy(out, h.d_out.p, (size_t) N * D * sizeof(float), hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_apt_write(dsr_apt* h, int s, const char* fileName)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); check_slot(*h, s); h->store[s].write(fileName); }); }
dsr_status dsr_apt_read(dsr_apt* h, int s, const char* fileName)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); check_slot(*h, s); h->store[s].read(fileName); }); }

dsr_status dsr_apt_adapt(dsr_apt* h, int s, dsr_gmm* target)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s); check_target(*h, target);
    h->d_out.reserve((size_t) h->G * h->D);
    run_apply(*h, s, s + 1, h->d_out.p, nullptr);
    std::vector<float> mu((size_t) h->G * h->D);
    DSR_HIP(hipMemcpy(mu.data(), h->d_out.p, mu.size() * sizeof(float), hipMemcpyDeviceToHost));
    target->mean.swap(mu); gmm_finish(*target);           // every scoring mode follows, as after dsr_mllr_adapt
  });
}

dsr_status dsr_apt_adapt_all(dsr_apt* h, float* means_dev, void* stream)
{
  return guard([&] {
    if (!h || !means_dev) throw Error(DSR_E_PARAMETER, "null argument");
    run_apply(*h, 0, h->S, means_dev, (hipStream_t) stream);
  });
}

dsr_status dsr_apt_reset_mean(dsr_apt* h, dsr_gmm* target)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_target(*h, target);
    target->mean = h->origMean; gmm_finish(*target);       // CodebookAdapt::resetMean
  });
}

dsr_status dsr_apt_set_timing(dsr_apt* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->timing = on != 0; }); }
dsr_status dsr_apt_kernel_ms(const dsr_apt* h, float ms[3])
{ return guard([&] { if (!h || !ms) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 3; i++) ms[i] = h->ms[i]; }); }

}  // extern "C"
