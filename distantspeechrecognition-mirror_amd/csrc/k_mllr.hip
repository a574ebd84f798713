// csrc/k_mllr.hip -- MLLR mean transforms for a batch of speakers: statistics, solves and the transformed means on the device.
//
// Replaces GaussListTrain (asr/train/estimateAdapt.cc:68-76, "eA"), EstimatorAdapt::ttlFrames (eA:1565-1572), MLLREstimatorAdapt::_calcZ /
// _calcGi / estimate (eA:2101-2195), EstimatorTreeMLLR (eA:3143-3165), estimateAdaptationParameters and LeafIterator::estimate (eA:3064-3133),
// MLLRTransformer::transform (asr/adapt/transform.cc:1770-1785, "tr") and TransformerTree::transform (tr:2149-2163), which work on one speaker
// and one Gaussian at a time, for S speakers at once.
//
//   k_mllr_take    count - denCount and sumO of a trainer's accumulator rows into a speaker slot (postProb(), codebookTrain.h:142-144)
//   k_mllr_stats   per (speaker, chunk of kChunk Gaussians of one leaf class): with xi = (mu, 1), rows i = feature, the contraction over the
//                  Gaussians g of   G_i[p][q] += (c_g iv_gi) xi_p xi_q  (p <= q, one column per pair)   and   z_i[n] += (sumO_gi iv_gi) xi_n
//                  on v_mfma_f64_16x16x4_f64.  Both operands are formed in registers; xi xi^T is never stored.  A Gaussian whose count
//                  rounds to float 0 is left out of both (eA:2110, 2138).  The z columns start at a multiple of 16, so a 16-column tile is of one kind.
//   k_mllr_reduce  per (speaker, node): every leaf below the node is the sum of its chunks in chunk order, the node the sum of its leaves in
//                  ascending class order; ttlFrames the same way.  No floating-point atomics: the same call twice gives the same bits.
//   k_mllr_solve   workgroup per (solve, row): G_i unpacked into LDS, cyclic Jacobi (mllr_jacobi.h) to G_i = V diag(lambda) V^T, then
//                  w_i = V diag(1 / lambda_k if |lambda_k| / max |lambda| >= 1e-7 else 0) V^T z_i -- for a symmetric matrix what
//                  gsl_linalg_SV_decomp and MaxSingularValueRatio give (eA:2156-2180).  Not converged or not finite: the solve's flag.
//   k_mllr_apply   thread per (speaker, Gaussian, row): float comp = bias; comp = float(double(comp) + A[m][n] double(mu[n])), n ascending.
// The back-off over the tree is a few integers per speaker and runs on the host between k_mllr_reduce and k_mllr_solve.
// This translation unit is compiled with -ffp-contract=off.
#include "launch.h"
#include "adapt.h"
#include "train.h"
#include "mfma64.h"
#include "mllr_jacobi.h"
#include <algorithm>
#include <cmath>
#include <set>

namespace dsr {

static constexpr int kChunk = 64;                         // Gaussians per workgroup of k_mllr_stats: 16 k-steps, their A operands stay in registers
static constexpr int kMaxD = 80;                          // two (D + 1)^2 fp64 matrices of k_mllr_solve fit the LDS
static constexpr int kSolveThreads = 128;

// sumOsq: NULL, or where the squared sums go (take_stats_sq)
__global__ __launch_bounds__(256) void k_mllr_take(const double* __restrict__ acc, int G, int D, double* __restrict__ c, double* __restrict__ sumO,
                                                   double* __restrict__ sumOsq)
{
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long) G * (D + 1)) return;
  const int g = (int) (idx / (D + 1)), d = (int) (idx - (long) g * (D + 1));
  const double* row = acc + (long) g * (2 * D + 4);
  if (d < D) { sumO[(long) g * D + d] = row[d]; if (sumOsq) sumOsq[(long) g * D + d] = row[D + d]; } else c[g] = __dsub_rn(row[2 * D], row[2 * D + 1]);
}

// chunk[3 k] = { leaf, first sorted Gaussian, Gaussians }; pq[col] = p | q << 16 of a G column, n of a z column, -1 of padding
__global__ __launch_bounds__(256) void k_mllr_stats(int D, int G, int NCp, int PZ, const float* __restrict__ mean, const float* __restrict__ ivar,
                                                    const double* __restrict__ cnt, const double* __restrict__ sumO, const int* __restrict__ gidx,
                                                    const int* __restrict__ chunk, const int* __restrict__ pq, double* __restrict__ part,
                                                    double* __restrict__ partTtl)
{
  __shared__ float xi[kChunk * (kMaxD + 1)]; __shared__ double wc[kChunk]; __shared__ int sg[kChunk]; __shared__ int live[kChunk];
  const int ch = blockIdx.x, s = blockIdx.y, nCh = gridDim.x, N1 = D + 1;
  const int i0 = chunk[3 * ch + 1], n = chunk[3 * ch + 2];
  for (int j = threadIdx.x; j < kChunk; j += blockDim.x) {
    int g = 0; double cv = 0.0;
    if (j < n) { g = gidx[i0 + j]; cv = cnt[(long) s * G + g]; }
    sg[j] = g; wc[j] = cv; live[j] = j < n && (float) cv != 0.0f;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n * N1; e += blockDim.x) { const int j = e / N1, d = e - j * N1; xi[e] = d < D ? mean[(long) sg[j] * D + d] : 1.0f; }
  if (threadIdx.x == 0) { double t = 0.0; for (int j = 0; j < n; j++) t = __dadd_rn(t, wc[j]); partTtl[(long) s * nCh + ch] = t; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  const int RT = (D + 15) >> 4, CT = NCp >> 4;
  double* out = part + ((long) s * nCh + ch) * D * NCp;
  for (int rt = 0; rt < RT; rt++) {
    const int row = rt * 16 + lo;                         // A: feature `row` of Gaussian 4 ks + hi
    double aG[kChunk / 4], aZ[kChunk / 4];
#pragma unroll
    for (int ks = 0; ks < kChunk / 4; ks++) {
      const int j = 4 * ks + hi; aG[ks] = 0.0; aZ[ks] = 0.0;
      if (row < D && live[j]) {
        const double iv = (double) ivar[(long) sg[j] * D + row];
        aG[ks] = __dmul_rn(wc[j], iv); aZ[ks] = __dmul_rn(sumO[((long) s * G + sg[j]) * D + row], iv);
      }
    }
    for (int ct = wave; ct < CT; ct += 4) {               // uniform per wave
      const int col = ct * 16 + lo, code = pq[col];
      const bool isZ = ct * 16 >= PZ;
      const int p = code < 0 ? 0 : (code & 0xffff), q = (code < 0 || isZ) ? 0 : (code >> 16);
      d4 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < kChunk / 4; ks++) {
        const int j = 4 * ks + hi;
        double b = 0.0;
        if (j < n && code >= 0) { b = (double) xi[j * N1 + p]; if (!isZ) b = __dmul_rn(b, (double) xi[j * N1 + q]); }      // exact: 24 + 24 bits
        c = mfma64(isZ ? aZ[ks] : aG[ks], b, c);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int orow = rt * 16 + hi + 4 * r;
        if (orow < D) out[(long) orow * NCp + col] = c[r];
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_mllr_reduce(int D, int NCp, int nCh, const int* __restrict__ leafChunk, const int* __restrict__ nodeLeafStart,
                                                     const int* __restrict__ nodeLeaf, const double* __restrict__ part, const double* __restrict__ partTtl,
                                                     double* __restrict__ stats, double* __restrict__ ttl)
{
  const int node = blockIdx.x, s = blockIdx.y, NN = gridDim.x;
  const long sz = (long) D * NCp;
  const int l0 = nodeLeafStart[node], l1 = nodeLeafStart[node + 1];
  for (long e = threadIdx.x; e < sz; e += blockDim.x) {
    double acc = 0.0;
    for (int li = l0; li < l1; li++) {
      const int leaf = nodeLeaf[li]; double t = 0.0;
      for (int ch = leafChunk[leaf]; ch < leafChunk[leaf + 1]; ch++) t = __dadd_rn(t, part[((long) s * nCh + ch) * sz + e]);
      acc = __dadd_rn(acc, t);
    }
    stats[((long) s * NN + node) * sz + e] = acc;
  }
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int li = l0; li < l1; li++) {
      const int leaf = nodeLeaf[li]; double t = 0.0;
      for (int ch = leafChunk[leaf]; ch < leafChunk[leaf + 1]; ch++) t = __dadd_rn(t, partTtl[(long) s * nCh + ch]);
      acc = __dadd_rn(acc, t);
    }
    ttl[(long) s * NN + node] = acc;
  }
}

// solve[2 k] = { speaker, node }; one workgroup per (k, row i): W[k][i][0 .. D]
__global__ __launch_bounds__(kSolveThreads) void k_mllr_solve(int D, int NN, int NCp, int PZ, const int* __restrict__ solve, const double* __restrict__ stats,
                                                              double* __restrict__ W, int* __restrict__ flag)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = D + 1, m = (n + 1) & ~1, nt = blockDim.x, tid = threadIdx.x;
  double* a = reinterpret_cast<double*>(smem);            // [n][n]
  double* v = a + n * n;                                  // [n][n]
  double* z = v + n * n;                                  // [n]
  double* t = z + n;                                      // [n]
  double* cs = t + n;                                     // [m]
  double* sq = cs + m;                                    // [2 nt]
  const int k = blockIdx.x / D, i = blockIdx.x - k * D;
  const double* src = stats + (((long) solve[2 * k] * NN + solve[2 * k + 1]) * D + i) * NCp;
  for (int e = tid; e < n * n; e += nt) {
    const int r = e / n, c = e - r * n, p = r < c ? r : c, q = r < c ? c : r;
    a[e] = src[p * n - (p * (p - 1)) / 2 + (q - p)];      // upper triangle, row by row; the lower one is its copy (eA:2123-2128)
    v[e] = r == c ? 1.0 : 0.0;
  }
  for (int e = tid; e < n; e += nt) z[e] = src[PZ + e];
  __syncthreads();
  bool ok = false;
  for (int sweep = 0; sweep <= kJacobiSweeps; sweep++) {
    mj_norms(a, n, sq, tid, nt);
    __syncthreads();
    double off, all; mj_norms_done(sq, nt, off, all);     // every thread sums the same numbers in the same order
    __syncthreads();
    if (!(all <= 1.7E308)) break;                         // NaN or infinite
    if (mj_converged(off, all, n)) { ok = true; break; }
    if (sweep == kJacobiSweeps) break;
    for (int r = 0; r < m - 1; r++) {
      mj_angles(a, n, m, r, cs, tid, nt);
      __syncthreads();
      mj_rows(a, n, m, r, cs, tid, nt);
      __syncthreads();
      mj_cols(a, v, n, m, r, cs, tid, nt);
      __syncthreads();
    }
  }
  for (int e = tid; e < n; e += nt) if (!(fabs(z[e]) <= 1.7E308)) ok = false;
  ok = __syncthreads_and(ok);
  if (!ok) { if (tid == 0) flag[k] = 1; for (int e = tid; e < n; e += nt) W[((long) k * D + i) * n + e] = 0.0; return; }
  double lmax = 0.0;
  for (int e = 0; e < n; e++) { const double l = fabs(a[e * n + e]); if (l > lmax) lmax = l; }
  for (int e = tid; e < n; e += nt) {
    double sum = 0.0;
    for (int j = 0; j < n; j++) sum = __dadd_rn(sum, __dmul_rn(v[j * n + e], z[j]));
    const double l = a[e * n + e];
    t[e] = (fabs(l) / lmax >= 1.0e-07) ? sum / l : 0.0;   // MaxSingularValueRatio, eA:2156, 2172-2179
  }
  __syncthreads();
  for (int e = tid; e < n; e += nt) {
    double sum = 0.0;
    for (int j = 0; j < n; j++) sum = __dadd_rn(sum, __dmul_rn(v[e * n + j], t[j]));
    W[((long) k * D + i) * n + e] = sum;
  }
}

// map[sp][g]: the transform of Gaussian g among Wtab[.][D][D + 1]
__global__ __launch_bounds__(256) void k_mllr_apply(int D, int G, const float* __restrict__ mean, const int* __restrict__ map, const double* __restrict__ Wtab,
                                                    float* __restrict__ out)
{
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long) G * D) return;
  const int sp = blockIdx.y, g = (int) (idx / D), m = (int) (idx - (long) g * D);
  const double* w = Wtab + ((long) map[(long) sp * G + g] * D + m) * (D + 1);
  const float* mu = mean + (long) g * D;
  float comp = (float) w[D];
  for (int n = 0; n < D; n++) comp = (float) __dadd_rn((double) comp, __dmul_rn(w[n], (double) mu[n]));
  out[((long) sp * G + g) * D + m] = comp;
}

void take_stats_sq(const dsr_train& t, int G, int D, double* c, double* sumO, double* sumOsq)
{
  if (t.G != G || t.D != D) throw Error(DSR_E_DIMENSION, "accumulators of %d Gaussians x %d for a model of %d x %d", t.G, t.D, G, D);
  launch(k_mllr_take, dim3(cdiv((long) G * (D + 1), 256)), dim3(256), 0, nullptr, t.d_acc.p, G, D, c, sumO, sumOsq);
  DSR_HIP(hipDeviceSynchronize());
}
void take_stats(const dsr_train& t, int G, int D, double* c, double* sumO) { take_stats_sq(t, G, D, c, sumO, nullptr); }

namespace {

void check_slot(const MllrHandle& h, int s) { if (s < 0 || s >= h.S) throw Error(DSR_E_INDEX, "speaker %d of %d", s, h.S); }

int node_index(const MllrHandle& h, unsigned node)
{
  std::vector<unsigned>::const_iterator it = std::lower_bound(h.nodes.begin(), h.nodes.end(), node);
  if (it == h.nodes.end() || *it != node) throw Error(DSR_E_KEY, "Could not find node %d.", node);
  return (int) (it - h.nodes.begin());
}

// BaseTree::node(idx, useAncestor = true) over the classes of a parameter tree (tr:2030-2049)
unsigned tree_node(const ParamTree& t, unsigned rc)
{
  if (rc == 0) throw Error(DSR_E_INDEX, "Regression class index must be >= 1");
  unsigned idx = rc;
  if (t.hasIndex(idx)) return idx;
  while (idx > 1) { idx /= 2; if (t.hasIndex(idx)) return idx; }
  throw Error(DSR_E_KEY, "Could not find node %d.", idx);
}

// the transform tables and per-Gaussian indices of speakers [s0, s1): one table per class of a speaker's tree
void build_tables(MllrHandle& h, int s0, int s1, std::vector<double>& tab, std::vector<int>& map)
{
  const int D = h.D; tab.clear(); map.assign((size_t) (s1 - s0) * h.G, 0);
  for (int s = s0; s < s1; s++) {
    const ParamTree& t = h.tree[s]; std::map<unsigned, int> at;
    for (int g = 0; g < h.G; g++) {
      const unsigned node = tree_node(t, h.regClass.empty() ? 0u : h.regClass[g]);
      std::map<unsigned, int>::iterator it = at.find(node);
      if (it == at.end()) {
        const MLLRParam& p = t.map.find(node)->second;
        if (p.size != D) throw Error(DSR_E_DIMENSION, "Sizes (%d vs. %d) do not match.", p.size, D);
        if ((int) p.bias.size() != D) throw Error(DSR_E_DIMENSION, "Feature lengths (%d vs. %d) do not match.", (int) p.bias.size(), D);
        it = at.insert(std::make_pair(node, (int) (tab.size() / ((size_t) D * (D + 1))))).first;
        for (int m = 0; m < D; m++) { for (int n = 0; n < D; n++) tab.push_back(p.matrix[(size_t) m * D + n]); tab.push_back(p.bias[m]); }
      }
      map[(size_t) (s - s0) * h.G + g] = it->second;
    }
  }
}

void mllr_estimate(MllrHandle& h, double threshold, hipStream_t st)
{
  const int D = h.D, G = h.G, S = h.S, N1 = D + 1;
  // EstimatorTreeMLLR (eA:3143-3165): the classes of the Gaussians are the leaves, their ancestors the internal nodes
  if (h.regClass.empty()) throw Error(DSR_E_INDEX, "Regression class index must be >= 1");
  std::set<unsigned> leafSet, nodeSet;
  for (int g = 0; g < G; g++) { if (h.regClass[g] == 0) throw Error(DSR_E_INDEX, "Regression class index must be >= 1"); leafSet.insert(h.regClass[g]); }
  for (std::set<unsigned>::iterator it = leafSet.begin(); it != leafSet.end(); ++it) for (unsigned a = *it; a > 0; a /= 2) nodeSet.insert(a);
  h.leaves.assign(leafSet.begin(), leafSet.end()); h.nodes.assign(nodeSet.begin(), nodeSet.end());
  const int NL = (int) h.leaves.size(), NN = (int) h.nodes.size();
  // Gaussians sorted by class (stable), cut into chunks that do not cross a class
  std::vector<int> leafOf(G), leafStart(NL + 1, 0), gidx(G);
  for (int g = 0; g < G; g++) { leafOf[g] = (int) (std::lower_bound(h.leaves.begin(), h.leaves.end(), (unsigned) h.regClass[g]) - h.leaves.begin()); leafStart[leafOf[g] + 1]++; }
  for (int l = 0; l < NL; l++) leafStart[l + 1] += leafStart[l];
  { std::vector<int> pos(leafStart.begin(), leafStart.end() - 1); for (int g = 0; g < G; g++) gidx[pos[leafOf[g]]++] = g; }
  std::vector<int> chunk, leafChunk(NL + 1, 0);
  for (int l = 0; l < NL; l++) {
    for (int i0 = leafStart[l]; i0 < leafStart[l + 1]; i0 += kChunk) { chunk.push_back(l); chunk.push_back(i0); chunk.push_back(std::min(kChunk, leafStart[l + 1] - i0)); }
    leafChunk[l + 1] = (int) (chunk.size() / 3);
  }
  const int nCh = leafChunk[NL];
  std::vector<int> nodeLeafStart(NN + 1, 0), nodeLeaf;
  for (int k = 0; k < NN; k++) {                          // GaussListTrain: the Gaussians with isAncestor(node, regClass), eA:68-76
    for (int l = 0; l < NL; l++) if (isAncestor(h.nodes[k], h.leaves[l])) nodeLeaf.push_back(l);
    nodeLeafStart[k + 1] = (int) nodeLeaf.size();
  }
  const int P = N1 * (N1 + 1) / 2; h.PZ = (P + 15) & ~15; h.NCp = (h.PZ + N1 + 15) & ~15;
  std::vector<int> pq(h.NCp, -1);
  { int col = 0; for (int p = 0; p < N1; p++) for (int q = p; q < N1; q++) pq[col++] = p | (q << 16); for (int n = 0; n < N1; n++) pq[h.PZ + n] = n; }
  if (S > 65535 || (long) S * NN * D > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "%d speakers x %d nodes in one call", S, NN);
  h.d_gidx.upload(gidx, st); h.d_chunk.upload(chunk, st); h.d_pq.upload(pq, st); h.d_leafChunk.upload(leafChunk, st);
  h.d_nodeLeafStart.upload(nodeLeafStart, st); h.d_nodeLeaf.upload(nodeLeaf, st);
  const size_t sz = (size_t) D * h.NCp;
  h.d_part.reserve((size_t) S * nCh * sz); h.d_partTtl.reserve((size_t) S * nCh); h.d_stats.reserve((size_t) S * NN * sz); h.d_ttl.reserve((size_t) S * NN);
  {
    ScopedTimer tm(h.timing, st);
    launch(k_mllr_stats, dim3(nCh, S), dim3(256), 0, st, D, G, h.NCp, h.PZ, h.d_mean.p, h.d_ivar.p, h.d_c.p, h.d_sumO.p, h.d_gidx.p, h.d_chunk.p,
                       h.d_pq.p, h.d_part.p, h.d_partTtl.p);
    launch(k_mllr_reduce, dim3(NN, S), dim3(256), 0, st, D, h.NCp, nCh, h.d_leafChunk.p, h.d_nodeLeafStart.p, h.d_nodeLeaf.p, h.d_part.p,
                       h.d_partTtl.p, h.d_stats.p, h.d_ttl.p);
    h.ms[0] = tm.stop();
  }
  h.ttl.assign((size_t) S * NN, 0.0);
  DSR_HIP(hipMemcpyAsync(h.ttl.data(), h.d_ttl.p, h.ttl.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  // LeafIterator::estimate (eA:3105-3133) for every speaker; estimateAdaptationParameters starts from a cleared tree (eA:3066-3067)
  h.plan.clear(); std::vector<int> solve; std::vector<int> solveOf;     // solveOf[step]: its solve, -1 for a copy
  const double thr = (double) (float) threshold;          // EstimateThreshold is a float
  for (int s = 0; s < S; s++) {
    std::set<unsigned> present;
    for (int l = 0; l < NL; l++) {
      const unsigned leaf = h.leaves[l]; unsigned rc;
      for (rc = leaf; rc > 0; rc /= 2) if (h.ttl[(size_t) s * NN + node_index(h, rc)] > thr) break;
      if (rc == 0) rc = 1;
      if (leaf != rc && present.count(rc)) { h.plan.push_back(MllrStep{s, (int) rc, (int) leaf, 1}); solveOf.push_back(-1); present.insert(leaf); continue; }
      h.plan.push_back(MllrStep{s, (int) rc, (int) leaf, 0}); solveOf.push_back((int) (solve.size() / 2));
      solve.push_back(s); solve.push_back(node_index(h, rc)); present.insert(leaf); present.insert(rc);
    }
  }
  const int nSolve = (int) (solve.size() / 2);
  std::vector<double> W((size_t) nSolve * D * N1); std::vector<int> flag(nSolve, 0);
  if (nSolve) {
    const int m = (N1 + 1) & ~1;
    const size_t lds = ((size_t) 2 * N1 * N1 + 2 * N1 + m + 2 * kSolveThreads) * sizeof(double);
    h.d_solve.upload(solve, st); h.d_W.reserve(W.size()); h.d_flag.reserve(nSolve);
    DSR_HIP(hipMemsetAsync(h.d_flag.p, 0, nSolve * sizeof(int), st));
    ScopedTimer tm(h.timing, st);
    launch(k_mllr_solve, dim3(nSolve * D), dim3(kSolveThreads), lds, st, D, NN, h.NCp, h.PZ, h.d_solve.p, h.d_stats.p, h.d_W.p, h.d_flag.p);
    h.ms[1] = tm.stop();
    DSR_HIP(hipMemcpyAsync(W.data(), h.d_W.p, W.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    DSR_HIP(hipMemcpyAsync(flag.data(), h.d_flag.p, nSolve * sizeof(int), hipMemcpyDeviceToHost, st));
    DSR_HIP(hipStreamSynchronize(st));
  }
  h.status.assign(S, 0);
  for (size_t i = 0; i < h.plan.size(); i++) if (solveOf[i] >= 0 && flag[solveOf[i]]) h.status[h.plan[i].speaker] = DSR_E_CONSISTENCY;
  std::vector<ParamTree> fresh(S);
  for (size_t i = 0; i < h.plan.size(); i++) {
    const MllrStep& p = h.plan[i]; if (h.status[p.speaker]) continue;
    ParamTree& t = fresh[p.speaker];
    if (p.copy) { t.find((unsigned) p.leaf, true); continue; }
    const double* w = W.data() + (size_t) solveOf[i] * D * N1;
    t.findMLLR((unsigned) p.leaf, true).assign(D, w); t.findMLLR((unsigned) p.node, true).assign(D, w);      // eA:2188-2192
  }
  int bad = -1, nBad = 0;
  for (int s = 0; s < S; s++) { if (h.status[s]) { if (bad < 0) bad = s; nBad++; continue; } h.tree[s].map.swap(fresh[s].map); h.tree[s].type = fresh[s].type; }
  if (nBad) throw Error(DSR_E_CONSISTENCY, "MLLR statistics of %d speaker(s), the first %d, are not finite or their eigen-decomposition did not converge", nBad, bad);
}

void run_apply(MllrHandle& h, int s0, int s1, float* out, hipStream_t st)
{
  std::vector<double> tab; std::vector<int> map; build_tables(h, s0, s1, tab, map);
  h.d_Wtab.upload(tab, st); h.d_map.upload(map, st);
  ScopedTimer tm(h.timing, st);
  launch(k_mllr_apply, dim3(cdiv((long) h.G * h.D, 256), s1 - s0), dim3(256), 0, st, h.D, h.G, h.d_mean.p, h.d_map.p, h.d_Wtab.p, out);
  h.ms[2] = tm.stop();
}

void check_target(const MllrHandle& h, const dsr_gmm* g)
{
  if (!g) throw Error(DSR_E_PARAMETER, "null argument");
  if (g->G != h.G || g->D != h.D) throw Error(DSR_E_DIMENSION, "model of %d Gaussians x %d for transforms of %d x %d", g->G, g->D, h.G, h.D);
}

}  // namespace
}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_mllr_create(const dsr_gmm* g, int S, dsr_mllr** out)
{
  return guard([&] {
    if (!g || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (S < 1) throw Error(DSR_E_PARAMETER, "%d speaker slots", S);
    if (g->D > kMaxD) throw Error(DSR_E_DIMENSION, "dimN = %d: MLLR is built for dimN <= %d", g->D, kMaxD);
    require_device();
    dsr_mllr* h = new dsr_mllr();
    try {
      h->S = S; h->D = g->D; h->G = g->G; h->origMean = g->mean; h->ivar = g->ivar; h->regClass = g->regClass;
      h->tree.resize(S); h->status.assign(S, 0);
      h->d_mean.upload(h->origMean); h->d_ivar.upload(h->ivar);
      h->d_c.reserve((size_t) S * h->G); h->d_sumO.reserve((size_t) S * h->G * h->D);
      DSR_HIP(hipMemset(h->d_c.p, 0, (size_t) S * h->G * sizeof(double))); DSR_HIP(hipMemset(h->d_sumO.p, 0, (size_t) S * h->G * h->D * sizeof(double)));
    } catch (...) { delete h; throw; }
    *out = h;
  });
}
void dsr_mllr_destroy(dsr_mllr* h) { delete h; }
int dsr_mllr_num_speakers(const dsr_mllr* h) { return h ? h->S : 0; }

dsr_status dsr_mllr_set_stats(dsr_mllr* h, int s, dsr_train* t)
{
  return guard([&] {
    if (!h || !t) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    take_stats(*t, h->G, h->D, h->d_c.p + (size_t) s * h->G, h->d_sumO.p + (size_t) s * h->G * h->D);
  });
}

dsr_status dsr_mllr_set_stats_arrays(dsr_mllr* h, int s, const double* c, const double* sumO)
{
  return guard([&] {
    if (!h || !c || !sumO) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(h->d_c.p + (size_t) s * h->G, c, (size_t) h->G * sizeof(double), hipMemcpyHostToDevice));
    DSR_HIP(hipMemcpy(h->d_sumO.p + (size_t) s * h->G * h->D, sumO, (size_t) h->G * h->D * sizeof(double), hipMemcpyHostToDevice));
  });
}

dsr_status dsr_mllr_estimate(dsr_mllr* h, double threshold, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); mllr_estimate(*h, threshold, (hipStream_t) stream); }); }

int dsr_mllr_speaker_status(const dsr_mllr* h, int s) { return (h && s >= 0 && s < h->S) ? h->status[s] : DSR_E_INDEX; }

dsr_status dsr_mllr_get_plan(const dsr_mllr* h, int* n, int32_t* steps)
{
  return guard([&] {
    if (!h || !n) throw Error(DSR_E_PARAMETER, "null argument");
    *n = (int) h->plan.size();
    if (steps) for (size_t i = 0; i < h->plan.size(); i++) { steps[4 * i] = h->plan[i].speaker; steps[4 * i + 1] = h->plan[i].node; steps[4 * i + 2] = h->plan[i].leaf; steps[4 * i + 3] = h->plan[i].copy; }
  });
}

dsr_status dsr_mllr_get_nodes(const dsr_mllr* h, int* n, uint32_t* nodes, int32_t* isLeaf)
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

dsr_status dsr_mllr_get_stats(dsr_mllr* h, int s, unsigned node, int row, double* Gi, double* z)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    if (h->nodes.empty()) throw Error(DSR_E_CONSISTENCY, "no statistics: call dsr_mllr_estimate first");
    if (row < 0 || row >= h->D) throw Error(DSR_E_INDEX, "row %d of %d", row, h->D);
    const int k = node_index(*h, node), n = h->D + 1, NN = (int) h->nodes.size();
    std::vector<double> r(h->NCp);
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(r.data(), h->d_stats.p + (((size_t) s * NN + k) * h->D + row) * h->NCp, r.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (Gi) { int col = 0; for (int p = 0; p < n; p++) for (int q = p; q < n; q++, col++) Gi[p * n + q] = Gi[q * n + p] = r[col]; }
    if (z) for (int e = 0; e < n; e++) z[e] = r[h->PZ + e];
  });
}

dsr_status dsr_mllr_ttl_frames(const dsr_mllr* h, int s, unsigned node, double* ttl)
{
  return guard([&] {
    if (!h || !ttl) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    *ttl = h->ttl[(size_t) s * h->nodes.size() + node_index(*h, node)];
  });
}

dsr_param_tree* dsr_mllr_tree(dsr_mllr* h, int s) { return (h && s >= 0 && s < h->S) ? &h->tree[s] : nullptr; }

dsr_status dsr_mllr_get_transform(dsr_mllr* h, int s, unsigned rc, double* W)
{
  return guard([&] {
    if (!h || !W) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    const dsr_status st = dsr_param_tree_get(&h->tree[s], rc, W); if (st) throw Error(st, "%s", dsr_last_error());
  });
}
dsr_status dsr_mllr_write(dsr_mllr* h, int s, const char* fileName)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); check_slot(*h, s); h->tree[s].write(fileName); }); }
dsr_status dsr_mllr_read(dsr_mllr* h, int s, const char* fileName)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); check_slot(*h, s); h->tree[s].read(fileName); }); }

dsr_status dsr_mllr_adapt(dsr_mllr* h, int s, dsr_gmm* target)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s); check_target(*h, target);
    h->d_out.reserve((size_t) h->G * h->D);
    run_apply(*h, s, s + 1, h->d_out.p, nullptr);
    std::vector<float> mu((size_t) h->G * h->D);
    DSR_HIP(hipMemcpy(mu.data(), h->d_out.p, mu.size() * sizeof(float), hipMemcpyDeviceToHost));
    target->mean.swap(mu); gmm_finish(*target);           // every scoring mode follows, as after dsr_train_update
  });
}

dsr_status dsr_mllr_adapt_all(dsr_mllr* h, float* means_dev, void* stream)
{
  return guard([&] {
    if (!h || !means_dev) throw Error(DSR_E_PARAMETER, "null argument");
    run_apply(*h, 0, h->S, means_dev, (hipStream_t) stream);
  });
}

dsr_status dsr_mllr_reset_mean(dsr_mllr* h, dsr_gmm* target)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_target(*h, target);
    target->mean = h->origMean; gmm_finish(*target);       // CodebookAdapt::resetMean
  });
}

dsr_status dsr_mllr_set_timing(dsr_mllr* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->timing = on != 0; }); }
dsr_status dsr_mllr_kernel_ms(const dsr_mllr* h, float ms[3])
{ return guard([&] { if (!h || !ms) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 3; i++) ms[i] = h->ms[i]; }); }

}  // extern "C"
