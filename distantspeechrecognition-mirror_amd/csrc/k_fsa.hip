// csrc/k_fsa.hip -- feature-space adaptation (constrained MLLR): statistics, estimation and the transform on the device.
//
// Replaces FeatureSpaceAdaptationFeature::_accuOne (asr/train/fsa.cc:187-245, "fsa"), accumulate / accumulateLattice (fsa:282-321),
// _calcCofactor / estimate (fsa:332-433) and next (fsa:247-280), which work on one frame, one accumulator and one transform at a time, for
// batches of items, several (accumulator, transform) pairs and whole utterances.
//
//   k_fsa_nearest  thread per item: the nearest Gaussian of the item's codebook under the scoring frame -- the one-hot addCount of
//                  CodebookBasic::_scoreOpt (codebookBasic.cc:431-554) -- with the arithmetic of scoring mode 0 (gmm_dist.h, shared with k_gmm.hip).
//   k_fsa_stats    items sorted by accumulator, then codebook (stable, on the host); one workgroup per chunk of kChunk items of one accumulator:
//                  with g the item's Gaussian and xi = (1, x) of the UNTRANSFORMED frame, rows i = feature, the contraction over the items of
//                      G_i[j][k] += (gamma iv_gi) xi_j xi_k  (j >= k, one column per pair)   and   z_i[n] += (gamma float(mu_gi iv_gi)) xi_n
//                  on v_mfma_f64_16x16x4_f64.  Both operands are exact in fp64 and formed in registers; xi xi^T is never stored.  The z columns
//                  start at a multiple of 16, so a 16-column tile is of one kind (the layout of k_mllr_stats with items for Gaussians).
//   k_fsa_reduce   workgroup per accumulator: the sum of its chunks in chunk order.  No floating-point atomics: the same call twice gives the
//                  same bits.  The host adds the sums to its accumulators (csrc/fsa.h).
//   k_fsa_eig      workgroup per (pair, row i): G_i^+ under the 1e-7 rule by Jacobi rotations in LDS (fsa_rows.h, mllr_jacobi.h).
//   k_fsa_rows     workgroup per pair: W, A^-1 and det in LDS, the iterN x dimN row updates (fsa_rows.h).  A pair whose statistics are not finite,
//                  whose decomposition did not converge or whose A leaves the condition bound is flagged and keeps its transform.
//   k_fsa_apply    thread per (frame, output dimension): float(shift w[d][0] + sum_i w[d][i + 1] x_i), a double sum with i ascending; for
//                  shift == -1 float(w[d][0] + x_d).
// The pair indexing and tile walk of k_fsa_stats restate k_mllr_stats': k_mllr.hip is left as it is, so its object code does not change.
// This translation unit is compiled with -ffp-contract=off.
#include "launch.h"
#include "fsa.h"
#include "lattice.h"
#include "mfma64.h"
#include "gmm_dist.h"
#include "fsa_rows.h"
#include <algorithm>
#include <cmath>

namespace dsr {

static constexpr int kChunk = 64;                         // items per workgroup of k_fsa_stats: 16 k-steps, their A operands stay in registers
static constexpr int kEigThreads = 128, kRowThreads = 256;

__global__ __launch_bounds__(256) void k_fsa_nearest(const float* __restrict__ x, int D, int DP, const int* __restrict__ off, const float* __restrict__ mean,
                                                     const float* __restrict__ ivar, const float* __restrict__ cst, const int* __restrict__ sFrame,
                                                     const int* __restrict__ sDist, long M, int* __restrict__ gsel)
{
  const long i = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const float* xp = x + (long) sFrame[i] * D;
  const int k = sDist[i], a = off[k], b = off[k + 1];
  float minDist = 1E20f; int minIdx = 0;
  for (int g = a; g < b; g++) {
    const float dist = gmm_dist_exact(cst[g], mean + (long) g * DP, ivar + (long) g * DP, xp, D);
    if (dist < minDist) { minDist = dist; minIdx = g - a; }
  }
  gsel[i] = a + minIdx;
}

// chunk[3 c] = { accumulator slot, first sorted item, items }; pq[col] = j | k << 16 of a G column, n of a z column, -1 of padding
__global__ __launch_bounds__(256) void k_fsa_stats(int D, int NCp, int PZ, const float* __restrict__ x, const float* __restrict__ mean,
                                                   const float* __restrict__ ivar, const int* __restrict__ sFrame, const float* __restrict__ sGamma,
                                                   const int* __restrict__ gsel, const int* __restrict__ chunk, const int* __restrict__ pq,
                                                   double* __restrict__ part)
{
  __shared__ float xi[kChunk * (kFsaMaxD + 1)]; __shared__ float gam[kChunk]; __shared__ int sg[kChunk]; __shared__ int sf[kChunk];
  const int ch = blockIdx.x, N1 = D + 1;
  const int i0 = chunk[3 * ch + 1], n = chunk[3 * ch + 2];
  for (int j = threadIdx.x; j < kChunk; j += blockDim.x) {
    const bool in = j < n;
    sg[j] = in ? gsel[i0 + j] : 0; gam[j] = in ? sGamma[i0 + j] : 0.0f; sf[j] = in ? sFrame[i0 + j] : 0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n * N1; e += blockDim.x) { const int j = e / N1, d = e - j * N1; xi[e] = d == 0 ? 1.0f : x[(long) sf[j] * D + d - 1]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  const int RT = (D + 15) >> 4, CT = NCp >> 4;
  double* out = part + (long) ch * D * NCp;
  for (int rt = 0; rt < RT; rt++) {
    const int row = rt * 16 + lo;                         // A: feature `row` of item 4 ks + hi
    double aG[kChunk / 4], aZ[kChunk / 4];
#pragma unroll
    for (int ks = 0; ks < kChunk / 4; ks++) {
      const int j = 4 * ks + hi; aG[ks] = 0.0; aZ[ks] = 0.0;
      if (row < D && j < n) {
        const float iv = ivar[(long) sg[j] * D + row], mu = mean[(long) sg[j] * D + row];
        aG[ks] = __dmul_rn((double) gam[j], (double) iv);                    // fsa:231-233
        aZ[ks] = __dmul_rn((double) gam[j], (double) __fmul_rn(mu, iv));     // fsa:221-223: the product of two floats is a float
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

__global__ __launch_bounds__(256) void k_fsa_reduce(long sz, const int* __restrict__ accChunk, const double* __restrict__ part, double* __restrict__ stats)
{
  const int slot = blockIdx.y, c0 = accChunk[slot], c1 = accChunk[slot + 1];
  const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= sz) return;
  double t = 0.0;
  for (int ch = c0; ch < c1; ch++) t = __dadd_rn(t, part[(long) ch * sz + e]);
  stats[(long) slot * sz + e] = t;
}

// one workgroup per (pair k, row i): Gsym [k][i][n][n] -> Ginv [k][i][n][n]
__global__ __launch_bounds__(kEigThreads) void k_fsa_eig(int D, const double* __restrict__ Gsym, double* __restrict__ Ginv, int* __restrict__ flag)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = D + 1, m = (n + 1) & ~1, nt = blockDim.x, tid = threadIdx.x;
  double* a = reinterpret_cast<double*>(smem);            // [n][n]
  double* v = a + n * n;                                  // [n][n]
  double* t = v + n * n;                                  // [n]
  double* cs = t + n;                                     // [m]
  double* sq = cs + m;                                    // [2 nt]
  const int k = blockIdx.x / D;
  const double* src = Gsym + (long) blockIdx.x * n * n;
  for (int e = tid; e < n * n; e += nt) a[e] = src[e];
  __syncthreads();
  const bool ok = fsa_eig_run(a, v, t, cs, sq, n, Ginv + (long) blockIdx.x * n * n, tid, nt, [] { __syncthreads(); });
  if (!ok && tid == 0) flag[k] = 1;
}

// one workgroup per pair: Wio [k][D][n] in and, unless the pair is flagged, out
__global__ __launch_bounds__(kRowThreads) void k_fsa_rows(int D, int iterN, const double* __restrict__ Ginv, const double* __restrict__ z,
                                                          const double* __restrict__ beta, double* __restrict__ Wio, int* __restrict__ flag)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = D + 1, nt = blockDim.x, tid = threadIdx.x, k = blockIdx.x;
  if (flag[k]) return;                                    // set by k_fsa_eig, a launch earlier: uniform
  FsaWork w; w.carve(reinterpret_cast<double*>(smem), D, nt);
  double* Wk = Wio + (long) k * D * n;
  for (int e = tid; e < D * n; e += nt) w.W[e] = Wk[e];
  __syncthreads();
  const bool ok = fsa_rows_run(w, D, iterN, Ginv + (long) k * D * n * n, z + (long) k * D * n, beta[k], tid, nt, [] { __syncthreads(); });
  if (!ok) { if (tid == 0) flag[k] = 1; return; }
  for (int e = tid; e < D * n; e += nt) Wk[e] = w.W[e];
}

// tranOfRow == nullptr: transform 0.  An index outside [0, nTran) gives NaN (the indices are device data the host does not see).
__global__ __launch_bounds__(256) void k_fsa_apply(int D, long N, int nTran, const float* __restrict__ x, const int* __restrict__ tranOfRow,
                                                   const double* __restrict__ Wall, float shift, float* __restrict__ out)
{
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * D) return;
  const long r = idx / D; const int d = (int) (idx - r * D);
  const int t = tranOfRow ? tranOfRow[r] : 0;
  if (t < 0 || t >= nTran) { out[idx] = __int_as_float(0x7fc00000); return; }
  const double* w = Wall + ((long) t * D + d) * (D + 1);
  const float* xp = x + r * D;
  if (shift == -1.0f) { out[idx] = (float) __dadd_rn(w[0], (double) xp[d]); return; }         // fsa:261-265
  double sum = __dmul_rn((double) shift, w[0]);                                              // fsa:270-274
  for (int i = 0; i < D; i++) sum = __dadd_rn(sum, __dmul_rn(w[i + 1], (double) xp[i]));
  out[idx] = (float) sum;
}

namespace {

struct Item { int accu, dist, frame; float gamma; long idx; };

// M items of _accuOne (fsa:187-245).  accepted [nAccu] or nullptr: the items each accumulator took in this call; nearest [M] or nullptr: the
// Gaussian (inside its codebook) each item chose, -1 for an item of a distribution that is not switched on.
void fsa_accumulate(FsaHandle& h, const float* xScore, const float* xSrc, long N, const int* frame, const int* dist, const float* gamma, const int* accu,
                    long M, int64_t* accepted, int32_t* nearest, hipStream_t st)
{
  const int D = h.D, N1 = D + 1;
  if (M < 0 || N < 0) throw Error(DSR_E_PARAMETER, "negative size");
  if (accepted) for (int a = 0; a < h.nAccu; a++) accepted[a] = 0;
  if (M == 0) return;
  if (nearest) for (long i = 0; i < M; i++) nearest[i] = -1;
  if (!xScore || !xSrc || !frame || !dist || !gamma || !accu) throw Error(DSR_E_PARAMETER, "null argument");
  if (M > 0x7fffffffL - kChunk) throw Error(DSR_E_DIMENSION, "%ld items in one call", M);
  GmmModel& m = *h.g;
  if (m.G != h.G || m.D != h.D || m.K != h.K) throw Error(DSR_E_CONSISTENCY, "the model changed under the adaptation handle");
  std::vector<Item> items; items.reserve((size_t) M);
  for (long i = 0; i < M; i++) {
    if (frame[i] < 0 || frame[i] >= N) throw Error(DSR_E_INDEX, "item %ld: frame %d of %ld", i, frame[i], N);
    if (dist[i] < 0 || dist[i] >= h.K) throw Error(DSR_E_INDEX, "item %ld: distribution %d of %d", i, dist[i], h.K);
    h.check_accu(accu[i], "FeatureSpaceAdaptationFeature::accumulate");
    if (!h.on[dist[i]]) continue;                         // fsa:189, before anything is counted
    items.push_back(Item{accu[i], dist[i], frame[i], gamma[i], i});
  }
  const long A = (long) items.size();
  if (A == 0) return;
  // _count and _beta in item order (fsa:191, 215): beta is a float sum
  for (long i = 0; i < A; i++) { const Item& it = items[i]; h.count[it.accu] += 1.0; h.beta[it.accu] = h.beta[it.accu] + it.gamma; if (accepted) accepted[it.accu]++; }
  std::stable_sort(items.begin(), items.end(), [](const Item& a, const Item& b) { return a.accu != b.accu ? a.accu < b.accu : a.dist < b.dist; });
  std::vector<int> sFrame(A), sDist(A), chunk, accChunk(1, 0), slotAccu; std::vector<float> sGamma(A);
  for (long i = 0; i < A; i++) { sFrame[i] = items[i].frame; sDist[i] = items[i].dist; sGamma[i] = items[i].gamma; }
  for (long i0 = 0; i0 < A;) {
    long i1 = i0; while (i1 < A && items[i1].accu == items[i0].accu) i1++;
    const int slot = (int) slotAccu.size(); slotAccu.push_back(items[i0].accu);
    for (long c0 = i0; c0 < i1; c0 += kChunk) { chunk.push_back(slot); chunk.push_back((int) c0); chunk.push_back((int) std::min<long>(kChunk, i1 - c0)); }
    accChunk.push_back((int) (chunk.size() / 3));
    i0 = i1;
  }
  const int nCh = (int) (chunk.size() / 3), nSlot = (int) slotAccu.size();
  const size_t sz = (size_t) D * h.NCp;
  h.d_frame.upload(sFrame, st); h.d_dist.upload(sDist, st); h.d_gamma.upload(sGamma, st); h.d_chunk.upload(chunk, st); h.d_accChunk.upload(accChunk, st);
  h.d_gsel.reserve((size_t) A); h.d_part.reserve((size_t) nCh * sz); h.d_stats.reserve((size_t) nSlot * sz);
  {
    ScopedTimer tm(h.timing, st);
    launch(k_fsa_nearest, dim3(cdiv(A, 256)), dim3(256), 0, st, xScore, D, m.Dp, m.d_off.p, m.d_mean.p, m.d_ivar.p, m.d_cst.p, h.d_frame.p, h.d_dist.p, A,
                       h.d_gsel.p);
    h.ms[0] = tm.stop();
  }
  {
    ScopedTimer tm(h.timing, st);
    launch(k_fsa_stats, dim3(nCh), dim3(256), 0, st, D, h.NCp, h.PZ, xSrc, h.d_mean.p, h.d_ivar.p, h.d_frame.p, h.d_gamma.p, h.d_gsel.p, h.d_chunk.p,
                       h.d_pq.p, h.d_part.p);
    launch(k_fsa_reduce, dim3(cdiv((long) sz, 256), nSlot), dim3(256), 0, st, (long) sz, h.d_accChunk.p, h.d_part.p, h.d_stats.p);
    h.ms[1] = tm.stop();
  }
  std::vector<double> stats((size_t) nSlot * sz); std::vector<int> gsel(nearest ? A : 0);
  DSR_HIP(hipMemcpyAsync(stats.data(), h.d_stats.p, stats.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  if (nearest) DSR_HIP(hipMemcpyAsync(gsel.data(), h.d_gsel.p, (size_t) A * sizeof(int), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  if (nearest) for (long i = 0; i < A; i++) nearest[items[i].idx] = gsel[i] - m.off[items[i].dist];
  for (int s = 0; s < nSlot; s++) {
    double* z = h.z.data() + (size_t) slotAccu[s] * h.zsz(); double* Gi = h.Gi.data() + (size_t) slotAccu[s] * h.gsz();
    for (int i = 0; i < D; i++) {
      const double* r = stats.data() + ((size_t) s * D + i) * h.NCp;
      int col = 0;
      for (int j = 0; j < N1; j++) for (int k = 0; k <= j; k++, col++) Gi[((size_t) i * N1 + j) * N1 + k] += r[col];      // the lower triangle, fsa:235-241
      for (int n = 0; n < N1; n++) z[(size_t) i * N1 + n] += r[h.PZ + n];
    }
  }
}

void fsa_estimate(FsaHandle& h, int iterN, const int* accuX, const int* tranX, int n, hipStream_t st)
{
  const int D = h.D, N1 = D + 1;
  if (n < 0 || iterN < 0) throw Error(DSR_E_PARAMETER, "negative count");
  if (n == 0) return;
  if (!accuX || !tranX) throw Error(DSR_E_PARAMETER, "null argument");
  for (int k = 0; k < n; k++) {
    h.check_accu(accuX[k], "FeatureSpaceAdaptationFeature::estimate"); h.check_tran(tranX[k], "FeatureSpaceAdaptationFeature::estimate");
    for (int l = 0; l < k; l++) if (tranX[l] == tranX[k]) throw Error(DSR_E_PARAMETER, "transformation %d is named twice in one estimate", tranX[k]);
  }
  const size_t gs = h.gsz(), zs = h.zsz();
  std::vector<double> Gs((size_t) n * gs), zz((size_t) n * zs), W0((size_t) n * zs), beta(n);
  for (int k = 0; k < n; k++) {
    const double* src = h.Gi.data() + (size_t) accuX[k] * gs; double* dst = Gs.data() + (size_t) k * gs;
    for (int i = 0; i < D; i++) for (int j = 0; j < N1; j++) for (int c = 0; c < N1; c++)                                   // _makeSymmetric, fsa:323-328
      dst[((size_t) i * N1 + j) * N1 + c] = src[((size_t) i * N1 + (j > c ? j : c)) * N1 + (j > c ? c : j)];
    std::copy(h.z.begin() + (size_t) accuX[k] * zs, h.z.begin() + (size_t) (accuX[k] + 1) * zs, zz.begin() + (size_t) k * zs);
    std::copy(h.W.begin() + (size_t) tranX[k] * zs, h.W.begin() + (size_t) (tranX[k] + 1) * zs, W0.begin() + (size_t) k * zs);      // from the current _w, fsa:376
    beta[k] = (double) h.beta[accuX[k]];
  }
  h.d_G.upload(Gs, st); h.d_z.upload(zz, st); h.d_W.upload(W0, st); h.d_beta.upload(beta, st);
  h.d_Ginv.reserve((size_t) n * gs); h.d_flag.reserve((size_t) n);
  DSR_HIP(hipMemsetAsync(h.d_flag.p, 0, (size_t) n * sizeof(int), st));
  {
    const int m = (N1 + 1) & ~1;
    const size_t lds = ((size_t) 2 * N1 * N1 + N1 + m + 2 * kEigThreads) * sizeof(double);
    ScopedTimer tm(h.timing, st);
    launch(k_fsa_eig, dim3(n * D), dim3(kEigThreads), lds, st, D, h.d_G.p, h.d_Ginv.p, h.d_flag.p);
    h.ms[2] = tm.stop();
  }
  {
    const size_t lds = FsaWork::doubles(D, kRowThreads) * sizeof(double) + (size_t) D * sizeof(int);
    ScopedTimer tm(h.timing, st);
    launch(k_fsa_rows, dim3(n), dim3(kRowThreads), lds, st, D, iterN, h.d_Ginv.p, h.d_z.p, h.d_beta.p, h.d_W.p, h.d_flag.p);
    h.ms[3] = tm.stop();
  }
  std::vector<int> flag(n);
  DSR_HIP(hipMemcpyAsync(W0.data(), h.d_W.p, W0.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipMemcpyAsync(flag.data(), h.d_flag.p, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  int bad = -1, nBad = 0;
  for (int k = 0; k < n; k++) {
    if (flag[k]) { h.status[tranX[k]] = DSR_E_CONSISTENCY; if (bad < 0) bad = tranX[k]; nBad++; continue; }
    h.status[tranX[k]] = 0;
    std::copy(W0.begin() + (size_t) k * zs, W0.begin() + (size_t) (k + 1) * zs, h.W.begin() + (size_t) tranX[k] * zs);
  }
  h.wDirty = true;
  if (nBad) throw Error(DSR_E_CONSISTENCY, "statistics of %d transformation(s), the first %d, are not finite, too few or badly conditioned; they are unchanged", nBad, bad);
}

}  // namespace

void fsa_apply(FsaHandle& h, const float* x, const int* tranOfRow, long N, float shift, float* out, hipStream_t st)
{
  if (N < 0) throw Error(DSR_E_PARAMETER, "negative frame count");
  if (N == 0) return;
  if (!x || !out) throw Error(DSR_E_PARAMETER, "null argument");
  if ((long) N * h.D > 0x7fffffffL * 256L) throw Error(DSR_E_DIMENSION, "%ld frames in one call", N);
  if (h.wDirty) { h.d_Wall.upload(h.W, st); h.wDirty = false; }
  ScopedTimer tm(h.timing, st);
  launch(k_fsa_apply, dim3(cdiv(N * h.D, 256)), dim3(256), 0, st, h.D, N, h.nTran, x, tranOfRow, h.d_Wall.p, shift, out);
  h.ms[4] = tm.stop();
}

}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_fsa_create(dsr_gmm* g, int nAccu, int nTran, dsr_fsa** out)
{
  return guard([&] {
    if (!g || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (nAccu < 1 || nTran < 1 || nAccu > 65535) throw Error(DSR_E_PARAMETER, "%d accumulators, %d transformations", nAccu, nTran);
    if (g->D > kFsaMaxD) throw Error(DSR_E_DIMENSION, "dimN = %d: feature-space adaptation is built for dimN <= %d", g->D, kFsaMaxD);
    if (g->D < 1 || g->K < 1) throw Error(DSR_E_DIMENSION, "empty model");
    require_device();
    dsr_fsa* h = new dsr_fsa();
    try {
      const int D = g->D, N1 = D + 1;
      h->g = g; h->D = D; h->G = g->G; h->K = g->K; h->maxRef = g->maxRef; h->nAccu = nAccu; h->nTran = nTran;      // _initialize, fsa:43-112
      h->on.assign(h->K, 0); h->count.assign(nAccu, 0.0); h->beta.assign(nAccu, 0.0f);
      h->z.assign((size_t) nAccu * h->zsz(), 0.0); h->Gi.assign((size_t) nAccu * h->gsz(), 0.0);
      h->W.assign((size_t) nTran * h->zsz(), 0.0); h->status.assign(nTran, 0);
      for (int t = 0; t < nTran; t++) for (int i = 0; i < D; i++) h->W[((size_t) t * D + i) * N1 + i + 1] = 1.0;
      const int P = N1 * (N1 + 1) / 2; h->PZ = (P + 15) & ~15; h->NCp = (h->PZ + N1 + 15) & ~15;
      std::vector<int> pq(h->NCp, -1);
      { int col = 0; for (int j = 0; j < N1; j++) for (int k = 0; k <= j; k++) pq[col++] = j | (k << 16); for (int n = 0; n < N1; n++) pq[h->PZ + n] = n; }
      h->d_pq.upload(pq); h->d_mean.upload(g->mean); h->d_ivar.upload(g->ivar);
    } catch (...) { delete h; throw; }
    *out = h;
  });
}
void dsr_fsa_destroy(dsr_fsa* h) { delete h; }

dsr_status dsr_fsa_accumulate(dsr_fsa* h, const float* xScore_dev, const float* xSrc_dev, int64_t N, const int32_t* frame, const int32_t* dist, const float* gamma,
                              const int32_t* accu, int64_t M, int64_t* accepted, int32_t* nearest, void* stream)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    fsa_accumulate(*h, xScore_dev, xSrc_dev, (long) N, frame, dist, gamma, accu, (long) M, accepted, nearest, (hipStream_t) stream);
  });
}

dsr_status dsr_fsa_accumulate_path(dsr_fsa* h, const float* xScore_dev, const float* xSrc_dev, int64_t T, const int32_t* distIds, int64_t pathLen, int accuX,
                                   float factor, unsigned* framesN, void* stream)
{
  return guard([&] {
    if (!h || (pathLen > 0 && !distIds)) throw Error(DSR_E_PARAMETER, "null argument");
    if (pathLen < 0 || pathLen > 0x7fffffffL) throw Error(DSR_E_PARAMETER, "bad path length");
    h->check_accu(accuX, "FeatureSpaceAdaptationFeature::accumulate");
    std::vector<int> frame, dist; unsigned frameX = 0;
    for (long i = 0; i < pathLen; i++) {                  // fsa:284-294: a name that is not found does not advance the frame
      if (distIds[i] < 0) continue;
      dist.push_back(distIds[i]); frame.push_back((int) frameX++);
    }
    std::vector<float> fac(frame.size(), factor); std::vector<int> accu(frame.size(), accuX);
    fsa_accumulate(*h, xScore_dev, xSrc_dev, (long) T, frame.data(), dist.data(), fac.data(), accu.data(), (long) frame.size(), nullptr, nullptr, (hipStream_t) stream);
    if (framesN) *framesN = frameX;
  });
}

dsr_status dsr_fsa_accumulate_lattice(dsr_fsa* h, dsr_lattice* L, const float* xScore_dev, const float* xSrc_dev, int64_t T, int accuX, float factor,
                                      unsigned* linksN, void* stream)
{
  return guard([&] {
    if (!h || !L) throw Error(DSR_E_PARAMETER, "null argument");
    h->check_accu(accuX, "FeatureSpaceAdaptationFeature::accumulateLattice");
    const size_t E = L->from.size(), nn = L->nodeFinal.size();
    std::vector<double> gamma(E); std::vector<int32_t> edgeLive(E), nodeLive(nn);
    const dsr_status s = dsr_lattice_get_state(L, gamma.data(), edgeLive.data(), nullptr, nodeLive.data(), nullptr, nullptr);
    if (s) throw Error(s, "%s", dsr_last_error());
    std::vector<int> frame, dist, accu; std::vector<float> fac; unsigned cnt = 0;
    for (size_t e = 0; e < E; e++) {                        // the links Lattice::EdgeIterator sees, fsa:303-319
      if (!edgeLive[e] || !nodeLive[L->from[e]]) continue;
      if (L->in[e] == 0) continue;
      if (gamma[e] > 10.0) continue;
      const float post = (float) ((double) factor * exp(-gamma[e]));
      if (L->in[e] - 1 >= (unsigned) h->K) throw Error(DSR_E_INDEX, "link %zu: distribution %u of %d", e, L->in[e] - 1, h->K);
      if (L->start[e] < 0 || L->end[e] >= T) throw Error(DSR_E_INDEX, "link %zu: frames %d..%d of %ld", e, L->start[e], L->end[e], (long) T);
      cnt++;
      for (int f = L->start[e]; f <= L->end[e]; f += 2) { frame.push_back(f); dist.push_back((int) L->in[e] - 1); fac.push_back(post); accu.push_back(accuX); }   // fsa:317-318
    }
    fsa_accumulate(*h, xScore_dev, xSrc_dev, (long) T, frame.data(), dist.data(), fac.data(), accu.data(), (long) frame.size(), nullptr, nullptr, (hipStream_t) stream);
    if (linksN) *linksN = cnt;
  });
}

dsr_status dsr_fsa_estimate(dsr_fsa* h, int iterN, const int32_t* accuX, const int32_t* tranX, int n, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); fsa_estimate(*h, iterN, accuX, tranX, n, (hipStream_t) stream); }); }

dsr_status dsr_fsa_apply(dsr_fsa* h, const float* x_dev, int64_t N, const int32_t* tranOfRow_dev, float shift, float* out_dev, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); fsa_apply(*h, x_dev, tranOfRow_dev, (long) N, shift, out_dev, (hipStream_t) stream); }); }

}  // extern "C"
