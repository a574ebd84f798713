// csrc/k_stc.hip -- semi-tied covariance (STC) and LDA transforms: statistics, estimation and the transforms on the device.
//
// Replaces STCEstimator::accumulate / Accu::accumulateW1 / accumulateW2 (asr/train/estimateAdapt.cc:2265-2294, 2569-2651, "eA"), makePosDef and
// _update (eA:2387-2464, 2689-2711), LDAEstimator::accumulate / Accu::accumulate (eA:2761-2790, 2989-3036) and _update (eA:2793-2836), and
// STCTransformer::_transform / LDATransformer::next (asr/adapt/transform.cc:1866-1879, 1937-1959, "tr"), which work on one frame and one
// estimator at a time, for batches of items, several estimators and whole utterances.
//
//   k_stc_nearest  thread per item: the nearest Gaussian of the item's codebook under the scoring frame -- the one-hot addCount of
//                  CodebookBasic::_scoreOpt -- and the distribution's score, with the arithmetic of scoring mode 0 (gmm_dist.h).
//   k_stc_stats    items sorted by estimator, then codebook (stable, on the host); one workgroup per chunk of kChunk items of one estimator.
//                  With g the item's Gaussian, c = float(addCount factor) and o = float(x - mu_g) (x under the estimator's current matrix when
//                  it cascades, eA:2276-2278), rows d = feature, the contraction over the items of
//                      sumOsq[d][(i, j)] += float(iv_gd c) (o_i o_j)   (j <= i, one column per pair, eA:2593-2603)   and, for factor <= 0,
//                      R[d][col]         += iv_gd float(-c / iv_g,col)                                                  (eA:2612-2648)
//                  on v_mfma_f64_16x16x4_f64.  Both operands are exact in fp64 and formed in registers.  The R columns start at a multiple
//                  of 16, so a 16-column tile is of one kind (the layout of k_fsa_stats with centred observations for xi = (1, x)).
//   k_lda_stats    the same chunks; within, between and mixture (eA:3012-3033) as three symmetric rank-n updates, rows i with the operand
//                  c o_i (exact: 24 + 24 bits), columns j with o_j, lower-triangle tiles only.
//   k_stc_reduce   workgroup row per estimator: the sum of its chunks in chunk order.  No floating-point atomics: the same call twice gives
//                  the same bits.  The host adds the sums to its accumulators (csrc/stc.h).
//   k_stc_eig      workgroup per (estimator, d): eigenvalues and inverse of sumOsq[d] + E regSq[d] by Jacobi rotations in LDS (stc_rows.h).
//   k_stc_rows     workgroup per estimator: A, A^-1 and the sign of det A in LDS, MaxItns x dimN row updates (stc_rows.h).
//   k_lda_solve    workgroup per estimator: the two eigen-decompositions and the products of the simultaneous diagonalisation (stc_rows.h).
//   k_stc_apply    thread per (frame, output dimension): float(sum_j double(x_j) M[i][j]), j ascending, no bias; outDim <= Din rows.
// The pair indexing and tile walk restate k_fsa_stats': k_fsa.hip and k_mllr.hip are left as they are, so their object code does not change.
// This translation unit is compiled with -ffp-contract=off.
#include "launch.h"
#include "stc.h"
#include "mfma64.h"
#include "gmm_dist.h"
#include "stc_rows.h"
#include <algorithm>
#include <cmath>

namespace dsr {

static constexpr int kChunk = 64;                         // items per workgroup of the statistics kernels: 16 k-steps
static constexpr int kEigThreads = 128, kRowThreads = 256;

__global__ __launch_bounds__(256) void k_stc_nearest(const float* __restrict__ x, int D, int DP, const int* __restrict__ off, const float* __restrict__ mean,
                                                     const float* __restrict__ ivar, const float* __restrict__ cst, const float* __restrict__ val,
                                                     const float* __restrict__ scale, const int* __restrict__ sFrame, const int* __restrict__ sDist, long M,
                                                     int* __restrict__ gsel, float* __restrict__ score)
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
  float sc = (float) (0.5 * (double) __fadd_rn(minDist, __fmul_rn(2.0f, val[a + minIdx])));      // as k_gmm_exact finishes mode 0
  const float s = scale[k]; if (s != 1.0f) sc = __fmul_rn(sc, s);
  score[i] = sc;
}

// the statistics' frame of item j, feature d: x, or x under the estimator's matrix A [D][D] (tr:1866-1879)
__device__ __forceinline__ float stat_feature(const float* __restrict__ xp, const double* __restrict__ A, int D, int d)
{
  if (!A) return xp[d];
  double sum = 0.0;
  for (int j = 0; j < D; j++) sum = __dadd_rn(sum, __dmul_rn((double) xp[j], A[(long) d * D + j]));
  return (float) sum;
}

// chunk[3 c] = { estimator, first sorted item, items }; pq[col] = i | j << 16 of a pair column, col of an R column, -1 of padding
__global__ __launch_bounds__(256) void k_stc_stats(int D, int NCp, int PZ, const float* __restrict__ x, const double* __restrict__ Aall,
                                                   const float* __restrict__ mean, const float* __restrict__ ivar, const int* __restrict__ sFrame,
                                                   const float* __restrict__ sFac, const int* __restrict__ gsel, const int* __restrict__ chunk,
                                                   const int* __restrict__ pq, double* __restrict__ part)
{
  __shared__ float o[kChunk * kStcMaxD]; __shared__ float fac[kChunk]; __shared__ int sg[kChunk]; __shared__ int sf[kChunk];
  const int ch = blockIdx.x;
  const int est = chunk[3 * ch], i0 = chunk[3 * ch + 1], n = chunk[3 * ch + 2];
  const double* A = Aall ? Aall + (long) est * D * D : nullptr;
  for (int j = threadIdx.x; j < kChunk; j += blockDim.x) {
    const bool in = j < n;
    sg[j] = in ? gsel[i0 + j] : 0; fac[j] = in ? sFac[i0 + j] : 0.0f; sf[j] = in ? sFrame[i0 + j] : 0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n * D; e += blockDim.x) {
    const int j = e / D, d = e - j * D;
    o[e] = __fsub_rn(stat_feature(x + (long) sf[j] * D, A, D, d), mean[(long) sg[j] * D + d]);      // eA:2590-2591
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  const int RT = (D + 15) >> 4, CT = NCp >> 4;
  double* out = part + (long) ch * D * NCp;
  for (int rt = 0; rt < RT; rt++) {
    const int row = rt * 16 + lo;                         // A: feature `row` of item 4 ks + hi
    double aW[kChunk / 4], aR[kChunk / 4];
#pragma unroll
    for (int ks = 0; ks < kChunk / 4; ks++) {
      const int j = 4 * ks + hi; aW[ks] = 0.0; aR[ks] = 0.0;
      if (row < D && j < n) {
        const float iv = ivar[(long) sg[j] * D + row];
        aW[ks] = (double) __fmul_rn(iv, fac[j]);                             // eA:2594: a float product
        if (!(fac[j] > 0.0f)) aR[ks] = (double) iv;                          // eA:2612, 2644
      }
    }
    for (int ct = wave; ct < CT; ct += 4) {               // uniform per wave
      const int col = ct * 16 + lo, code = pq[col];
      const bool isR = ct * 16 >= PZ;
      const int p = code < 0 ? 0 : (code & 0xffff), q = (code < 0 || isR) ? 0 : (code >> 16);
      d4 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < kChunk / 4; ks++) {
        const int j = 4 * ks + hi;
        double b = 0.0;
        if (j < n && code >= 0) {
          if (!isR) b = __dmul_rn((double) o[j * D + p], (double) o[j * D + q]);                  // exact: 24 + 24 bits
          else if (!(fac[j] > 0.0f)) b = (double) __fdiv_rn(-fac[j], ivar[(long) sg[j] * D + p]);  // eA:2621, 2632: floats
        }
        c = mfma64(isR ? aR[ks] : aW[ks], b, c);
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int orow = rt * 16 + hi + 4 * r;
        if (orow < D) out[(long) orow * NCp + col] = c[r];
      }
    }
  }
}

// part [chunk][3][D][D]: within, between, mixture; tiles above the diagonal are not written (k_stc_reduce does not read them)
__global__ __launch_bounds__(256) void k_lda_stats(int D, const float* __restrict__ x, const float* __restrict__ mean, const float* __restrict__ mu0,
                                                   const int* __restrict__ sFrame, const float* __restrict__ sFac, const int* __restrict__ gsel,
                                                   const int* __restrict__ chunk, double* __restrict__ part)
{
  __shared__ float o[3][kChunk * kStcMaxD]; __shared__ float fac[kChunk]; __shared__ int sg[kChunk]; __shared__ int sf[kChunk];
  const int ch = blockIdx.x;
  const int i0 = chunk[3 * ch + 1], n = chunk[3 * ch + 2];
  for (int j = threadIdx.x; j < kChunk; j += blockDim.x) {
    const bool in = j < n;
    sg[j] = in ? gsel[i0 + j] : 0; fac[j] = in ? sFac[i0 + j] : 0.0f; sf[j] = in ? sFrame[i0 + j] : 0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < n * D; e += blockDim.x) {
    const int j = e / D, d = e - j * D;
    const float xv = x[(long) sf[j] * D + d], mu = mean[(long) sg[j] * D + d], m0 = mu0[d];
    o[0][e] = __fsub_rn(xv, mu); o[1][e] = __fsub_rn(mu, m0); o[2][e] = __fsub_rn(xv, m0);       // eA:3013-3015
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  const int RT = (D + 15) >> 4, TT = RT * (RT + 1) / 2;
  double* out = part + (long) ch * 3 * D * D;
  for (int t = wave; t < 3 * TT; t += 4) {                // uniform per wave
    const int mat = t / TT; int rt = 0, ct = t - mat * TT;
    while (ct > rt) { ct -= rt + 1; rt++; }
    const float* om = o[mat];
    const int row = rt * 16 + lo, col = ct * 16 + lo;
    d4 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < kChunk / 4; ks++) {
      const int j = 4 * ks + hi;
      double a = 0.0, b = 0.0;
      if (j < n) {
        if (row < D) a = __dmul_rn((double) fac[j], (double) om[j * D + row]);                  // exact: 24 + 24 bits, eA:3022
        if (col < D) b = (double) om[j * D + col];
      }
      c = mfma64(a, b, c);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int orow = rt * 16 + hi + 4 * r;
      if (orow < D && col < D) out[((long) mat * D + orow) * D + col] = c[r];
    }
  }
}

// tri > 0: the elements are tri x tri matrices of which only column <= row is summed (the rest is zero)
__global__ __launch_bounds__(256) void k_stc_reduce(long sz, int tri, const int* __restrict__ accChunk, const double* __restrict__ part, double* __restrict__ stats)
{
  const int slot = blockIdx.y, c0 = accChunk[slot], c1 = accChunk[slot + 1];
  const long e = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= sz) return;
  double t = 0.0;
  if (tri <= 0 || (e % tri) <= ((e / tri) % tri))
    for (int ch = c0; ch < c1; ch++) t = __dadd_rn(t, part[(long) ch * sz + e]);
  stats[(long) slot * sz + e] = t;
}

// one workgroup per (estimator k, row d): G [k][d][D][D] -> Ginv, ev [k][d][2]
__global__ __launch_bounds__(kEigThreads) void k_stc_eig(int D, const double* __restrict__ G, double* __restrict__ Ginv, double* __restrict__ ev, int* __restrict__ flag)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = D, m = (n + 1) & ~1, nt = blockDim.x, tid = threadIdx.x;
  double* a = reinterpret_cast<double*>(smem);            // [n][n]
  double* v = a + n * n;                                  // [n][n]
  double* t = v + n * n;                                  // [n]
  double* cs = t + n;                                     // [m]
  double* sq = cs + m;                                    // [2 nt]
  const int k = blockIdx.x / D;
  const double* src = G + (long) blockIdx.x * n * n;
  for (int e = tid; e < n * n; e += nt) a[e] = src[e];
  __syncthreads();
  const bool ok = stc_eig_run(a, v, t, cs, sq, n, Ginv + (long) blockIdx.x * n * n, ev + 2 * (long) blockIdx.x, tid, nt, [] { __syncthreads(); });
  if (!ok && tid == 0) flag[k] = 1;
}

// one workgroup per estimator: Aio [k][D][D] in and, unless the estimator is flagged, out; Ai [k][D][D] the result's inverse
__global__ __launch_bounds__(kRowThreads) void k_stc_rows(int D, int itns, const double* __restrict__ Ginv, const double* __restrict__ gamma, double* __restrict__ Aio,
                                                          double* __restrict__ Ai, int* __restrict__ flag)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nt = blockDim.x, tid = threadIdx.x, k = blockIdx.x;
  if (flag[k]) return;                                    // set on the host or by k_stc_eig, a launch earlier: uniform
  StcWork w; w.carve(reinterpret_cast<double*>(smem), D, nt);
  double* Ak = Aio + (long) k * D * D;
  for (int e = tid; e < D * D; e += nt) w.A[e] = Ak[e];
  __syncthreads();
  const bool ok = stc_rows_run(w, D, itns, Ginv + (long) k * D * D * D, gamma[k], tid, nt, [] { __syncthreads(); });
  if (!ok) { if (tid == 0) flag[k] = 1; return; }
  for (int e = tid; e < D * D; e += nt) { Ak[e] = w.A[e]; Ai[(long) k * D * D + e] = w.Ai[e]; }
}

// one workgroup per estimator: W, B [k][D][D] symmetric -> L [k][D][D], ev [k][2 D]
__global__ __launch_bounds__(kRowThreads) void k_lda_solve(int D, const double* __restrict__ W, const double* __restrict__ B, double* __restrict__ L,
                                                           double* __restrict__ ev, int* __restrict__ flag)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int n = D, m = (n + 1) & ~1, nt = blockDim.x, tid = threadIdx.x, k = blockIdx.x;
  double* a = reinterpret_cast<double*>(smem);
  double* v = a + n * n; double* u = v + n * n; double* lam = u + n * n; double* cs = lam + 2 * n; double* sq = cs + m;
  int* ord = reinterpret_cast<int*>(sq + 2 * nt);
  const bool ok = lda_run(W + (long) k * n * n, B + (long) k * n * n, a, v, u, lam, cs, sq, ord, n, L + (long) k * n * n, ev + 2 * (long) k * n, tid, nt,
                          [] { __syncthreads(); });
  if (!ok && tid == 0) flag[k] = 1;
}

// M [Din][Din] of which the first outDim rows are used; x [N][Din] -> out [N][outDim]
__global__ __launch_bounds__(256) void k_stc_apply(int Din, int outDim, long N, const float* __restrict__ x, const double* __restrict__ M, float* __restrict__ out)
{
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= N * outDim) return;
  const long r = idx / outDim; const int i = (int) (idx - r * outDim);
  const float* xp = x + r * Din; const double* mr = M + (long) i * Din;
  double sum = 0.0;
  for (int j = 0; j < Din; j++) sum = __dadd_rn(sum, __dmul_rn((double) xp[j], mr[j]));          // tr:1873-1876, 1951-1954
  out[idx] = (float) sum;
}

namespace {

struct Item { int est, dist, frame; float fac; long idx; };
struct Plan {
  std::vector<Item> items;                                // sorted by estimator, then codebook
  std::vector<int> chunk, accChunk, slotEst; std::vector<int> gsel; std::vector<float> score;
  int nCh = 0, nSlot = 0;
};

// checks the M items, sorts them, cuts the chunks, and finds every item's Gaussian and score (k_stc_nearest)
void plan_items(XfBase& h, const float* xScore, long N, const int* frame, const int* dist, const float* fac, const int* est, long M, const char* who, Plan& p,
                hipStream_t st)
{
  if (!xScore || !frame || !dist || !fac || !est) throw Error(DSR_E_PARAMETER, "null argument");
  if (M > 0x7fffffffL - kChunk) throw Error(DSR_E_DIMENSION, "%ld items in one call", M);
  if (!h.g) throw Error(DSR_E_CONSISTENCY, "%s: a transformer without a distribution set has no statistics", who);
  GmmModel& m = *h.g;
  if (m.G != h.G || m.D != h.D || m.K != h.K) throw Error(DSR_E_CONSISTENCY, "the model changed under the estimator handle");
  p.items.reserve((size_t) M);
  for (long i = 0; i < M; i++) {
    if (frame[i] < 0 || frame[i] >= N) throw Error(DSR_E_INDEX, "item %ld: frame %d of %ld", i, frame[i], N);
    if (dist[i] < 0 || dist[i] >= h.K) throw Error(DSR_E_INDEX, "item %ld: distribution %d of %d", i, dist[i], h.K);
    h.check_est(est[i], who);
    p.items.push_back(Item{est[i], dist[i], frame[i], fac[i], i});
  }
  std::stable_sort(p.items.begin(), p.items.end(), [](const Item& a, const Item& b) { return a.est != b.est ? a.est < b.est : a.dist < b.dist; });
  std::vector<int> sFrame(M), sDist(M); std::vector<float> sFac(M);
  for (long i = 0; i < M; i++) { sFrame[i] = p.items[i].frame; sDist[i] = p.items[i].dist; sFac[i] = p.items[i].fac; }
  p.accChunk.assign(1, 0);
  for (long i0 = 0; i0 < M;) {
    long i1 = i0; while (i1 < M && p.items[i1].est == p.items[i0].est) i1++;
    p.slotEst.push_back(p.items[i0].est);
    for (long c0 = i0; c0 < i1; c0 += kChunk) { p.chunk.push_back(p.items[i0].est); p.chunk.push_back((int) c0); p.chunk.push_back((int) std::min<long>(kChunk, i1 - c0)); }
    p.accChunk.push_back((int) (p.chunk.size() / 3));
    i0 = i1;
  }
  p.nCh = (int) (p.chunk.size() / 3); p.nSlot = (int) p.slotEst.size();
  h.d_frame.upload(sFrame, st); h.d_dist.upload(sDist, st); h.d_fac.upload(sFac, st); h.d_chunk.upload(p.chunk, st); h.d_accChunk.upload(p.accChunk, st);
  h.d_gsel.reserve((size_t) M); h.d_score.reserve((size_t) M);
  {
    ScopedTimer tm(h.timing, st);
    launch(k_stc_nearest, dim3(cdiv(M, 256)), dim3(256), 0, st, xScore, h.D, m.Dp, m.d_off.p, m.d_mean.p, m.d_ivar.p, m.d_cst.p, m.d_val.p, m.d_scale.p,
                       h.d_frame.p, h.d_dist.p, M, h.d_gsel.p, h.d_score.p);
    h.ms[0] = tm.stop();
  }
  p.gsel.resize((size_t) M); p.score.resize((size_t) M);
  DSR_HIP(hipMemcpyAsync(p.gsel.data(), h.d_gsel.p, (size_t) M * sizeof(int), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipMemcpyAsync(p.score.data(), h.d_score.p, (size_t) M * sizeof(float), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
}

void hand_back(const XfBase& h, const Plan& p, int32_t* nearest, float* score)
{
  for (size_t i = 0; i < p.items.size(); i++) {
    if (nearest) nearest[p.items[i].idx] = p.gsel[i] - h.g->off[p.items[i].dist];
    if (score) score[p.items[i].idx] = p.score[i];
  }
}

}  // namespace

void stc_accumulate(StcHandle& h, const float* xScore, const float* xSrc, long N, const int* frame, const int* dist, const float* fac, const int* est, long M,
                    int32_t* nearest, float* score, hipStream_t st)
{
  const int D = h.D;
  if (M < 0 || N < 0) throw Error(DSR_E_PARAMETER, "negative size");
  if (M == 0) return;
  if (!xSrc) throw Error(DSR_E_PARAMETER, "null argument");
  Plan p; plan_items(h, xScore, N, frame, dist, fac, est, M, "STCEstimator::accumulate", p, st);
  const size_t sz = (size_t) D * h.NCp;
  h.d_part.reserve((size_t) p.nCh * sz); h.d_stats.reserve((size_t) p.nSlot * sz);
  if (h.cascade && h.aDirty) { h.d_Aall.upload(h.A, st); h.aDirty = false; }
  {
    ScopedTimer tm(h.timing, st);
    launch(k_stc_stats, dim3(p.nCh), dim3(256), 0, st, D, h.NCp, h.PZ, xSrc, h.cascade ? h.d_Aall.p : (const double*) nullptr, h.d_mean.p, h.d_ivar.p,
                       h.d_frame.p, h.d_fac.p, h.d_gsel.p, h.d_chunk.p, h.d_pq.p, h.d_part.p);
    launch(k_stc_reduce, dim3(cdiv((long) sz, 256), p.nSlot), dim3(256), 0, st, (long) sz, 0, h.d_accChunk.p, h.d_part.p, h.d_stats.p);
    h.ms[1] = tm.stop();
  }
  std::vector<double> stats((size_t) p.nSlot * sz);
  DSR_HIP(hipMemcpyAsync(stats.data(), h.d_stats.p, stats.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  hand_back(h, p, nearest, score);
  // the handle changes only now that the device's part of the call is done.  _count and _denCount in item order (eA:2579-2584): count =
  // addCount (1.0f) x factor
  for (long i = 0; i < M; i++) { const float c = fac[i]; if (c > 0.0f) h.count[est[i]] += c; else if (c < 0.0f) h.denCount[est[i]] -= c; }
  std::vector<char> den(h.nEst, 0);
  for (long i = 0; i < M; i++) if (!(fac[i] > 0.0f)) den[est[i]] = 1;
  for (int s = 0; s < p.nSlot; s++) {
    const int e = p.slotEst[s];
    double* S = h.sumOsq.data() + (size_t) e * h.ssz(); double* R = h.regSq.data() + (size_t) e * h.ssz();
    const double* Ai = h.Ainv.data() + (size_t) e * h.msz();
    for (int d = 0; d < D; d++) {
      const double* r = stats.data() + ((size_t) s * D + d) * h.NCp;
      int col = 0;
      for (int i = 0; i < D; i++) for (int j = 0; j <= i; j++, col++) S[((size_t) d * D + i) * D + j] += r[col];      // the lower triangle, eA:2597-2601
      if (!den[e]) continue;
      // regSq[d] += sum_col R[d][col] a_col a_col^T with a_col the columns of _stcInv (eA:2628-2647)
      for (int i = 0; i < D; i++) for (int j = 0; j <= i; j++) {
        double sum = 0.0;
        for (int c = 0; c < D; c++) sum += r[h.PZ + c] * (Ai[(size_t) i * D + c] * Ai[(size_t) j * D + c]);
        R[((size_t) d * D + i) * D + j] += sum;
      }
    }
  }
}

void lda_accumulate(LdaHandle& h, const float* xScore, const float* xSrc, long N, const int* frame, const int* dist, const float* fac, const int* est, long M,
                    int32_t* nearest, float* score, hipStream_t st)
{
  const int D = h.D;
  if (M < 0 || N < 0) throw Error(DSR_E_PARAMETER, "negative size");
  if (M == 0) return;
  if (!xSrc || !dist) throw Error(DSR_E_PARAMETER, "null argument");
  if (!h.g) throw Error(DSR_E_CONSISTENCY, "LDAEstimator::accumulate: a transformer without a distribution set has no statistics");
  for (long i = 0; i < M; i++)                            // eA:2995, before anything is counted
    if (dist[i] >= 0 && dist[i] < h.K && h.g->refN[dist[i]] != h.globalRefN)
      throw Error(DSR_E_DIMENSION, "Codebook sizes (%d and %d) do not match.", h.g->refN[dist[i]], h.globalRefN);
  Plan p; plan_items(h, xScore, N, frame, dist, fac, est, M, "LDAEstimator::accumulate", p, st);
  const size_t sz = (size_t) 3 * D * D;
  h.d_part.reserve((size_t) p.nCh * sz); h.d_stats.reserve((size_t) p.nSlot * sz);
  {
    ScopedTimer tm(h.timing, st);
    launch(k_lda_stats, dim3(p.nCh), dim3(256), 0, st, D, xSrc, h.d_mean.p, h.d_mu0.p, h.d_frame.p, h.d_fac.p, h.d_gsel.p, h.d_chunk.p, h.d_part.p);
    launch(k_stc_reduce, dim3(cdiv((long) sz, 256), p.nSlot), dim3(256), 0, st, (long) sz, D, h.d_accChunk.p, h.d_part.p, h.d_stats.p);
    h.ms[1] = tm.stop();
  }
  std::vector<double> stats((size_t) p.nSlot * sz);
  DSR_HIP(hipMemcpyAsync(stats.data(), h.d_stats.p, stats.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  hand_back(h, p, nearest, score);
  for (long i = 0; i < M; i++) h.count[est[i]] += fac[i];                                         // eA:3004; the handle changes only now
  for (int s = 0; s < p.nSlot; s++) {
    const int e = p.slotEst[s];
    double* dst[3] = { h.within.data() + (size_t) e * h.msz(), h.between.data() + (size_t) e * h.msz(), h.mixture.data() + (size_t) e * h.msz() };
    for (int mat = 0; mat < 3; mat++) {
      const double* r = stats.data() + ((size_t) s * 3 + mat) * h.msz();
      for (int i = 0; i < D; i++) for (int j = 0; j <= i; j++) dst[mat][(size_t) i * D + j] += r[(size_t) i * D + j];
    }
  }
}

// STCEstimator::estimate (eA:2296-2316) for n estimators at once
void stc_estimate(StcHandle& h, const int* estX, int n, double minE, double multE, hipStream_t st)
{
  const int D = h.D;
  if (n < 0) throw Error(DSR_E_PARAMETER, "negative count");
  if (n == 0) return;
  if (!estX) throw Error(DSR_E_PARAMETER, "null argument");
  if (!h.g) throw Error(DSR_E_CONSISTENCY, "STCEstimator::estimate: a transformer without a distribution set has no statistics");
  for (int k = 0; k < n; k++) {
    h.check_est(estX[k], "STCEstimator::estimate");
    for (int l = 0; l < k; l++) if (estX[l] == estX[k]) throw Error(DSR_E_PARAMETER, "estimator %d is named twice in one estimate", estX[k]);
  }
  const size_t ss = h.ssz(), ms = h.msz();
  // sumOsq() / regSq() copy the lower triangle up on every read (estimateAdapt.h:688-689): the accumulators themselves become symmetric
  for (int k = 0; k < n; k++)
    for (double* M : { h.sumOsq.data() + (size_t) estX[k] * ss, h.regSq.data() + (size_t) estX[k] * ss })
      for (int d = 0; d < D; d++) for (int i = 0; i < D; i++) for (int j = i + 1; j < D; j++) M[((size_t) d * D + i) * D + j] = M[((size_t) d * D + j) * D + i];
  std::vector<double> G((size_t) n * ss), E(n, minE), ev((size_t) n * D * 2); std::vector<int> flag(n, 0), done(n, 0);
  h.d_Ginv.reserve((size_t) n * ss); h.d_ev.reserve(ev.size()); h.d_flag.reserve((size_t) n);
  const size_t ldsE = ((size_t) 2 * D * D + D + ((D + 1) & ~1) + 2 * kEigThreads) * sizeof(double);
  {
    // makePosDef (eA:2689-2711): E doubles until every sumOsq[d] + E regSq[d] is positive definite.  An estimator that is not and whose regSq is
    // zero, or that is still not after 64 doublings, can never be (the reference would not return): it is flagged.
    h.ms[2] = 0.0f;                                       // the k_stc_eig launches alone, summed; the host's part of makePosDef is not in it
    for (int round = 0; round <= 64; round++) {
      for (int k = 0; k < n; k++) {
        if (done[k] || flag[k]) continue;
        const double* S = h.sumOsq.data() + (size_t) estX[k] * ss; const double* R = h.regSq.data() + (size_t) estX[k] * ss; double* g = G.data() + (size_t) k * ss;
        for (size_t e = 0; e < ss; e++) g[e] = S[e] + E[k] * R[e];                                // eA:2698-2699
      }
      h.d_G.upload(G, st);
      DSR_HIP(hipMemsetAsync(h.d_flag.p, 0, (size_t) n * sizeof(int), st));
      {
        ScopedTimer tm(h.timing, st);
        launch(k_stc_eig, dim3(n * D), dim3(kEigThreads), ldsE, st, D, h.d_G.p, h.d_Ginv.p, h.d_ev.p, h.d_flag.p);
        h.ms[2] += tm.stop();
      }
      std::vector<int> f(n);
      DSR_HIP(hipMemcpyAsync(ev.data(), h.d_ev.p, ev.size() * sizeof(double), hipMemcpyDeviceToHost, st));
      DSR_HIP(hipMemcpyAsync(f.data(), h.d_flag.p, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, st));
      DSR_HIP(hipStreamSynchronize(st));
      bool again = false;
      for (int k = 0; k < n; k++) {
        if (done[k] || flag[k]) continue;
        if (f[k]) { flag[k] = 1; continue; }
        bool pd = true;
        for (int d = 0; d < D; d++) if (!stc_posdef(ev[((size_t) k * D + d) * 2], ev[((size_t) k * D + d) * 2 + 1], D)) pd = false;
        if (pd) { done[k] = 1; continue; }
        const double* R = h.regSq.data() + (size_t) estX[k] * ss; bool any = false;
        for (size_t e = 0; e < ss && !any; e++) any = R[e] != 0.0;
        if (!any || round == 64) { flag[k] = 1; continue; }
        E[k] *= 2.0; again = true;
      }
      if (!again) break;
    }
  }
  // an estimator that was done in an earlier round is decomposed again in the later ones, from the same G to the same bits
  std::vector<double> A0((size_t) n * ms), gamma(n);
  for (int k = 0; k < n; k++) {
    E[k] *= multE;                                        // eA:2710; _update inverts with the multiplied E (eA:2400-2410), see below
    std::copy(h.A.begin() + (size_t) estX[k] * ms, h.A.begin() + (size_t) (estX[k] + 1) * ms, A0.begin() + (size_t) k * ms);
    gamma[k] = h.mmi ? h.denCount[estX[k]] * E[k] : h.count[estX[k]];                             // eA:2437
  }
  if (multE != 1.0) {                                     // the inverses belong to the final E
    for (int k = 0; k < n; k++) {
      const double* S = h.sumOsq.data() + (size_t) estX[k] * ss; const double* R = h.regSq.data() + (size_t) estX[k] * ss; double* g = G.data() + (size_t) k * ss;
      for (size_t e = 0; e < ss; e++) g[e] = S[e] + E[k] * R[e];
    }
    h.d_G.upload(G, st);
    std::vector<int> f(n);
    DSR_HIP(hipMemsetAsync(h.d_flag.p, 0, (size_t) n * sizeof(int), st));
    {
      ScopedTimer tm(h.timing, st);
      launch(k_stc_eig, dim3(n * D), dim3(kEigThreads), ldsE, st, D, h.d_G.p, h.d_Ginv.p, h.d_ev.p, h.d_flag.p);
      h.ms[2] += tm.stop();
    }
    DSR_HIP(hipMemcpyAsync(ev.data(), h.d_ev.p, ev.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    DSR_HIP(hipMemcpyAsync(f.data(), h.d_flag.p, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, st));
    DSR_HIP(hipStreamSynchronize(st));
    for (int k = 0; k < n; k++) {
      if (f[k]) flag[k] = 1;
      for (int d = 0; d < D; d++) if (!stc_posdef(ev[((size_t) k * D + d) * 2], ev[((size_t) k * D + d) * 2 + 1], D)) flag[k] = 1;      // Ginv is zero there
    }
  }
  h.d_A.upload(A0, st); h.d_gamma.upload(gamma, st); h.d_Ai.reserve((size_t) n * ms);
  h.d_flag.upload(flag, st);
  {
    const size_t lds = StcWork::doubles(D, kRowThreads) * sizeof(double) + (size_t) D * sizeof(int);
    ScopedTimer tm(h.timing, st);
    launch(k_stc_rows, dim3(n), dim3(kRowThreads), lds, st, D, kStcMaxItns, h.d_Ginv.p, h.d_gamma.p, h.d_A.p, h.d_Ai.p, h.d_flag.p);
    h.ms[3] = tm.stop();
  }
  std::vector<double> Anew((size_t) n * ms), Ainew((size_t) n * ms);
  DSR_HIP(hipMemcpyAsync(Anew.data(), h.d_A.p, Anew.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipMemcpyAsync(Ainew.data(), h.d_Ai.p, Ainew.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipMemcpyAsync(flag.data(), h.d_flag.p, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  int bad = -1, nBad = 0;
  for (int k = 0; k < n; k++) {
    const int e = estX[k];
    if (flag[k]) { h.status[e] = DSR_E_CONSISTENCY; if (bad < 0) bad = e; nBad++; continue; }      // keeps its matrix, _stcInv and E
    h.status[e] = 0; h.E[e] = E[k];
    double* A = h.A.data() + (size_t) e * ms; double* Ai = h.Ainv.data() + (size_t) e * ms;
    const double* B = Anew.data() + (size_t) k * ms; const double* Bi = Ainew.data() + (size_t) k * ms;
    if (!h.cascade) { std::copy(B, B + ms, A); std::copy(Bi, Bi + ms, Ai); continue; }
    // eA:2298-2307: the new matrix left-multiplies the old; (B A)^-1 = A^-1 B^-1
    std::vector<double> P(ms), Pi(ms);
    for (int i = 0; i < D; i++) for (int j = 0; j < D; j++) {
      double s = 0.0, t = 0.0;
      for (int c = 0; c < D; c++) { s += B[(size_t) i * D + c] * A[(size_t) c * D + j]; t += Ai[(size_t) i * D + c] * Bi[(size_t) c * D + j]; }
      P[(size_t) i * D + j] = s; Pi[(size_t) i * D + j] = t;
    }
    std::copy(P.begin(), P.end(), A); std::copy(Pi.begin(), Pi.end(), Ai);
  }
  h.aDirty = true;
  if (nBad) throw Error(DSR_E_CONSISTENCY, "statistics of %d estimator(s), the first %d, are not finite, too few or badly conditioned; they are unchanged", nBad, bad);
}

// LDAEstimator::estimate (eA:2752-2836) for n estimators at once
void lda_estimate(LdaHandle& h, const int* estX, int n, hipStream_t st)
{
  const int D = h.D;
  if (n < 0) throw Error(DSR_E_PARAMETER, "negative count");
  if (n == 0) return;
  if (!estX) throw Error(DSR_E_PARAMETER, "null argument");
  if (!h.g) throw Error(DSR_E_CONSISTENCY, "LDAEstimator::estimate: a transformer without a distribution set has no statistics");
  for (int k = 0; k < n; k++) {
    h.check_est(estX[k], "LDAEstimator::estimate");
    for (int l = 0; l < k; l++) if (estX[l] == estX[k]) throw Error(DSR_E_PARAMETER, "estimator %d is named twice in one estimate", estX[k]);
  }
  const size_t ms = h.msz();
  std::vector<double> W((size_t) n * ms), B((size_t) n * ms);
  for (int k = 0; k < n; k++) {
    const int e = estX[k]; const double cnt = h.count[e];
    double* M[3] = { h.within.data() + (size_t) e * ms, h.between.data() + (size_t) e * ms, h.mixture.data() + (size_t) e * ms };
    for (int mat = 0; mat < 3; mat++) {
      for (size_t i = 0; i < ms; i++) M[mat][i] = M[mat][i] / cnt;                                // scaleScatterMatrices, eA:2921-2932: in place, every call
      for (int i = 0; i < D; i++) for (int j = i + 1; j < D; j++) M[mat][(size_t) i * D + j] = M[mat][(size_t) j * D + i];      // within() / between() copy the triangle up
    }
    std::copy(M[0], M[0] + ms, W.begin() + (size_t) k * ms); std::copy(M[1], M[1] + ms, B.begin() + (size_t) k * ms);
  }
  h.d_W.upload(W, st); h.d_B.upload(B, st); h.d_L.reserve((size_t) n * ms); h.d_ev.reserve((size_t) n * 2 * D); h.d_flag.reserve((size_t) n);
  DSR_HIP(hipMemsetAsync(h.d_flag.p, 0, (size_t) n * sizeof(int), st));
  {
    const size_t lds = ((size_t) 3 * D * D + 2 * D + ((D + 1) & ~1) + 2 * kRowThreads) * sizeof(double) + (size_t) D * sizeof(int);
    ScopedTimer tm(h.timing, st);
    launch(k_lda_solve, dim3(n), dim3(kRowThreads), lds, st, D, h.d_W.p, h.d_B.p, h.d_L.p, h.d_ev.p, h.d_flag.p);
    h.ms[2] = tm.stop();
  }
  std::vector<double> L((size_t) n * ms), ev((size_t) n * 2 * D); std::vector<int> flag(n);
  DSR_HIP(hipMemcpyAsync(L.data(), h.d_L.p, L.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipMemcpyAsync(ev.data(), h.d_ev.p, ev.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipMemcpyAsync(flag.data(), h.d_flag.p, (size_t) n * sizeof(int), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  int bad = -1, nBad = 0;
  for (int k = 0; k < n; k++) {
    const int e = estX[k];
    if (flag[k]) { h.status[e] = DSR_E_CONSISTENCY; if (bad < 0) bad = e; nBad++; continue; }
    h.status[e] = 0;
    std::copy(L.begin() + (size_t) k * ms, L.begin() + (size_t) (k + 1) * ms, h.L.begin() + (size_t) e * ms);
    std::copy(ev.begin() + (size_t) k * 2 * D, ev.begin() + (size_t) (k + 1) * 2 * D, h.ev.begin() + (size_t) e * 2 * D);
  }
  h.lDirty = true;
  if (nBad) throw Error(DSR_E_CONSISTENCY, "statistics of %d estimator(s), the first %d, are not finite; their matrices are unchanged", nBad, bad);
}

static void apply_matrix(XfBase& h, const double* M, int Din, int outDim, const float* x, long N, float* out, hipStream_t st)
{
  if (N < 0) throw Error(DSR_E_PARAMETER, "negative frame count");
  if (N == 0) return;
  if (!x || !out) throw Error(DSR_E_PARAMETER, "null argument");
  if ((long) N * outDim > 0x7fffffffL * 256L) throw Error(DSR_E_DIMENSION, "%ld frames in one call", N);
  ScopedTimer tm(h.timing, st);
  launch(k_stc_apply, dim3(cdiv(N * outDim, 256)), dim3(256), 0, st, Din, outDim, N, x, M, out);
  h.ms[4] = tm.stop();
}

void stc_apply(StcHandle& h, const float* x, long N, int estX, float* out, hipStream_t st)
{
  h.check_est(estX, "STCTransformer");
  if (h.aDirty) { require_device(); h.d_Aall.upload(h.A, st); h.aDirty = false; }
  apply_matrix(h, h.d_Aall.p + (size_t) estX * h.msz(), h.D, h.D, x, N, out, st);
}

void lda_apply(LdaHandle& h, const float* x, long N, int estX, int outDim, float* out, hipStream_t st)
{
  h.check_est(estX, "LDATransformer");
  if (outDim < 1 || outDim > h.D) throw Error(DSR_E_DIMENSION, "LDA output size %d of a %d-dimensional source", outDim, h.D);
  if (h.lDirty) { require_device(); h.d_Lall.upload(h.L, st); h.lDirty = false; }
  apply_matrix(h, h.d_Lall.p + (size_t) estX * h.msz(), h.D, outDim, x, N, out, st);
}

}  // namespace dsr

using namespace dsr;

namespace {

// one distribution per frame of a path (eA:2269-2283, 2765-2787): _dss->find() of an unknown name throws there
template <class H, class F> double run_path(H& h, const int32_t* distIds, int64_t pathLen, int64_t T, int estX, float factor, const char* who, F accumulate)
{
  if (pathLen > 0 && !distIds) throw Error(DSR_E_PARAMETER, "null argument");
  if (pathLen < 0 || pathLen > 0x7fffffffL) throw Error(DSR_E_PARAMETER, "bad path length");
  h.check_est(estX, who);
  if (pathLen > T) throw Error(DSR_E_INDEX, "%s: a path of %ld distributions over %ld frames", who, (long) pathLen, (long) T);
  std::vector<int> frame((size_t) pathLen), dist((size_t) pathLen), est((size_t) pathLen, estX); std::vector<float> fac((size_t) pathLen, factor), score((size_t) pathLen);
  for (long i = 0; i < pathLen; i++) {
    if (distIds[i] < 0) throw Error(DSR_E_INDEX, "%s: entry %ld of the path names no distribution of the set", who, i);
    frame[i] = (int) i; dist[i] = distIds[i];
  }
  accumulate(frame.data(), dist.data(), fac.data(), est.data(), (long) pathLen, score.data());
  double total = 0.0;
  for (long i = 0; i < pathLen; i++) total += score[i];
  return total;
}

}  // namespace

extern "C" {

static void stc_init(dsr_stc* h, dsr_gmm* g, int D, int nEst, int cascade, int mmiEstimation)
{
  h->g = g; h->D = D; h->G = g ? g->G : 0; h->K = g ? g->K : 0; h->nEst = nEst; h->cascade = cascade != 0; h->mmi = mmiEstimation != 0;
  h->count.assign(nEst, 0.0); h->denCount.assign(nEst, 0.0); h->totalPr.assign(nEst, 0.0); h->E.assign(nEst, 0.0); h->totalT.assign(nEst, 0u);
  h->A.assign((size_t) nEst * h->msz(), 0.0); h->Ainv.assign((size_t) nEst * h->msz(), 0.0); h->status.assign(nEst, 0);
  for (int e = 0; e < nEst; e++) for (int i = 0; i < D; i++) { h->A[(size_t) e * h->msz() + (size_t) i * D + i] = 1.0; h->Ainv[(size_t) e * h->msz() + (size_t) i * D + i] = 1.0; }      // _identity, eA:2254-2263
  if (!g) return;
  h->sumOsq.assign((size_t) nEst * h->ssz(), 0.0); h->regSq.assign((size_t) nEst * h->ssz(), 0.0);
  const int P = D * (D + 1) / 2; h->PZ = (P + 15) & ~15; h->NCp = (h->PZ + D + 15) & ~15;
  std::vector<int> pq(h->NCp, -1);
  { int col = 0; for (int i = 0; i < D; i++) for (int j = 0; j <= i; j++) pq[col++] = i | (j << 16); for (int c = 0; c < D; c++) pq[h->PZ + c] = c; }
  h->d_pq.upload(pq); h->d_mean.upload(g->mean); h->d_ivar.upload(g->ivar);
}

dsr_status dsr_stc_create(dsr_gmm* g, int nEst, int cascade, int mmiEstimation, dsr_stc** out)
{
  return guard([&] {
    if (!g || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (nEst < 1 || nEst > 65535) throw Error(DSR_E_PARAMETER, "%d estimators", nEst);
    if (g->D > kStcMaxD) throw Error(DSR_E_DIMENSION, "dimN = %d: STC estimation is built for dimN <= %d", g->D, kStcMaxD);
    if (g->D < 1 || g->K < 1) throw Error(DSR_E_DIMENSION, "empty model");
    require_device();
    std::unique_ptr<dsr_stc> h(new dsr_stc()); stc_init(h.get(), g, g->D, nEst, cascade, mmiEstimation);
    *out = h.release();
  });
}
// STCTransformer alone (tr:1790-1796): one matrix of dimN x dimN, the identity; nothing to accumulate or estimate
dsr_status dsr_stc_create_transformer(int dimN, dsr_stc** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (dimN < 1 || dimN > 4096) throw Error(DSR_E_DIMENSION, "dimN = %d", dimN);
    std::unique_ptr<dsr_stc> h(new dsr_stc()); stc_init(h.get(), nullptr, dimN, 1, 0, 0);
    *out = h.release();
  });
}
void dsr_stc_destroy(dsr_stc* h) { delete h; }

dsr_status dsr_stc_accumulate(dsr_stc* h, const float* xScore_dev, const float* xSrc_dev, int64_t N, const int32_t* frame, const int32_t* dist, const float* factor,
                              const int32_t* est, int64_t M, int32_t* nearest, float* score, void* stream)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    stc_accumulate(*h, xScore_dev, xSrc_dev, (long) N, frame, dist, factor, est, (long) M, nearest, score, (hipStream_t) stream);
  });
}

dsr_status dsr_stc_accumulate_path(dsr_stc* h, const float* xScore_dev, const float* xSrc_dev, int64_t T, const int32_t* distIds, int64_t pathLen, int estX,
                                   float factor, unsigned* framesN, void* stream)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    const double totalPr = run_path(*h, distIds, pathLen, T, estX, factor, "STCEstimator::accumulate",
      [&](const int* fr, const int* ds, const float* fa, const int* es, long M, float* sc) { stc_accumulate(*h, xScore_dev, xSrc_dev, (long) T, fr, ds, fa, es, M, nullptr, sc, (hipStream_t) stream); });
    if (factor > 0.0f) { h->totalPr[estX] += totalPr; h->totalT[estX] += (unsigned) pathLen; }   // eA:2284-2287
    else h->totalPr[estX] += -totalPr;
    if (framesN) *framesN = (unsigned) pathLen;
  });
}

dsr_status dsr_stc_estimate(dsr_stc* h, const int32_t* estX, int n, double minE, double multE, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); stc_estimate(*h, estX, n, minE, multE, (hipStream_t) stream); }); }

dsr_status dsr_stc_apply(dsr_stc* h, const float* x_dev, int64_t N, int estX, float* out_dev, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); stc_apply(*h, x_dev, (long) N, estX, out_dev, (hipStream_t) stream); }); }

static void lda_init(dsr_lda* h, dsr_gmm* g, dsr_gmm* global, int D, int nEst)
{
  h->g = g; h->D = D; h->G = g ? g->G : 0; h->K = g ? g->K : 0; h->nEst = nEst;
  h->count.assign(nEst, 0.0); h->status.assign(nEst, 0); h->ev.assign((size_t) nEst * 2 * D, 0.0);
  h->L.assign((size_t) nEst * h->msz(), 0.0);
  for (int e = 0; e < nEst; e++) for (int i = 0; i < D; i++) h->L[(size_t) e * h->msz() + (size_t) i * D + i] = 1.0;      // TransformMatrix::_initialize
  if (!g) return;
  h->globalRefN = global->refN[0]; h->mu0.assign(global->mean.begin(), global->mean.begin() + D);
  // the reference's Accu never calls zero() in its constructor and starts from unset memory (eA:2877-2894); here it starts from zero
  h->within.assign((size_t) nEst * h->msz(), 0.0); h->between.assign((size_t) nEst * h->msz(), 0.0); h->mixture.assign((size_t) nEst * h->msz(), 0.0);
  h->d_mean.upload(g->mean); h->d_mu0.upload(h->mu0);
}

dsr_status dsr_lda_create(dsr_gmm* g, dsr_gmm* global, int nEst, dsr_lda** out)
{
  return guard([&] {
    if (!g || !global || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (nEst < 1 || nEst > 65535) throw Error(DSR_E_PARAMETER, "%d estimators", nEst);
    if (g->D > kStcMaxD) throw Error(DSR_E_DIMENSION, "dimN = %d: LDA estimation is built for dimN <= %d", g->D, kStcMaxD);
    if (g->D < 1 || g->K < 1 || global->K < 1 || global->G < 1) throw Error(DSR_E_DIMENSION, "empty model");
    if (global->D != g->D) throw Error(DSR_E_DIMENSION, "Feature lengths (%d vs. %d) do not match.", global->D, g->D);
    require_device();
    std::unique_ptr<dsr_lda> h(new dsr_lda()); lda_init(h.get(), g, global, g->D, nEst);
    *out = h.release();
  });
}
// LDATransformer alone (tr:1884-1897): one matrix of dimN x dimN over a source of dimN, the identity
dsr_status dsr_lda_create_transformer(int dimN, dsr_lda** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (dimN < 1 || dimN > 4096) throw Error(DSR_E_DIMENSION, "dimN = %d", dimN);
    std::unique_ptr<dsr_lda> h(new dsr_lda()); lda_init(h.get(), nullptr, nullptr, dimN, 1);
    *out = h.release();
  });
}
void dsr_lda_destroy(dsr_lda* h) { delete h; }

dsr_status dsr_lda_accumulate(dsr_lda* h, const float* xScore_dev, const float* xSrc_dev, int64_t N, const int32_t* frame, const int32_t* dist, const float* factor,
                              const int32_t* est, int64_t M, int32_t* nearest, float* score, void* stream)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    lda_accumulate(*h, xScore_dev, xSrc_dev, (long) N, frame, dist, factor, est, (long) M, nearest, score, (hipStream_t) stream);
  });
}

dsr_status dsr_lda_accumulate_path(dsr_lda* h, const float* xScore_dev, const float* xSrc_dev, int64_t T, const int32_t* distIds, int64_t pathLen, int estX,
                                   float factor, double* score, void* stream)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    const double total = run_path(*h, distIds, pathLen, T, estX, factor, "LDAEstimator::accumulate",
      [&](const int* fr, const int* ds, const float* fa, const int* es, long M, float* sc) { lda_accumulate(*h, xScore_dev, xSrc_dev, (long) T, fr, ds, fa, es, M, nullptr, sc, (hipStream_t) stream); });
    if (score) *score = total;                            // eA:2783, 2789
  });
}

dsr_status dsr_lda_estimate(dsr_lda* h, const int32_t* estX, int n, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); lda_estimate(*h, estX, n, (hipStream_t) stream); }); }

dsr_status dsr_lda_apply(dsr_lda* h, const float* x_dev, int64_t N, int estX, int outDim, float* out_dev, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); lda_apply(*h, x_dev, (long) N, estX, outDim, out_dev, (hipStream_t) stream); }); }

}  // extern "C"
