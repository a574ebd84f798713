// csrc/k_train.hip -- forward-backward statistics of GMM training on the device.
//
// Replaces DistribTrain::accumulate (asr/train/distribTrain.cc:74-80) -> CodebookTrain::accumulate (asr/train/codebookTrain.cc:90-112) ->
// CodebookBasic::_scoreAll (asr/gaussian/codebookBasic.cc:645-766), CodebookTrain::Accu::accumulate (codebookTrain.cc:520-540, 354-358) and
// DistribTrain::Accu::accumulate (distribTrain.cc:133-142) for batches of (frame, distribution, factor) items, and the drivers
// DistribSetTrain::accumulate / accumulateLattice (distribTrain.cc:515-561).
//
//   k_train_post    thread per item: the _scoreAll chain and the normalisation in the reference's order and precision (the distance loop is
//                   k_gmm_all's, so logdist has the same bits), gamma[item][r] = float(posterior * factor), the float score, a flag for a
//                   NaN score or a posterior sum that is zero / not finite.
//   k_train_acc     items sorted by codebook (stable counting sort on the host); one workgroup per (codebook, chunk of kChunk items) forms
//                   Gamma^T [X | X o X | 1(factor > 0) | 1(factor <= 0)] -- sumO, sumOsq, count and -denCount in one contraction of 2 dimN + 2
//                   columns on v_mfma_f64_16x16x4_f64.  The operands are the float gamma and x widened to fp64 (x x is exact in fp64).
//   k_train_reduce  workgroup per codebook: the chunk partials are summed in chunk order and added to the accumulator rows, unless the flag
//                   is set.  No floating-point atomics anywhere: the same call twice gives the same bits.
// This translation unit is compiled with -ffp-contract=off.
#include "launch.h"
#include "train.h"
#include "lattice.h"
#include "mfma64.h"
#include <cmath>

namespace dsr {

static constexpr int kChunk = 256;                        // items per workgroup of k_train_acc

__global__ __launch_bounds__(256) void k_train_post(const float* __restrict__ x, int D, int DP, const int* __restrict__ off,
                                                    const float* __restrict__ mean, const float* __restrict__ ivar, const float* __restrict__ cst,
                                                    const float* __restrict__ val, const float* __restrict__ scale, const int* __restrict__ sFrame,
                                                    const int* __restrict__ sDist, const float* __restrict__ sFactor, const int* __restrict__ start,
                                                    const long long* __restrict__ gbase, long M, float* __restrict__ gamma, float* __restrict__ score,
                                                    int* __restrict__ flag)
{
  const long i = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= M) return;
  const int k = sDist[i]; const float f = sFactor[i];
  const float* xp = x + (long) sFrame[i] * D;
  const int a = off[k], R = off[k + 1] - a; const float sc = scale[k];
  float* gr = gamma + gbase[k] + (i - start[k]) * R;     // this item's row: logdist, then mixVal, then gamma
  double minlog = 1E20;
  for (int r = 0; r < R; r++) {
    const int g = a + r;
    double dist = (double) cst[g];
    for (int d = 0; d < D; d++) { const double diff = (double) __fsub_rn(mean[(long) g * DP + d], xp[d]); dist = __dadd_rn(dist, __dmul_rn(__dmul_rn(diff, diff), (double) ivar[(long) g * DP + d])); }
    const float ld = (float) (0.5 * dist);
    gr[r] = ld;
    if ((double) ld < minlog) minlog = (double) ld;
  }
  float res; double s;
  if (R == 1) {                                           // codebookBasic.cc:742-747
    res = __fmul_rn(sc, __fadd_rn(gr[0], val[a])); gr[0] = 1.0f; s = 1.0;
  } else {
    s = 0.0;
    for (int r = 0; r < R; r++) {                          // :756-762: the sum is over the float mixVal
      const double e = __dmul_rn((double) sc, __dsub_rn(minlog, (double) gr[r]));
      float mv = 0.0f;
      if (e > -100.0) { mv = (float) exp(__dsub_rn(e, (double) __fmul_rn(sc, val[a + r]))); s = __dadd_rn(s, (double) mv); }
      gr[r] = mv;
    }
    res = (float) __dsub_rn(__dmul_rn((double) sc, minlog), log(s));
  }
  if (res != res || !(s > 0.0) || s > 1.7E308) *flag = 1;
  for (int r = 0; r < R; r++) gr[r] = __fmul_rn((float) ((double) gr[r] / s), f);     // codebookTrain.cc:100-105, :523
  score[i] = res;
}

// chunk[4 c] = { codebook, first sorted item, items, offset of the chunk's partial [R][2 D + 2] }
__global__ __launch_bounds__(256) void k_train_acc(const float* __restrict__ x, int D, const int* __restrict__ off, const int* __restrict__ sFrame,
                                                   const float* __restrict__ sFactor, const int* __restrict__ start, const long long* __restrict__ gbase,
                                                   const long long* __restrict__ chunk, const float* __restrict__ gamma, double* __restrict__ part)
{
  __shared__ int sfr[kChunk]; __shared__ float sfa[kChunk];
  const long long* ch = chunk + 4 * (long) blockIdx.x;
  const int k = (int) ch[0], i0 = (int) ch[1], n = (int) ch[2];
  const int R = off[k + 1] - off[k], NC = 2 * D + 2, RT = (R + 15) >> 4, CT = (NC + 15) >> 4;
  const float* gr = gamma + gbase[k] + (long) (i0 - start[k]) * R;
  double* out = part + ch[3];
  for (int j = threadIdx.x; j < n; j += blockDim.x) { sfr[j] = sFrame[i0 + j]; sfa[j] = sFactor[i0 + j]; }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lo = lane & 15, hi = lane >> 4;
  for (int tile = wave; tile < RT * CT; tile += 4) {       // uniform per wave
    const int rt = tile / CT, ct = tile - rt * CT;
    const int row = rt * 16 + lo, col = ct * 16 + lo;      // A: Gaussian `row` of item 4 ks + hi; B: column `col` of the same item
    const bool rowOk = row < R, colOk = col < NC;
    const int d = col < D ? col : col - D;
    d4 c = {0.0, 0.0, 0.0, 0.0};
    for (int j0 = 0; j0 < n; j0 += 16) {                   // four k-steps' loads in flight before the MFMAs that need them
      double av[4], bv[4];
#pragma unroll
      for (int s = 0; s < 4; s++) {
        const int j = j0 + 4 * s + hi;
        av[s] = 0.0; bv[s] = 0.0;
        if (j < n) {
          if (rowOk) av[s] = (double) gr[(long) j * R + row];
          if (colOk) {
            if (col < 2 * D) { const double xv = (double) x[(long) sfr[j] * D + d]; bv[s] = col < D ? xv : xv * xv; }
            else bv[s] = ((col == 2 * D) == (sfa[j] > 0.0f)) ? 1.0 : 0.0;
          }
        }
      }
#pragma unroll
      for (int s = 0; s < 4; s++) c = mfma64(av[s], bv[s], c);
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int orow = rt * 16 + hi + 4 * q;
      if (orow < R && colOk) out[(long) orow * NC + col] = c[q];
    }
  }
}

__global__ __launch_bounds__(256) void k_train_reduce(int D, const int* __restrict__ off, const int* __restrict__ cstart, const long long* __restrict__ pbase,
                                                      const double* __restrict__ part, const int* __restrict__ flag, double* __restrict__ acc)
{
  if (*flag) return;
  const int k = blockIdx.x, c0 = cstart[k], c1 = cstart[k + 1];
  if (c0 == c1) return;
  const int a = off[k], R = off[k + 1] - a, NC = 2 * D + 2, NA = 2 * D + 4;
  const double* p = part + pbase[k];
  for (int e = threadIdx.x; e < R * NC; e += blockDim.x) {
    double s = 0.0;
    for (int c = 0; c < c1 - c0; c++) s = __dadd_rn(s, p[(long) c * R * NC + e]);
    const int r = e / NC, col = e - r * NC;
    double* row = acc + (long) (a + r) * NA;
    if (col < 2 * D) row[col] = __dadd_rn(row[col], s);
    else if (col == 2 * D) { row[2 * D] = __dadd_rn(row[2 * D], s); row[2 * D + 2] = __dadd_rn(row[2 * D + 2], s); }          // count: codebook, distribution
    else { row[2 * D + 1] = __dsub_rn(row[2 * D + 1], s); row[2 * D + 3] = __dsub_rn(row[2 * D + 3], s); }                    // denCount -= gamma
  }
}

void TrainAccu::resize()
{
  D = g->D; G = g->G; NA = 2 * D + 4;
  h.assign((size_t) G * NA, 0.0); push();
}
void TrainAccu::pull()
{
  h.resize((size_t) G * NA);
  DSR_HIP(hipDeviceSynchronize());
  if (G) DSR_HIP(hipMemcpy(h.data(), d_acc.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
}
void TrainAccu::push() { d_acc.upload(h); }

void train_accumulate(TrainAccu& t, const float* x, long N, const int* frame, const int* dist, const float* factor, long M, float* score, hipStream_t st)
{
  GmmModel& m = *t.g;
  if (M < 0 || N < 0) throw Error(DSR_E_PARAMETER, "negative size");
  if (M == 0) return;
  if (!x || !frame || !dist || !factor) throw Error(DSR_E_PARAMETER, "null argument");
  if (M > 0x7fffffffL - kChunk) throw Error(DSR_E_DIMENSION, "%ld items in one call (at most 2^31 - 257)", M);
  if (t.G != m.G || t.D != m.D) throw Error(DSR_E_CONSISTENCY, "the model changed under the training handle");
  const int K = m.K;
  std::vector<int> start(K + 1, 0);
  for (long i = 0; i < M; i++) {
    if (frame[i] < 0 || frame[i] >= N) throw Error(DSR_E_INDEX, "item %ld: frame %d of %ld", i, frame[i], N);
    if (dist[i] < 0 || dist[i] >= K) throw Error(DSR_E_INDEX, "item %ld: distribution %d of %d", i, dist[i], K);
    if (!std::isfinite(factor[i])) throw Error(DSR_E_PARAMETER, "item %ld: factor is not finite", i);
    start[dist[i] + 1]++;
  }
  for (int k = 0; k < K; k++) start[k + 1] += start[k];
  // stable counting sort by distribution (= codebook) id
  std::vector<int> perm(M), sFrame(M), sDist(M), pos(start.begin(), start.end() - 1); std::vector<float> sFactor(M);
  for (long i = 0; i < M; i++) { const int p = pos[dist[i]]++; perm[p] = (int) i; sFrame[p] = frame[i]; sDist[p] = dist[i]; sFactor[p] = factor[i]; }
  std::vector<long long> gbase(K), pbase(K), chunk; std::vector<int> cstart(K + 1, 0);
  long long gtot = 0, ptot = 0;
  for (int k = 0; k < K; k++) {
    const int cnt = start[k + 1] - start[k], R = m.refN[k]; const long long psz = (long long) R * (2 * m.D + 2);
    gbase[k] = gtot; gtot += (long long) cnt * R; pbase[k] = ptot;
    for (int i0 = 0; i0 < cnt; i0 += kChunk) {
      chunk.push_back(k); chunk.push_back(start[k] + i0); chunk.push_back(cnt - i0 < kChunk ? cnt - i0 : kChunk); chunk.push_back(ptot); ptot += psz;
    }
    cstart[k + 1] = (int) (chunk.size() / 4);
  }
  const int nChunks = cstart[K];
  t.d_frame.upload(sFrame, st); t.d_dist.upload(sDist, st); t.d_factor.upload(sFactor, st); t.d_start.upload(start, st); t.d_gbase.upload(gbase, st);
  t.d_chunk.upload(chunk, st); t.d_cstart.upload(cstart, st); t.d_pbase.upload(pbase, st);
  t.d_gamma.reserve((size_t) gtot); t.d_part.reserve((size_t) ptot); t.d_score.reserve((size_t) M); t.d_flag.reserve(1);
  DSR_HIP(hipMemsetAsync(t.d_flag.p, 0, sizeof(int), st));
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (t.timing) { for (int i = 0; i < 3; i++) DSR_HIP(hipEventCreate(&ev[i])); DSR_HIP(hipEventRecord(ev[0], st)); }
  launch(k_train_post, dim3(cdiv(M, 256)), dim3(256), 0, st, x, m.D, m.Dp, m.d_off.p, m.d_mean.p, m.d_ivar.p, m.d_cst.p, m.d_val.p, m.d_scale.p,
                     t.d_frame.p, t.d_dist.p, t.d_factor.p, t.d_start.p, t.d_gbase.p, M, t.d_gamma.p, t.d_score.p, t.d_flag.p);
  if (t.timing) DSR_HIP(hipEventRecord(ev[1], st));
  launch(k_train_acc, dim3(nChunks), dim3(256), 0, st, x, m.D, m.d_off.p, t.d_frame.p, t.d_factor.p, t.d_start.p, t.d_gbase.p, t.d_chunk.p,
                     t.d_gamma.p, t.d_part.p);
  launch(k_train_reduce, dim3(K), dim3(256), 0, st, m.D, m.d_off.p, t.d_cstart.p, t.d_pbase.p, t.d_part.p, t.d_flag.p, t.d_acc.p);
  if (t.timing) DSR_HIP(hipEventRecord(ev[2], st));
  int flag = 0; std::vector<float> ss(score ? M : 0);
  DSR_HIP(hipMemcpyAsync(&flag, t.d_flag.p, sizeof(int), hipMemcpyDeviceToHost, st));
  if (score) DSR_HIP(hipMemcpyAsync(ss.data(), t.d_score.p, M * sizeof(float), hipMemcpyDeviceToHost, st));
  DSR_HIP(hipStreamSynchronize(st));
  if (t.timing) {
    DSR_HIP(hipEventElapsedTime(&t.ms[0], ev[0], ev[1])); DSR_HIP(hipEventElapsedTime(&t.ms[1], ev[1], ev[2]));
    for (int i = 0; i < 3; i++) (void) hipEventDestroy(ev[i]);
  }
  if (score) for (long p = 0; p < M; p++) score[perm[p]] = ss[p];
  if (flag) throw Error(DSR_E_NUMERIC, "Utterance log-likelihood is NaN");     // codebookTrain.cc:97-98; the accumulators are as before the call
}

}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_train_create(dsr_gmm* g, double massThreshold, dsr_train** out)
{
  return guard([&] {
    if (!g || !out) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    dsr_train* t = new dsr_train(); t->g = g; t->minCount = massThreshold;
    try { t->resize(); } catch (...) { delete t; throw; }
    *out = t;
  });
}
void dsr_train_destroy(dsr_train* t) { delete t; }
int dsr_train_num_gaussians(const dsr_train* t) { return t ? t->G : 0; }
dsr_status dsr_train_set_timing(dsr_train* t, int on) { return guard([&] { if (!t) throw Error(DSR_E_PARAMETER, "null argument"); t->timing = on != 0; }); }
dsr_status dsr_train_kernel_ms(const dsr_train* t, float ms[2])
{ return guard([&] { if (!t || !ms) throw Error(DSR_E_PARAMETER, "null argument"); ms[0] = t->ms[0]; ms[1] = t->ms[1]; }); }

dsr_status dsr_train_upload_features(dsr_train* t, const float* x_host, int64_t N, const float** x_dev)
{
  return guard([&] {
    if (!t || !x_dev || (N > 0 && !x_host)) throw Error(DSR_E_PARAMETER, "null argument");
    if (N < 0) throw Error(DSR_E_PARAMETER, "negative frame count");
    t->d_feat.upload(x_host, (size_t) N * t->g->D); *x_dev = t->d_feat.p;
  });
}

dsr_status dsr_train_accumulate(dsr_train* t, const float* x, int64_t N, const int32_t* frame, const int32_t* dist, const float* factor, int64_t M,
                                float* score, void* stream)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    train_accumulate(*t, x, (long) N, frame, dist, factor, (long) M, score, (hipStream_t) stream);
  });
}

dsr_status dsr_train_accumulate_path(dsr_train* t, const float* x, int64_t T, const int32_t* distIds, float factor, double* score, void* stream)
{
  return guard([&] {
    if (!t || (T > 0 && !distIds)) throw Error(DSR_E_PARAMETER, "null argument");
    if (T < 0 || T > 0x7fffffffL) throw Error(DSR_E_PARAMETER, "bad frame count");
    std::vector<int> frame((size_t) T); std::vector<float> fac((size_t) T, factor), sc((size_t) T);
    for (long i = 0; i < T; i++) frame[i] = (int) i;
    train_accumulate(*t, x, (long) T, frame.data(), distIds, fac.data(), (long) T, sc.data(), (hipStream_t) stream);
    double s = 0.0; for (long i = 0; i < T; i++) s += (double) sc[i];       // distribTrain.cc:519-521
    if (score) *score = s;
  });
}

dsr_status dsr_train_accumulate_lattice(dsr_train* t, dsr_lattice* L, const float* x, int64_t T, float factor, unsigned* linksN, void* stream)
{
  return guard([&] {
    if (!t || !L) throw Error(DSR_E_PARAMETER, "null argument");
    const size_t E = L->from.size(), nn = L->nodeFinal.size();
    std::vector<double> gamma(E); std::vector<int32_t> edgeLive(E), nodeLive(nn);
    const dsr_status s = dsr_lattice_get_state(L, gamma.data(), edgeLive.data(), nullptr, nodeLive.data(), nullptr, nullptr);
    if (s) throw Error(s, "%s", dsr_last_error());
    std::vector<int> frame, dist; std::vector<float> fac; unsigned cnt = 0;
    for (size_t e = 0; e < E; e++) {                        // the links Lattice::EdgeIterator sees, distribTrain.cc:532-559
      if (!edgeLive[e] || !nodeLive[L->from[e]]) continue;
      if (L->in[e] == 0) continue;
      if (gamma[e] > 10.0) continue;
      const float post = (float) ((double) factor * exp(-gamma[e]));
      if (L->in[e] - 1 >= (unsigned) t->g->K) throw Error(DSR_E_INDEX, "link %zu: distribution %u of %d", e, L->in[e] - 1, t->g->K);
      if (L->start[e] < 0 || L->end[e] >= T) throw Error(DSR_E_INDEX, "link %zu: frames %d..%d of %ld", e, L->start[e], L->end[e], (long) T);
      cnt++;
      for (int f = L->start[e]; f <= L->end[e]; f++) { frame.push_back(f); dist.push_back((int) L->in[e] - 1); fac.push_back(post); }
    }
    train_accumulate(*t, x, (long) T, frame.data(), dist.data(), fac.data(), (long) frame.size(), nullptr, (hipStream_t) stream);
    if (linksN) *linksN = cnt;
  });
}

}  // extern "C"
