// csrc/k_sad.hip -- speech activity detection, btk/sad/sad.{h,cc} (include/dsr.h section 7b): EnergyVADMetric, SimpleEnergyVAD,
// PowerSpectrumVADMetric / NormalizedEnergyMetric / TSPSVADMetric, CCCVADMetric, the hangover segmenters, and the spectral-shape operators
// of sadFeature.cc (EnergyDiffusion, BandEnergyRatio, NegativeEntropy, SignificantSubbands).
//
// Every metric keeps the reference's operation order and the float / double of every intermediate; the file is built without FMA contraction.
// Batch arrays are [U][Tmax][...] with an optional nframes_dev [U]; frames at or past an utterance's count are never read and come out zero.
// Carried state goes in and out as arrays: two calls that carry it equal one call.
//
//   k_frame_energy   a thread per frame: the serial fp64 sum of squares (float frames) or of |z|^2 (complex frames), i ascending.
//   k_energy_walk    one wavefront per utterance, frames in order.  `sum > sorted[k]` holds exactly when more than k history entries lie below
//                    `sum`, so nothing is sorted: the history is a ring in LDS (its order never matters), the lanes take every 64th entry,
//                    ballot + popcount count the entries below.  The hangover counters of the metric ride along in registers.
//   k_simple_walk    a thread per utterance: E <- gamma E + (1 - gamma) e, e / E > threshold.
//   k_band_power     a thread per (utterance, frame, channel): the fp64 band sum; k_power_decide a thread per frame over the channels in order.
//   k_ccc            one workgroup per frame walks the channels 1 .. C-1 in order on ONE LDS buffer of fftLen complex fp64 that is cleared once
//                    a frame (sad.cc:855), so a band-limited channel sees its predecessor's time-domain output outside the band, as there.
//                    The inverse transform is fft_lds.h's after an in-place bit reversal; the n-best pass keeps candidate i in lane i of wave 0
//                    and visits only the samples above the last candidate (ballot), in index order, with the reference's insertion rule.
//   k_hangover       a thread per utterance: the head / tail state machine of HangoverVADFeature::next over the metrics' decisions.
//   k_gather         the emitted frames, packed.
//   k_gg             the generalised-Gaussian metrics (negentropy, mutual information, likelihood ratio): a workgroup per utterance, a thread per
//                    bin, frames in chunks; the per-bin fp64 terms go through LDS to an ordered bin sum a frame.
//   k_shape          the four spectral-shape operators of sadFeature.cc, a thread per frame.
#include "launch.h"
#include "fft_lds.h"
#include <algorithm>
#include <cmath>

using namespace dsr;

namespace {

// (clampT of dev_math.h in the spelling these kernels were compiled with: the other one changes their instruction schedule)
__device__ __forceinline__ int clampT(const int* nf, int u, int Tmax) { if (!nf) return Tmax; const int t = nf[u]; return t < 0 ? 0 : (t > Tmax ? Tmax : t); }

// ---- EnergyVADMetric::_aboveThreshold (sad.cc:486-490) and SimpleEnergyVAD::next (sad.cc:184-186): the frame's energy
template <class T> __device__ __forceinline__ double sq(T v);
template <> __device__ __forceinline__ double sq<float>(float v) { const double d = v; return d * d; }
template <> __device__ __forceinline__ double sq<double2>(double2 v) { return v.x * v.x + v.y * v.y; }        // gsl_complex_abs2

template <class T>
__global__ __launch_bounds__(256) void k_frame_energy(const T* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int N, double* __restrict__ e)
{
  const size_t f = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t) U * Tmax) return;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { e[f] = 0.0; return; }
  const T* r = x + f * N;
  double sum = 0.0;
  for (int i = 0; i < N; i++) sum += sq<T>(r[i]);
  e[f] = sum;
}

// ---- EnergyVADMetric::next (sad.cc:484-554).  cnt[u] = (aboveThresholdN, belowThresholdN, recognizing, ring position)
__global__ __launch_bounds__(64) void k_energy_walk(const double* __restrict__ e, const int* __restrict__ nf, int Tmax, int N, unsigned medianIndex, unsigned headN,
                                                    unsigned tailN, double* __restrict__ hist, int* __restrict__ cnt, double* __restrict__ dec, int* __restrict__ updates)
{
  extern __shared__ double sad_h[];
  const int u = blockIdx.x, lane = threadIdx.x;
  const int T = clampT(nf, u, Tmax);
  double* hu = hist + (size_t) u * N;
  for (int i = lane; i < N; i += 64) sad_h[i] = hu[i];
  unsigned aboveN = (unsigned) cnt[4 * u], belowN = (unsigned) cnt[4 * u + 1];
  bool rec = cnt[4 * u + 2] != 0;
  int pos = cnt[4 * u + 3], upd = 0;
  if (pos < 0 || pos >= N) pos = 0;                                    // a state array that is not this metric's must not index past the ring
  __syncthreads();
  for (int t = 0; t < T; t++) {
    const double sum = e[(size_t) u * Tmax + t];
    unsigned below = 0;
    for (int base = 0; base < N; base += 64) {
      const int i = base + lane;
      below += (unsigned) __popcll(__ballot(i < N && sad_h[i] < sum));
    }
    __syncthreads();                                                   // every lane has read the history before this frame's entry replaces one
    if (!rec && aboveN == 0) {                                         // sad.cc:495, before this frame's counters change
      if (lane == 0) sad_h[pos] = sum;
      pos = pos + 1 == N ? 0 : pos + 1; upd++;
    }
    __syncthreads();
    const bool above = below > medianIndex;
    if (rec) {
      if (above) belowN = 0;
      else { belowN++; if (belowN == tailN) { rec = false; aboveN = 0; } }
    } else {
      if (above) { aboveN++; if (aboveN == headN) { rec = true; belowN = 0; } }
      else aboveN = 0;
    }
    if (lane == 0) dec[(size_t) u * Tmax + t] = above ? 1.0 : 0.0;
  }
  for (int t = T + lane; t < Tmax; t += 64) dec[(size_t) u * Tmax + t] = 0.0;
  for (int i = lane; i < N; i += 64) hu[i] = sad_h[i];
  if (lane == 0) { cnt[4 * u] = (int) aboveN; cnt[4 * u + 1] = (int) belowN; cnt[4 * u + 2] = rec ? 1 : 0; cnt[4 * u + 3] = pos; if (updates) updates[u] = upd; }
}

__global__ void k_energy_init(double* hist, int* cnt, int U, int N, double initial, int countersOnly)
{
  const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (!countersOnly && i < (size_t) U * N) hist[i] = initial;
  if (i < (size_t) U) { cnt[4 * i] = 0; cnt[4 * i + 1] = 0; cnt[4 * i + 2] = 0; if (!countersOnly) cnt[4 * i + 3] = 0; }
}

// ---- SimpleEnergyVAD::next (sad.cc:188-190)
__global__ __launch_bounds__(64) void k_simple_walk(const double* __restrict__ e, const int* __restrict__ nf, int U, int Tmax, double threshold, double gamma,
                                                    double* __restrict__ E, double* __restrict__ dec, double* __restrict__ score)
{
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= U) return;
  const int T = clampT(nf, u, Tmax);
  double se = E[u];
  for (int t = 0; t < Tmax; t++) {
    const size_t f = (size_t) u * Tmax + t;
    if (t >= T) { dec[f] = 0.0; score[f] = 0.0; continue; }
    const double cur = e[f];
    se = gamma * se + (1.0 - gamma) * cur;
    const double ratio = cur / se;
    score[f] = ratio; dec[f] = ratio > threshold ? 1.0 : 0.0;
  }
  E[u] = se;
}

// ---- the band power of PowerSpectrumVADMetric / NormalizedEnergyMetric / TSPSVADMetric (sad.cc:680-687): only bin 0 has weight 1
__global__ __launch_bounds__(256) void k_band_power(const float* __restrict__ P, const int* __restrict__ nf, int U, int C, int Tmax, int F, int lowX, int highX,
                                                    unsigned fftLen, double* __restrict__ pw)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tmax * C) return;
  const int c = (int) (idx % C), t = (int) ((idx / C) % Tmax), u = (int) (idx / ((size_t) C * Tmax));
  if (t >= clampT(nf, u, Tmax)) { pw[idx] = 0.0; return; }
  const float* r = P + (((size_t) u * C + c) * Tmax + t) * F;
  double p = 0.0;
  for (int b = lowX; b <= highX; b++) {
    if (b == 0) p += (double) r[b];
    else p += 2.0 * (double) r[b];
  }
  pw[idx] = p / (double) fftLen;
}

// kind 0: power ratio (sad.cc:697-702), 1: energy ratio (:771, :781-793), 2: TSPS (:1011-1021)
__global__ __launch_bounds__(256) void k_power_decide(const double* __restrict__ pw, const int* __restrict__ nf, int U, int C, int Tmax, int kind, double E0,
                                                      double* __restrict__ dec, double* __restrict__ score)
{
  const size_t f = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t) U * Tmax) return;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { dec[f] = 0.0; score[f] = 0.0; return; }
  const double* p = pw + f * C;
  double total = 0.0;
  for (int c = 0; c < C; c++) total += kind == 1 ? sqrt(p[c]) : p[c];
  double s; bool speech;
  if (kind == 0)      { s = p[0] / total; speech = s > E0 / (double) (unsigned) C; }
  else if (kind == 1) { s = sqrt(p[0]) / total; speech = s > E0 / (double) (unsigned) C; }
  else                { const double tgt = p[0]; s = log(tgt / (total - tgt)) - log(E0 / total); speech = s > 0; }
  score[f] = s; dec[f] = speech ? 1.0 : -1.0;
}

// ---- CCCVADMetric::next (sad.cc:842-941)
__device__ __forceinline__ double lane_d(double v, int l) { return __shfl(v, l, 64); }

template <class CT>
__global__ void k_ccc(const CT* __restrict__ X, const int* __restrict__ nf, int U, int C, int Tmax, int N, int logN, int lowX, int highX, int nCand, double threshold,
                      double* __restrict__ dec, double* __restrict__ score, double* __restrict__ cands, int nbest)
{
  extern __shared__ double ccc_lds[];
  double* re = ccc_lds; double* im = re + N; double* twr = im + N; double* twi = twr + fft_tw_entries(N);
  const int f = blockIdx.x, u = f / Tmax, t = f % Tmax, tid = threadIdx.x, nth = blockDim.x;
  if (t >= clampT(nf, u, Tmax)) {                                                                 // uniform for the workgroup
    if (tid == 0) { dec[f] = 0.0; score[f] = 0.0; }
    if (cands && tid < nCand) cands[(size_t) f * nCand + tid] = 0.0;
    return;
  }
  fft_tw_init(twr, twi, N);
  for (int k = tid; k < N; k += nth) { re[k] = 0.0; im[k] = 0.0; }                                // once a frame, not once a channel (sad.cc:855)
  const CT* ref = X + (((size_t) u * C) * Tmax + t) * N;
  double total = 0.0;
  for (int c = 1; c < C; c++) {
    const CT* ch = X + (((size_t) u * C + c) * Tmax + t) * N;
    __syncthreads();
    for (int b = lowX + tid; b <= highX; b += nth) {
      const double x1 = ref[b].x, y1 = -(double) ref[b].y, x2 = ch[b].x, y2 = ch[b].y;            // conj(val1) * val2, gsl_complex_mul
      const double cr = x1 * x2 - y1 * y2, ci = x1 * y2 + y1 * x2;
      const double a = hypot(cr, ci);
      const double pr = cr / a, pi = ci / a;
      if (2 * b == N) { re[b] = pr; im[b] = -pi; }                                                // the mirror of N/2 is N/2, written second
      else { re[b] = pr; im[b] = pi; if (b > 0) { re[N - b] = pr; im[N - b] = -pi; } }
    }
    __syncthreads();
    for (int k = tid; k < N; k += nth) {                                                          // in place into bit-reversed order
      const int j = brev(k, logN);
      if (k < j) { const double a = re[k], b = im[k]; re[k] = re[j]; im[k] = im[j]; re[j] = a; im[j] = b; }
    }
    fft_run(re, im, twr, twi, N, 1.0);
    const double norm = 1.0 / (double) (unsigned) N;
    for (int k = tid; k < N; k += nth) { re[k] *= norm; im[k] *= norm; }
    __syncthreads();
    if (!nbest) { if (tid == 0) total += re[0]; }                                                 // the timing variant: transforms only
    else if (tid < 64) {                                                                          // wave 0: candidate i lives in lane i
      const int lane = tid;
      double cand = lane == 0 ? re[0] : -1e10;
      for (int base = 0; base < N; base += 64) {
        const int k = base + lane;
        const double v = (k >= 1 && k < N) ? re[k] : 0.0;
        int done = -1;
        while (true) {
          const double last = lane_d(cand, nCand - 1);
          const unsigned long long m = __ballot(k >= 1 && k < N && lane > done && v > last);
          if (!m) break;
          const int first = __ffsll((long long) m) - 1;
          const double cc = lane_d(v, first), top = lane_d(cand, 0);
          if (cc > top) { const double up = __shfl_up(cand, 1, 64); if (lane > 0) cand = up; }   // shifted only if it also exceeds slot 0 ...
          if (lane == 0) cand = cc;                                                               // ... but always stored there (sad.cc:898-900)
          done = first;
        }
      }
      double m = 0.0;
      for (int i = 0; i < nCand; i++) m += lane_d(cand, i);
      m /= (double) (unsigned) nCand;
      total += m;
      if (cands && c == C - 1 && lane < nCand) cands[(size_t) f * nCand + lane] = cand;           // _ccList as the last channel leaves it
    }
  }
  if (tid == 0) {
    total = total / (double) (unsigned) (C - 1);
    score[f] = total; dec[f] = total < threshold ? 1.0 : -1.0;
  }
}

// ---- HangoverVADFeature::next (sad.cc:1767-1837) with the decision logic of the three classes (:1756-1765, :1853-1879, :1904-1945)
struct HangArgs { double thr[8]; };

__device__ __forceinline__ bool hang_above(const double* __restrict__ dec, size_t plane, size_t f, int K, int kind, const HangArgs& a, int& code)
{
  if (kind == 0) return dec[f] > a.thr[0];
  if (kind == 2 && K < 3) return false;                                // sad.cc:1906-1909
  if (dec[f] < 0.5) { code = -1; return false; }
  if (kind == 1) {
    if (dec[plane + f] < 0.5) { code = 2; return true; }
    if (dec[2 * plane + f] > 0.5) { code = 3; return true; }
    code = -3; return false;
  }
  for (int s = 1; s < K; s++) if (dec[s * plane + f] > 0.5) { code = s + 1; return true; }
  code = -K; return false;
}

__global__ __launch_bounds__(64) void k_hangover(const double* __restrict__ dec, const int* __restrict__ nf, int K, int U, int Tmax, int kind, HangArgs a, unsigned headN,
                                                 unsigned tailN, int* __restrict__ start, int* __restrict__ length, int* __restrict__ consumed, int* __restrict__ dm)
{
  const int u = blockIdx.x * 64 + threadIdx.x;
  if (u >= U) return;
  const int T = clampT(nf, u, Tmax);
  const size_t plane = (size_t) U * Tmax, row = (size_t) u * Tmax;
  unsigned aboveN = 0, belowN = 0;
  int code = 0, s = 0, len = 0, st = 0;
  bool rec = false, ended = false;
  for (; s < T && !ended; s++) {
    const bool above = hang_above(dec, plane, row + s, K, kind, a, code);
    dm[row + s] = code;
    if (!rec) {
      if (above) { aboveN++; if (aboveN == headN) { rec = true; st = s + 1 - (int) headN; len = (int) headN; } }
      else aboveN = 0;
    } else {
      if (above) belowN = 0;
      else { belowN++; if (belowN == tailN) { ended = true; continue; } }    // pulled, not emitted; `continue` still counts it as consumed
      len++;
    }
  }
  for (int t = s; t < Tmax; t++) dm[row + t] = 0;
  start[u] = rec ? st : T - (int) headN;                               // _prefixN - _headN, also when the source ended first
  length[u] = len; consumed[u] = s;
}

__global__ __launch_bounds__(256) void k_gather(const float* __restrict__ x, const int* __restrict__ start, const int* __restrict__ length, int U, int Tmax, int dim,
                                                float* __restrict__ y)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tmax * dim) return;
  const int i = (int) (idx % dim), j = (int) ((idx / dim) % Tmax), u = (int) (idx / ((size_t) dim * Tmax));
  const int s = start[u] + j;
  y[idx] = (j < length[u] && s >= 0 && s < Tmax) ? x[((size_t) u * Tmax + s) * dim + i] : 0.0f;
}

// ---- the spectral-shape operators of sadFeature.cc, a thread per frame, the source's row read in place
// norm() (sadFeature.cc:27-33): float products added to an fp64 sum, its root returned as a float and widened again by normalize() (:35-39)
__device__ __forceinline__ double shape_sigma(const float* r, int n)
{
  double norm = 0.0;
  for (int i = 0; i < n; i++) norm += (double) (r[i] * r[i]);
  return (double) (float) sqrt(norm);
}

// op 0 EnergyDiffusionFeature (:93-118), 1 BandEnergyRatioFeature (:129-153), 2 NegativeEntropyFeature (:205-243), 3 SignificantSubbandsFeature (:253-274)
__global__ __launch_bounds__(256) void k_shape(const float* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int n, int op, int threshX, float thresh,
                                               float* __restrict__ y)
{
  const size_t f = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t) U * Tmax) return;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[f] = 0.0f; return; }
  const float* r = x + f * n;
  if (op == 0) {
    double norm = 0.0;
    for (int j = 0; j < n; j++) { const double val = r[j]; norm += val * val; }
    norm = sqrt(norm);
    double diff = 0.0;
    for (int j = 0; j < n; j++) { const double nval = (double) r[j] / norm; diff -= (nval > 0.0 ? nval * log10(nval) : 0.0); }
    y[f] = (float) diff;
  } else if (op == 1) {
    float ssLow = 0.0f, ssHigh = 0.0f;
    for (int j = 0; j < threshX; j++) { const float val = r[j]; ssLow += val * val; }
    for (int j = threshX; j < n; j++) { const float val = r[j]; ssHigh += val * val; }
    y[f] = sqrtf(ssLow / ssHigh);
  } else if (op == 2) {
    double sum = 0.0, sumS = 0.0;
    for (int j = 0; j < n; j++) { const float val = r[j]; const float w = val < 0 ? -val : val; sum += (double) w; sumS += (double) (w * w); }
    const double mean = sum / (double) (unsigned) n;
    const double dev = sqrt((sumS / (double) (unsigned) (n - 1)) - (mean * mean));
    sum = 0.0;
    for (int j = 0; j < n; j++) { const float val = r[j]; const float w = val < 0 ? -val : val; const float z = (float) (((double) w - mean) / dev); sum += log(cosh((double) z)); }
    const double EGy = sum / (double) (unsigned) n, EGgy = 0.374576;
    y[f] = (float) (100.0 * (EGy - EGgy) * (EGy - EGgy));
  } else {
    const double sigma = shape_sigma(r, n);
    double sum = 0.0;
    for (int j = 0; j < n; j++) { const float w = (float) ((double) r[j] / sigma); if (w > thresh) sum += 1.0; }
    y[f] = (float) sum;
  }
}

// ---- NegentropyVADMetric (sad.cc:1103-1131), MutualInformationVADMetric (:1437-1535), LikelihoodRatioVADMetric (:1572-1621)
// One workgroup per utterance; thread b owns bin b (and b + 256, ...).  Frames go in chunks of TC: every thread walks the chunk's frames in order
// for its bins -- the rho recursion of the mutual information is serial in the frames, rho is used before it is updated -- and leaves the
// per-bin terms in LDS; then thread j sums frame j's terms over the bins lowX .. highX ascending, which is the reference's order.
// tab[b] = (f, Bc, normalisation, fJ, BJ, joint normalisation); kind 0 negentropy, 1 mutual information, 2 likelihood ratio.
__device__ __forceinline__ double gg_loglhood(double absX, double scale, double f, double Bc, double nm) { return nm - pow(absX / (scale * Bc), f) - 2.0 * log(scale); }

__global__ __launch_bounds__(256) void k_gg(const double2* __restrict__ X1, const double2* __restrict__ X2, const float* __restrict__ e1, const float* __restrict__ e2,
                                            const int* __restrict__ nf, int Tmax, int N, int F, int envDim, int lowX, int highX, unsigned binN, int kind, int TC,
                                            const double* __restrict__ tab, double gF, double gBc, double gNm, double fixedThr, double twiddle, double threshold, double beta,
                                            double2* __restrict__ rho, double* __restrict__ dec, double* __restrict__ score, double* __restrict__ thr)
{
  extern __shared__ double gg_lds[];
  double* term = gg_lds; double* tterm = gg_lds + (size_t) TC * F;
  const int u = blockIdx.x, tid = threadIdx.x;
  const int T = clampT(nf, u, Tmax);
  const bool total = kind == 1 && !(twiddle < 0.0);
  for (int t0 = 0; t0 < T; t0 += TC) {
    const int tc = T - t0 < TC ? T - t0 : TC;
    for (int b = tid; b < F; b += 256) {
      const double f = tab[6 * b], Bc = tab[6 * b + 1], nm = tab[6 * b + 2];
      double2 r = make_double2(0.0, 0.0);
      if (kind == 1) r = rho[(size_t) u * F + b];
      for (int j = 0; j < tc; j++) {
        const size_t fr = (size_t) u * Tmax + t0 + j;
        const double2 x1 = X1[fr * N + b];
        const double a1 = hypot(x1.x, x1.y);
        double v;
        if (kind == 0) {
          const double sg = sqrt((double) e1[fr * envDim + b]);
          v = gg_loglhood(a1, sg, f, Bc, nm) - gg_loglhood(a1, sg, gF, gBc, gNm);          // gF = 2.0 at run time: the same pow as the bin's, so a Gaussian bin gives exactly 0
        } else if (kind == 2) {
          const double2 x2 = X2[fr * N + b];
          const double sg = sqrt(((double) e1[fr * envDim + b] + (double) e2[fr * envDim + b]) / 2);     // of the unrooted envelopes, as written (:1594-1596)
          v = gg_loglhood(a1, sg, f, Bc, nm) - gg_loglhood(hypot(x2.x, x2.y), sg, f, Bc, nm);
        } else {
          const double2 x2 = X2[fr * N + b];
          const double s1 = sqrt((double) e1[fr * envDim + b]), s2 = sqrt((double) e2[fr * envDim + b]);
          const double fJ = tab[6 * b + 3], BJ = tab[6 * b + 4], nJ = tab[6 * b + 5];
          const double abs2r = r.x * r.x + r.y * r.y;
          if (total) tterm[(size_t) j * F + b] = -log(1.0 - abs2r);
          // logLhood of the joint pdf (:1252-1284): the scaled adjugate of Sigma_X, s = X^H Sigma_X^-1 X written out
          const double ss = s1 * s2, s12x = r.x * ss, s12y = r.y * ss;
          const double det = s1 * s1 * s2 * s2 * (1.0 - abs2r), inv = 1.0 / det;
          const double m00 = (s2 * s2) * inv, m11 = (s1 * s1) * inv, m01x = -s12x * inv, m01y = -s12y * inv;          // m10 = conj(m01)
          const double y0x = (m00 * x1.x) + (m01x * x2.x - m01y * x2.y), y0y = (m00 * x1.y) + (m01x * x2.y + m01y * x2.x);
          const double y1x = (m01x * x1.x + m01y * x1.y) + (m11 * x2.x), y1y = (m01x * x1.y - m01y * x1.x) + (m11 * x2.y);
          const double sx = (x1.x * y0x + x1.y * y0y) + (x2.x * y1x + x2.y * y1y), sy = (x1.x * y0y - x1.y * y0x) + (x2.x * y1y - x2.y * y1x);
          const double ssqrt = sqrt(hypot(sx, sy));
          const double joint = nJ - pow(ssqrt / (sqrt(2.0) * BJ), fJ) - log(det);
          v = joint - gg_loglhood(a1, s1, f, Bc, nm) - gg_loglhood(hypot(x2.x, x2.y), s2, f, Bc, nm);
          // the cross-correlation coefficient for the next frame (:1504-1510)
          const double cx = (x1.x * x2.x + x1.y * x2.y) / ss, cy = (x1.y * x2.x - x1.x * x2.y) / ss;
          r.x = r.x * beta + cx * (1.0 - beta); r.y = r.y * beta + cy * (1.0 - beta);
          const double ar = hypot(r.x, r.y);
          if (ar >= (1.0 - 0.10)) { const double sc = (1.0 - 0.10) / ar; r.x *= sc; r.y *= sc; }
        }
        term[(size_t) j * F + b] = v;
      }
      if (kind == 1) rho[(size_t) u * F + b] = r;
    }
    __syncthreads();
    for (int j = tid; j < tc; j += 256) {
      double sum = 0.0, tot = fixedThr;
      for (int b = lowX; b <= highX; b++) {
        const double v = term[(size_t) j * F + b];
        sum += b == 0 ? v : 2.0 * v;
        if (total) { const double w = tterm[(size_t) j * F + b]; tot += b == 0 ? w : 2.0 * w; }
      }
      sum /= (double) binN;
      const double th = kind == 1 ? (total ? tot * (twiddle / (double) binN) : threshold) : threshold;
      const size_t fr = (size_t) u * Tmax + t0 + j;
      score[fr] = sum; dec[fr] = sum > th ? 1.0 : 0.0;
      if (thr) thr[fr] = th;
    }
    __syncthreads();
  }
  for (int t = T + tid; t < Tmax; t += 256) { const size_t fr = (size_t) u * Tmax + t; score[fr] = 0.0; dec[fr] = 0.0; if (thr) thr[fr] = 0.0; }
}

struct SScratch { DevBuf<double> e, pw; };
PerStream<SScratch> s_scratch;

void batch(const void* x, int U, int Tmax, int dim)
{
  if (!x) throw Error(DSR_E_PARAMETER, "null argument");
  if (U < 1 || Tmax < 0 || dim < 1) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d Tmax=%d dim=%d", U, Tmax, dim);
  if ((double) U * (double) Tmax >= 2147483648.0) throw Error(DSR_E_DIMENSION, "too many frames (%d x %d)", U, Tmax);
  if ((double) U * (double) Tmax * (double) dim >= 4294967296.0 * 256.0) throw Error(DSR_E_DIMENSION, "batch of %d x %d x %d elements is too large", U, Tmax, dim);
  require_device();
}
dim3 grid256(size_t n) { return dim3((unsigned) ((n + 255) / 256)); }

unsigned median_index(double threshold, int energiesN)
{
  if (energiesN < 1 || energiesN > 8192) throw Error(DSR_E_DIMENSION, "energiesN = %d is outside [1, 8192] (the history lives in LDS).", energiesN);
  if (!(threshold >= 0.0 && threshold < 1.0))                          // unsigned(threshold * energiesN) indexes one past the sorted array (sad.cc:443, 507)
    throw Error(DSR_E_DIMENSION, "Threshold %g is outside [0, 1).", threshold);
  return (unsigned) (threshold * energiesN);
}

}  // namespace

extern "C" {

dsr_status dsr_sad_energy_state_init(double* hist_dev, int32_t* counters_dev, int U, int energiesN, double initialEnergy, int countersOnly, void* stream)
{
  return guard([&] {
    if (!hist_dev || !counters_dev || U < 1 || energiesN < 1) throw Error(DSR_E_PARAMETER, "bad argument");
    require_device();
    const size_t n = std::max((size_t) U * energiesN, (size_t) U);
    launch(k_energy_init, grid256(n), dim3(256), 0, (hipStream_t) stream, hist_dev, counters_dev, U, energiesN, initialEnergy, countersOnly);
  });
}

dsr_status dsr_sad_energy_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double threshold, unsigned headN, unsigned tailN, int energiesN,
                              double* hist_dev, int32_t* counters_dev, double* decision_dev, double* score_dev, int32_t* updates_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, U, Tmax, dim);
    if (!hist_dev || !counters_dev || !decision_dev || !score_dev) throw Error(DSR_E_PARAMETER, "null argument");
    const unsigned mi = median_index(threshold, energiesN);
    hipStream_t st = (hipStream_t) stream;
    if (Tmax > 0)
      launch(k_frame_energy<float>, grid256((size_t) U * Tmax), dim3(256), 0, st, x_dev, nframes_dev, U, Tmax, dim, score_dev);
    launch(k_energy_walk, dim3(U), dim3(64), (size_t) energiesN * sizeof(double), st, score_dev, nframes_dev, Tmax, energiesN, mi, headN, tailN, hist_dev,
                       counters_dev, decision_dev, updates_dev);
  });
}

dsr_status dsr_sad_energy_percentile(const double* hist_host, int energiesN, double percentile, double* value)
{
  return guard([&] {
    if (!hist_host || !value || energiesN < 1) throw Error(DSR_E_PARAMETER, "bad argument");
    if (percentile < 0.0 || percentile > 100.0) throw Error(DSR_E_DIMENSION, "Percentile %g is out of range [0.0, 100.0].", percentile);   // sad.cc:512-513
    const int k = int((percentile / 100.0) * energiesN);
    if (k >= energiesN) throw Error(DSR_E_DIMENSION, "Percentile %g reads entry %d of %d sorted energies.", percentile, k, energiesN);
    std::vector<double> s(hist_host, hist_host + energiesN);
    std::sort(s.begin(), s.end());
    *value = s[k] / energiesN;                                          // sad.cc:518
  });
}

dsr_status dsr_sad_simple_energy_run(const void* X_dev, const int32_t* nframes_dev, int U, int Tmax, int fftLen, double threshold, double gamma, double* E_dev,
                                     double* decision_dev, double* score_dev, void* stream)
{
  return guard([&] {
    batch(X_dev, U, Tmax, fftLen);
    if (!E_dev || !decision_dev || !score_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    SScratch& sc = s_scratch.at(st);
    sc.e.reserve((size_t) U * Tmax);
    launch(k_frame_energy<double2>, grid256((size_t) U * Tmax), dim3(256), 0, st, (const double2*) X_dev, nframes_dev, U, Tmax, fftLen, sc.e.p);
    launch(k_simple_walk, dim3(cdiv(U, 64)), dim3(64), 0, st, sc.e.p, nframes_dev, U, Tmax, threshold, gamma, E_dev, decision_dev, score_dev);
  });
}

dsr_status dsr_sad_band(unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, unsigned* lowX, unsigned* highX, unsigned* binN)
{
  return guard([&] {
    if (!lowX || !highX || !binN) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftLen < 2) throw Error(DSR_E_DIMENSION, "fftLen = %u", fftLen);
    unsigned lo = 0, hi = fftLen / 2;                                   // sad.cc:595-629
    if (!(lowCutoff < 0.0)) {
      if (lowCutoff >= sampleRate / 2.0) throw Error(DSR_E_DIMENSION, "Low cutoff cannot be %10.1f", lowCutoff);
      lo = (unsigned) ((lowCutoff / sampleRate) * fftLen);
    }
    if (!(highCutoff < 0.0)) {
      if (highCutoff >= sampleRate / 2.0) throw Error(DSR_E_DIMENSION, "High cutoff cannot be %10.1f", highCutoff);
      hi = (unsigned) ((highCutoff / sampleRate) * fftLen + 0.5);
    }
    *lowX = lo; *highX = hi;
    *binN = lo > 0 ? 2 * (hi - lo + 1) : 2 * (hi - lo) + 1;
  });
}

dsr_status dsr_sad_power_run(const float* P_dev, const int32_t* nframes_dev, int U, int C, int Tmax, unsigned fftLen, unsigned lowX, unsigned highX, int kind, double E0,
                             double* decision_dev, double* powers_dev, double* score_dev, void* stream)
{
  return guard([&] {
    const int F = (int) (fftLen / 2 + 1);
    batch(P_dev, U, Tmax, F);
    if (!decision_dev || !powers_dev || !score_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (C < 1 || (double) U * Tmax * C >= 2147483648.0) throw Error(DSR_E_DIMENSION, "bad channel count %d", C);
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    if (lowX > highX || highX >= (unsigned) F) throw Error(DSR_E_DIMENSION, "Bins %u .. %u lie outside a spectrum of %d bins.", lowX, highX, F);
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    launch(k_band_power, grid256((size_t) U * Tmax * C), dim3(256), 0, st, P_dev, nframes_dev, U, C, Tmax, F, (int) lowX, (int) highX, fftLen, powers_dev);
    launch(k_power_decide, grid256((size_t) U * Tmax), dim3(256), 0, st, powers_dev, nframes_dev, U, C, Tmax, kind, E0, decision_dev, score_dev);
  });
}

static dsr_status ccc_run(const void* X_dev, int isDouble, const int32_t* nframes_dev, int U, int C, int Tmax, unsigned fftLen, unsigned lowX, unsigned highX,
                          unsigned nCand, double threshold, double* decision_dev, double* score_dev, double* cands_dev, int nbest, void* stream)
{
  return guard([&] {
    batch(X_dev, U, Tmax, (int) fftLen);
    if (!decision_dev || !score_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftLen < 4 || fftLen > 2048 || (fftLen & (fftLen - 1))) throw Error(DSR_E_DIMENSION, "fftLen = %u is no power of two in [4, 2048].", fftLen);
    if (C < 2) throw Error(DSR_E_DIMENSION, "CCCVADMetric needs at least 2 channels, got %d.", C);
    if (nCand < 1 || nCand > 64) throw Error(DSR_E_DIMENSION, "nCand = %u is outside [1, 64].", nCand);
    if (lowX > highX || highX > fftLen / 2) throw Error(DSR_E_DIMENSION, "Bins %u .. %u lie outside 0 .. %u.", lowX, highX, fftLen / 2);
    if (Tmax == 0) return;
    const int N = (int) fftLen; int logN = 0; while ((1 << logN) < N) logN++;
    const size_t lds = (size_t) (2 * N + 2 * fft_tw_entries(N)) * sizeof(double);
    const dim3 grid((unsigned) ((size_t) U * Tmax)), block(fft_block(N / 2));
    hipStream_t st = (hipStream_t) stream;
    if (isDouble)
      launch(k_ccc<double2>, grid, block, lds, st, (const double2*) X_dev, nframes_dev, U, C, Tmax, N, logN, (int) lowX, (int) highX, (int) nCand, threshold,
                         decision_dev, score_dev, cands_dev, nbest);
    else
      launch(k_ccc<float2>, grid, block, lds, st, (const float2*) X_dev, nframes_dev, U, C, Tmax, N, logN, (int) lowX, (int) highX, (int) nCand, threshold,
                         decision_dev, score_dev, cands_dev, nbest);
  });
}

dsr_status dsr_sad_ccc_run(const void* X_dev, int isDouble, const int32_t* nframes_dev, int U, int C, int Tmax, unsigned fftLen, unsigned lowX, unsigned highX,
                           unsigned nCand, double threshold, double* decision_dev, double* score_dev, double* cands_dev, void* stream)
{ return ccc_run(X_dev, isDouble, nframes_dev, U, C, Tmax, fftLen, lowX, highX, nCand, threshold, decision_dev, score_dev, cands_dev, 1, stream); }

dsr_status dsr_sad_ccc_transforms_only(const void* X_dev, int isDouble, int U, int C, int Tmax, unsigned fftLen, unsigned lowX, unsigned highX, double* decision_dev,
                                       double* score_dev, void* stream)
{ return ccc_run(X_dev, isDouble, nullptr, U, C, Tmax, fftLen, lowX, highX, 1, 0.0, decision_dev, score_dev, nullptr, 0, stream); }

dsr_status dsr_sad_hangover_run(const double* decisions_dev, const int32_t* nframes_dev, int K, int U, int Tmax, const double* thresholds, unsigned headN, unsigned tailN,
                                int kind, int32_t* start_dev, int32_t* length_dev, int32_t* consumed_dev, int32_t* decision_metric_dev, void* stream)
{
  return guard([&] {
    batch(decisions_dev, U, Tmax, 1);
    if (!thresholds || !start_dev || !length_dev || !consumed_dev || !decision_metric_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (K < 1 || K > 8) throw Error(DSR_E_DIMENSION, "%d metrics: 1 to 8 are supported.", K);
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    if (kind == 1 && K != 3) throw Error(DSR_E_DIMENSION, "HangoverMIVADFeature takes 3 metrics, got %d.", K);
    if (headN < 1) throw Error(DSR_E_DIMENSION, "headN = 0: the reference's ring of buffered frames would be empty.");
    HangArgs a; for (int k = 0; k < 8; k++) a.thr[k] = k < K ? thresholds[k] : 0.0;
    launch(k_hangover, dim3(cdiv(U, 64)), dim3(64), 0, (hipStream_t) stream, decisions_dev, nframes_dev, K, U, Tmax, kind, a, headN, tailN, start_dev,
                       length_dev, consumed_dev, decision_metric_dev);
  });
}

dsr_status dsr_sad_gather_run(const float* x_dev, const int32_t* start_dev, const int32_t* length_dev, int U, int Tmax, int dim, float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, U, Tmax, dim);
    if (!start_dev || !length_dev || !y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (Tmax == 0) return;
    launch(k_gather, grid256((size_t) U * Tmax * dim), dim3(256), 0, (hipStream_t) stream, x_dev, start_dev, length_dev, U, Tmax, dim, y_dev);
  });
}

dsr_status dsr_sad_band_ratio_index(int dim, float sampleRate, float threshF, int* threshX)
{
  return guard([&] {
    if (!threshX || dim < 1) throw Error(DSR_E_PARAMETER, "bad argument");
    const float mx = sampleRate / 2.0, df = mx / (unsigned) dim, tf = (threshF > 0.0) ? threshF : mx / 2.0f;        // sadFeature.cc:124-125
    const int tx = int(floor(tf / df));
    if (tx < 0 || tx > dim) throw Error(DSR_E_DIMENSION, "The threshold %g Hz is bin %d of %d: the low band would be read past the frame.", tf, tx, dim);
    *threshX = tx;
  });
}

dsr_status dsr_sad_shape_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, int op, float sampleRate, float thresh, float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, U, Tmax, dim);
    if (!y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (op < 0 || op > 3) throw Error(DSR_E_PARAMETER, "operator %d", op);
    int tx = 0;
    if (op == 1 && dsr_sad_band_ratio_index(dim, sampleRate, thresh, &tx)) throw Error(DSR_E_DIMENSION, "%s", dsr_last_error());
    if (Tmax == 0) return;
    launch(k_shape, grid256((size_t) U * Tmax), dim3(256), 0, (hipStream_t) stream, x_dev, nframes_dev, U, Tmax, dim, op, tx, thresh, y_dev);
  });
}

}  // extern "C"

// ---- the host side of the generalised-Gaussian metrics
struct dsr_sad_gg {
  unsigned fftLen = 0, lowX = 0, highX = 0, binN = 0; int F = 0; bool joint = false;
  std::vector<double> tab; double gBc = 1.0, gNm = 0.0, fixedThr = 0.0; DevBuf<double> dTab; bool up = false;
};

namespace {
void gg_marginal(double f, double& Bc, double& nm)                     // sad.cc:1038-1049
{
  Bc = exp((std::lgamma(2.0 / f) - std::lgamma(4.0 / f)) / 2.0);
  nm = log(f / (2 * M_PI * Bc * Bc * std::tgamma(2.0 / f)));
}
double gg_match_marginal(double f)                                     // :1312-1321
{
  const double Bc2 = exp(std::lgamma(2.0 / f) - std::lgamma(4.0 / f));
  return -(2.0 * ((2.0 / f) - log(f / (2.0 * M_PI * Bc2 * std::tgamma(2.0 / f)))));
}
double gg_match_joint(double fJ)                                       // :1323-1332
{
  const double BJ4 = exp((std::lgamma(4.0 / fJ) - std::lgamma(6.0 / fJ)) * 2.0);
  return -((4.0 / fJ) - log(fJ / (8.0 * M_PI * M_PI * BJ4 * std::tgamma(4.0 / fJ))));
}
double gg_match(double f)                                              // :1338-1369; the reference loops for ever where this does not converge
{
  double a = f / 3.0, c = 2.0; const double match = gg_match_marginal(f);
  for (int it = 0; it < 200; it++) {
    const double b = (a + c) / 2.0, ratiob = gg_match_joint(b);
    if (fabs(match - ratiob) < 1.0e-06) return b;
    if (ratiob > match) a = b; else c = b;
  }
  throw Error(DSR_E_NUMERIC, "The joint shape factor matching %g was not found in 200 bisection steps.", f);
}
}  // namespace

extern "C" {

dsr_status dsr_sad_gg_create(const double* shapeFactors, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, int joint, dsr_sad_gg** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftLen < 2 || fftLen > 4096) throw Error(DSR_E_DIMENSION, "fftLen = %u is outside [2, 4096].", fftLen);
    std::unique_ptr<dsr_sad_gg> g(new dsr_sad_gg());
    unsigned lo, hi, bn;
    if (dsr_sad_band(fftLen, sampleRate, lowCutoff, highCutoff, &lo, &hi, &bn)) throw Error(DSR_E_DIMENSION, "%s", dsr_last_error());
    g->fftLen = fftLen; g->lowX = lo; g->highX = hi; g->binN = bn; g->F = (int) (fftLen / 2 + 1); g->joint = joint != 0;
    g->tab.assign((size_t) g->F * 6, 0.0);
    gg_marginal(2.0, g->gBc, g->gNm);
    for (int b = 0; b < g->F; b++) {
      const double f = shapeFactors ? shapeFactors[b] : 2.0;
      if (!(f > 0.0)) throw Error(DSR_E_PARAMETER, "Shape factor %g of bin %d is not positive.", f, b);
      double Bc, nm; gg_marginal(f, Bc, nm);
      double* r = &g->tab[(size_t) b * 6]; r[0] = f; r[1] = Bc; r[2] = nm;
      if (!joint) continue;
      const double fJ = gg_match(f);                                    // :1198-1246
      const double BJ = exp((std::lgamma(4.0 / fJ) - std::lgamma(6.0 / fJ)) / 2.0);
      r[3] = fJ; r[4] = BJ; r[5] = log(fJ / (8.0 * M_PI * M_PI * BJ * BJ * BJ * BJ * std::tgamma(4.0 / fJ)));
      double thresh = 2.0 * ((2.0 / f) - log(f / (2.0 * M_PI * (Bc * Bc) * std::tgamma(2.0 / f))));          // :1399-1434
      thresh -= ((4.0 / fJ) - log(fJ / (8.0 * M_PI * M_PI * pow(BJ, 4.0) * std::tgamma(4.0 / fJ))));
      if ((unsigned) b >= lo && (unsigned) b <= hi) g->fixedThr += b == 0 ? thresh : 2.0 * thresh;
    }
    *out = g.release();
  });
}
void dsr_sad_gg_destroy(dsr_sad_gg* g) { delete g; }
dsr_status dsr_sad_gg_table(const dsr_sad_gg* g, double* table, double* fixedThreshold)
{
  return guard([&] {
    if (!g || !table || !fixedThreshold) throw Error(DSR_E_PARAMETER, "null argument");
    memcpy(table, g->tab.data(), g->tab.size() * sizeof(double)); *fixedThreshold = g->fixedThr;
  });
}
dsr_status dsr_sad_gg_read_shape_factors(const char* directory, unsigned fftLen, double* shapeFactors)
{
  return guard([&] {
    if (!directory || !shapeFactors) throw Error(DSR_E_PARAMETER, "null argument");
    for (unsigned b = 0; b <= fftLen / 2; b++) {                       // sad.cc:1077-1095: the second token of the first line
      char name[1024]; snprintf(name, sizeof name, "%s/_M-%04d", directory, b);
      FILE* fp = fopen(name, "r");
      if (!fp) throw Error(DSR_E_IO, "Could not open file %s.", name);
      char line[1024]; const bool got = fgets(line, sizeof line, fp) != nullptr; fclose(fp);
      char* tok = got ? strtok(line, " ") : nullptr; tok = tok ? strtok(nullptr, " ") : nullptr;
      if (!tok) throw Error(DSR_E_PARSE, "%s: the first line has no second token.", name);
      shapeFactors[b] = strtod(tok, nullptr);
    }
  });
}
dsr_status dsr_sad_gg_run(dsr_sad_gg* g, int kind, const void* X1_dev, const void* X2_dev, const float* env1_dev, const float* env2_dev, int envDim,
                          const int32_t* nframes_dev, int U, int Tmax, double twiddle, double threshold, double beta, void* rho_dev, double* decision_dev,
                          double* score_dev, double* threshold_dev, void* stream)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null model");
    batch(X1_dev, U, Tmax, (int) g->fftLen);
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    if (!env1_dev || !decision_dev || !score_dev || (kind > 0 && (!X2_dev || !env2_dev))) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind == 1 && (!rho_dev || !g->joint)) throw Error(DSR_E_PARAMETER, "the mutual information needs the joint model and the rho state");
    if (envDim < g->F) throw Error(DSR_E_DIMENSION, "A spectral envelope of %d elements where %d bins are read.", envDim, g->F);
    hipStream_t st = (hipStream_t) stream;
    if (!g->up) { g->dTab.upload(g->tab, st); g->up = true; }
    int TC = 4096 / g->F; TC = TC < 1 ? 1 : (TC > 16 ? 16 : TC);
    const size_t lds = (size_t) 2 * TC * g->F * sizeof(double);
    launch(k_gg, dim3(U), dim3(256), lds, st, (const double2*) X1_dev, (const double2*) X2_dev, env1_dev, env2_dev, nframes_dev, Tmax, (int) g->fftLen, g->F,
                       envDim, (int) g->lowX, (int) g->highX, g->binN, kind, TC, g->dTab.p, 2.0, g->gBc, g->gNm, g->fixedThr, twiddle, threshold, beta, (double2*) rho_dev,
                       decision_dev, score_dev, threshold_dev);
  });
}

}  // extern "C"
