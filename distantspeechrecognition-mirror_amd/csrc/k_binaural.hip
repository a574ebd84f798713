// csrc/k_binaural.hip -- two-channel time-frequency masks and their threshold estimators (include/dsr.h section 6a-3):
// BinaryMaskFilter, KimBinaryMaskFilter, IIDBinaryMaskFilter, KimITDThresholdEstimator, IIDThresholdEstimator and
// FDIIDThresholdEstimator of btk/postfilter/binauralprocessing.{h,cc}.
//
// Masks (k_mask): one lane per (utterance, bin), frames in order -- the smoothed mask mu is a first-order recursion along time, held
// and computed in fp32 as the reference's `float mu` is, with explicit round-to-nearest multiplies and adds (no fused multiply-add).
//
// Estimators.  The reference evaluates, per frame, every candidate threshold against every bin.  Each decision is monotone in the
// candidate (the table is strictly increasing and a <= b + th is monotone in th), so a (frame, bin) item is described by the first
// candidate index k at which the reference's own predicate -- evaluated in its own floating-point form against the table, by bisection --
// turns true.  An item adds its "predicate true" value to every candidate i >= k and its "predicate false" value to every i < k:
//   S[i] = sum_{k <= i} vTrue + sum_{k > i} vFalse
// Both sums are of non-negative terms; they are formed as an ascending and a descending running sum of two LDS histograms (never as a
// difference), so nothing cancels.  Cost per frame is O(bins + candidates) instead of O(bins x candidates).
//   k_est_band   Kim and IID: a workgroup takes a slice of 32 of an utterance's frames; the histograms of up to 1024 candidates fit 64 KB
//                of LDS; Kim scans and applies pow() per frame, IID (linear in the items) scans once per slice and side.
//                Slice partials go to a workspace and k_est_reduce adds them to the caller's accumulators in slice order.
//   k_est_fd     FDIID: a workgroup takes one bin of an utterance over all frames, scans once, and owns its accumulators.
#include "launch.h"
#include <cmath>

using namespace dsr;

namespace {

constexpr int BS = 256;

// calcITDf (binauralprocessing.cc:12-33) as written
__device__ __forceinline__ double calc_itd(int f, int M, float2 L, float2 R)
{
  const double aL = atan2((double) L.y, (double) L.x), aR = atan2((double) R.y, (double) R.x);
  const double d1 = fabs(aL - aR), d2 = fabs(aL - aR - 2 * M_PI), d3 = fabs(aL - aR + 2 * M_PI);
  double d = d1 < d2 ? d1 : d2;
  if (d3 < d) d = d3;
  return d / (2 * M_PI * f / M);
}

struct MkPar { int kind, chanX, U, Tmax, F, M, outBins, outIsDouble, carry; float threshold, alpha, dEta; };

__global__ void __launch_bounds__(64) k_mask(const float2* __restrict__ XL, const float2* __restrict__ XR, const int* __restrict__ nframes,
                                              const double* __restrict__ thrAtFreq, float* __restrict__ state, void* __restrict__ out,
                                              float* __restrict__ muOut, double* __restrict__ itdOut, MkPar p)
{
  const int f = blockIdx.x * 64 + threadIdx.x, u = blockIdx.y;
  if (f >= p.F) return;
  int nf = nframes ? nframes[u] : p.Tmax; nf = nf < 0 ? 0 : nf > p.Tmax ? p.Tmax : nf;
  float prev = p.carry ? state[(size_t) u * p.F + f] : 1.0f;
  const float oma = __fsub_rn(1.0f, p.alpha), omaEta = __fmul_rn(oma, p.dEta);
  const float thr = (p.kind == 2 && thrAtFreq) ? (float) thrAtFreq[f] : p.threshold;       // _threshold = gsl_vector_get(...) rounds to float (:456-457)
  for (int t = 0; t < p.Tmax; t++) {
    const size_t row = (size_t) u * p.Tmax + t;
    double re = 0.0, im = 0.0, itd = 0.0; float mu = 0.0f;
    if (t < nf && p.kind != 0) {
      const float2 L = XL[row * p.F + f], R = XR[row * p.F + f];
      if (f == 0) { re = L.x; im = L.y; mu = prev; }
      else {
        bool pass; float2 X;
        if (p.kind == 1) {                                                 // KimBinaryMaskFilter::masking1 (:135-176)
          itd = calc_itd(f, p.M, L, R);
          const bool le = itd <= (double) thr;
          pass = p.chanX == 0 ? le : !le; X = p.chanX == 0 ? L : R;
        } else {                                                           // IIDBinaryMaskFilter::masking1 (:441-485)
          X = p.chanX == 0 ? L : R; const float2 I = p.chanX == 0 ? R : L;
          const double PT = hypot((double) X.x, (double) X.y), PI = hypot((double) I.x, (double) I.y);
          pass = !(PT <= (PI + (double) thr));
        }
        mu = __fadd_rn(__fmul_rn(p.alpha, prev), pass ? oma : omaEta);
        re = (double) X.x * (double) mu; im = (double) X.y * (double) mu; prev = mu;
      }
    }
    store_c(out, row * p.outBins + f, re, im, p.outIsDouble);
    if (p.outBins == p.M && f > 0 && f < p.M / 2) store_c(out, row * p.outBins + (p.M - f), re, -im, p.outIsDouble);
    if (muOut) muOut[row * p.F + f] = mu;
    if (itdOut) itdOut[row * p.F + f] = itd;
  }
  if (nf > 0 && p.kind != 0) state[(size_t) u * p.F + f] = prev;
}
__global__ void k_fill_f(float* p, size_t n, float v) { const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; if (i < n) p[i] = v; }

// ---------------------------------------------------------------------------------------------------------------------------------
// estimators

struct EsPar { int kind, U, Tmax, F, M, nCand, nLoop, f0, f1, slice, G; double eta, pc; };   // nCand: the arrays' length; nLoop <= nCand: the candidates the loop reaches

// first index in [0, n) whose candidate makes the predicate true, n when none does; pred(i) is monotone in i
template <class P> __device__ __forceinline__ int first_true(int n, P pred)
{
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (pred(mid)) hi = mid; else lo = mid + 1; }
  return lo;
}
// Inclusive running sum in place over A[0..n), ascending (reverse = false) or descending, by ONE wave.  Lane l owns a contiguous chunk; every
// value is base(l) + local, with local the left-to-right sum inside the chunk and base(l) the left-to-right sum of the chunk totals before l.
// Adding the zeros of empty slots changes nothing, so two candidates between which no item falls get bit-identical sums -- the reference's
// exact ties (runs of candidates that decide every item alike) stay exact ties, and its first/last-minimum rule picks the same index.
__device__ void wave_scan(double* A, int n, bool reverse)
{
  const int lane = threadIdx.x & 63, ch = (n + 63) / 64, b = lane * ch, e = (b + ch < n) ? b + ch : n;
  double tot = 0.0;
  for (int j = b; j < e; j++) tot += A[reverse ? n - 1 - j : j];
  double base = 0.0;
  for (int j = 0; j < 63; j++) { const double tj = __shfl(tot, j, 64); if (j < lane) base += tj; }
  double local = 0.0;
  for (int j = b; j < e; j++) { const int i = reverse ? n - 1 - j : j; local += A[i]; A[i] = base + local; }
}
// the 4 waves of a workgroup share out `narr` arrays of W1 doubles: even ones ascend ("true" values), odd ones descend ("false" values)
__device__ __forceinline__ void scan_arrays(double* H, int narr, int W1)
{
  for (int a = threadIdx.x >> 6; a < narr; a += BS / 64) wave_scan(H + a * W1, W1, (a & 1) != 0);
  __syncthreads();
}

// One window of W = 1024 candidates (the create call refuses longer tables).  Kim: 2 pairs (P_T of the left channel, P_I of the right).
// IID: the T side and the I side have their own keys and their own accumulators, so they run as two passes of 3 pairs (Y1, Y2, Y4) each.
// LDS: 2 NP (W+1) doubles = 32.0 KB / 48.1 KB.
constexpr int W = 1024, W1 = W + 1, CPT = W / BS;
template <int KIND> struct Band { static constexpr int NP = KIND == 0 ? 2 : 3, NACC = KIND == 0 ? 5 : 6, SIDES = KIND == 0 ? 1 : 2; };

template <int KIND> __global__ void __launch_bounds__(BS) k_est_band(const float2* __restrict__ XL, const float2* __restrict__ XR, const int* __restrict__ nframes,
                                                                      const float* __restrict__ cand, double* __restrict__ part, EsPar p)
{
  using B = Band<KIND>; constexpr int NP = B::NP;
  __shared__ double H[2 * NP * W1];
  const int tid = threadIdx.x, g = blockIdx.x, u = blockIdx.y;
  int nf = nframes ? nframes[u] : p.Tmax; nf = nf < 0 ? 0 : nf > p.Tmax ? p.Tmax : nf;
  const int t0 = g * p.slice, t1 = (t0 + p.slice < nf) ? t0 + p.slice : nf;
  double* out = part + ((size_t) u * p.G + g) * B::NACC * p.nCand;
  for (int side = 0; side < B::SIDES; side++) {
    double acc[CPT][KIND == 0 ? 5 : 3];
    for (int a = 0; a < CPT; a++) for (int q = 0; q < (KIND == 0 ? 5 : 3); q++) acc[a][q] = 0.0;
    bool dirty = true;
    for (int t = t0; t < t1; t++) {
      if (dirty) { for (int j = tid; j < 2 * NP * W1; j += BS) H[j] = 0.0; dirty = false; __syncthreads(); }
      const size_t row = ((size_t) u * p.Tmax + t) * p.F;
      for (int f = p.f0 + tid; f < p.f1; f += BS) {
        const float2 L = XL[row + f], R = XR[row + f];
        const double lr = L.x, li = L.y, rr = R.x, ri = R.y;
        if (KIND == 0) {                                                   // KimITDThresholdEstimator::accumStats1 (:314-353)
          const double itd = calc_itd(f, p.M, L, R);
          const int s = first_true(p.nLoop, [&](int i) { return itd <= (double) cand[i]; });
          const double a1 = lr * lr + li * li, aE = (lr * p.eta) * (lr * p.eta) + (li * p.eta) * (li * p.eta);
          const double b1 = rr * rr + ri * ri, bE = (rr * p.eta) * (rr * p.eta) + (ri * p.eta) * (ri * p.eta);
          atomicAdd(&H[0 * W1 + s], a1); atomicAdd(&H[1 * W1 + s], aE);    // pair 0 = P_T: true -> mu_T = 1
          atomicAdd(&H[2 * W1 + s], bE); atomicAdd(&H[3 * W1 + s], b1);    // pair 1 = P_I: true -> mu_I = dEta
        } else {                                                           // IIDThresholdEstimator::accumStats1 (:549-605), one side
          const double PT = hypot(lr, li), PI = hypot(rr, ri), e2 = 2.0 * p.pc;
          const int s = side == 0 ? first_true(p.nLoop, [&](int i) { return PT <= (PI + (double) cand[i]); })
                                  : first_true(p.nLoop, [&](int i) { return PI <= (PT + (double) cand[i]); });
          const double xr = side == 0 ? lr : rr, xi = side == 0 ? li : ri;
          const double y1 = pow(side == 0 ? PT : PI, e2), yE = pow(hypot(xr * p.eta, xi * p.eta), e2), y1s = y1 * y1, yEs = yE * yE;
          atomicAdd(&H[0 * W1 + s], yE); atomicAdd(&H[1 * W1 + s], y1); atomicAdd(&H[2 * W1 + s], yEs); atomicAdd(&H[3 * W1 + s], y1s);
          atomicAdd(&H[4 * W1 + s], yEs * yEs); atomicAdd(&H[5 * W1 + s], y1s * y1s);
        }
      }
      __syncthreads();
      if (KIND == 0 || t == t1 - 1) {
        scan_arrays(H, 2 * NP, W1);
        for (int a = 0; a < CPT; a++) {
          const int s = tid + a * BS; if (s >= p.nLoop) continue;
          double S[NP];
          for (int q = 0; q < NP; q++) S[q] = H[(2 * q) * W1 + s] + H[(2 * q + 1) * W1 + s + 1];
          if (KIND == 0) {
            const double RT = pow(S[0], p.pc), RI = pow(S[1], p.pc);
            acc[a][0] += RT * RI; acc[a][1] += RT; acc[a][2] += RI; acc[a][3] += RT * RT; acc[a][4] += RI * RI;
          } else
            for (int q = 0; q < NP; q++) acc[a][q] += S[q];
        }
        dirty = true; __syncthreads();
      }
    }
    for (int a = 0; a < CPT; a++) {
      const int i = tid + a * BS; if (i >= p.nLoop) continue;
      if (KIND == 0) for (int q = 0; q < 5; q++) out[(size_t) q * p.nCand + i] = acc[a][q];
      else for (int q = 0; q < 3; q++) out[(size_t) (2 * q + side) * p.nCand + i] = acc[a][q];      // mean_T, mean_I, sigma_T, sigma_I, Y4_T, Y4_I
    }
  }
}
// accumulators [U][NACC][nCand] (+ the sample count behind them) += the slice partials, in slice order
__global__ void k_est_reduce(const double* __restrict__ part, const int* __restrict__ nframes, double* __restrict__ state, int U, int G, int n, int Tmax, size_t perU)
{
  const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; if (i >= (size_t) U * (n + 1)) return;
  const int u = (int) (i / (n + 1)), j = (int) (i % (n + 1));
  int nf = nframes ? nframes[u] : Tmax; nf = nf < 0 ? 0 : nf > Tmax ? Tmax : nf;
  if (nf == 0) return;
  double* s = state + (size_t) u * perU;
  if (j == n) { s[perU - 1] += (double) nf; return; }
  double v = s[j];
  for (int g = 0; g < G; g++) v += part[((size_t) u * G + g) * n + j];
  s[j] = v;
}

// FDIIDThresholdEstimator::accumStats1 (:800-844): per bin and candidate, Y4 += Y2T^2 + Y2I^2, mean += Y1T + Y1I, sigma += Y2T + Y2I.
// A workgroup owns one bin of one utterance over all its frames; the T and the I item of a frame go into the same three histogram pairs,
// each under its own key.  3 pairs x 2 x 1025 doubles = 48.0 KB.  The loads are 8 B at a stride of a frame row; the bins next to it are
// other workgroups' and share its cache lines.
__global__ void __launch_bounds__(BS) k_est_fd(const float2* __restrict__ XL, const float2* __restrict__ XR, const int* __restrict__ nframes,
                                                const float* __restrict__ cand, double* __restrict__ state, EsPar p, size_t perU)
{
  constexpr int NA = 6;
  __shared__ double H[NA * W1];
  const int tid = threadIdx.x, u = blockIdx.y, f = 1 + blockIdx.x;
  int nf = nframes ? nframes[u] : p.Tmax; nf = nf < 0 ? 0 : nf > p.Tmax ? p.Tmax : nf;
  if (nf == 0 || f >= p.F) return;
  double* st = state + (size_t) u * perU;
  const size_t plane = (size_t) p.F * p.nCand;                             // state: Y4 [F][nCand], mean [F][nCand], sigma [F][nCand], nSamples
  for (int j = tid; j < NA * W1; j += BS) H[j] = 0.0;
  __syncthreads();
  for (int t = tid; t < nf; t += BS) {
    const size_t idx = ((size_t) u * p.Tmax + t) * p.F + f;
    const float2 L = XL[idx], R = XR[idx];
    const double lr = L.x, li = L.y, rr = R.x, ri = R.y;
    const double PT = hypot(lr, li), PI = hypot(rr, ri), e2 = 2.0 * p.pc;
    const int sT = first_true(p.nLoop, [&](int i) { return PT <= (PI + (double) cand[i]); });
    const int sI = first_true(p.nLoop, [&](int i) { return PI <= (PT + (double) cand[i]); });
    const double yT1 = pow(PT, e2), yTE = pow(hypot(lr * p.eta, li * p.eta), e2), yI1 = pow(PI, e2), yIE = pow(hypot(rr * p.eta, ri * p.eta), e2);
    const double yT1s = yT1 * yT1, yTEs = yTE * yTE, yI1s = yI1 * yI1, yIEs = yIE * yIE;
    atomicAdd(&H[0 * W1 + sT], yTEs * yTEs); atomicAdd(&H[1 * W1 + sT], yT1s * yT1s); atomicAdd(&H[0 * W1 + sI], yIEs * yIEs); atomicAdd(&H[1 * W1 + sI], yI1s * yI1s);
    atomicAdd(&H[2 * W1 + sT], yTE); atomicAdd(&H[3 * W1 + sT], yT1); atomicAdd(&H[2 * W1 + sI], yIE); atomicAdd(&H[3 * W1 + sI], yI1);
    atomicAdd(&H[4 * W1 + sT], yTEs); atomicAdd(&H[5 * W1 + sT], yT1s); atomicAdd(&H[4 * W1 + sI], yIEs); atomicAdd(&H[5 * W1 + sI], yI1s);
  }
  __syncthreads();
  scan_arrays(H, NA, W1);
  for (int j = tid; j < 3 * p.nLoop; j += BS) {
    const int i = j % p.nLoop, q = j / p.nLoop;
    st[q * plane + (size_t) f * p.nCand + i] += H[(2 * q) * W1 + i] + H[(2 * q + 1) * W1 + i + 1];
  }
  if (blockIdx.x == 0 && tid == 0) st[perU - 1] += (double) nf;
}

}  // namespace

struct dsr_binmask {
  int kind = 0, chanX = 0, M = 0, F = 0; float threshold = 0, alpha = 0, dEta = 0.01f, dPowerCoeff = 0; bool carry = false;
  bool haveThr = false; std::vector<double> thr; DevBuf<double> d_thr; bool dirty = false;
};
struct dsr_thest {
  int kind = 0, M = 0, F = 0, nCand = 0, f0 = 1, f1 = 0; float minTh = 0, maxTh = 0, width = 0, dEta = 0.01f, dPowerCoeff = 0; double beta = 3.0;
  std::vector<float> cand; DevBuf<float> d_cand; bool uploaded = false;
  int nacc() const { return kind == 0 ? 5 : kind == 1 ? 6 : 3; }
  size_t per_u() const { return (kind == 2 ? (size_t) 3 * F * nCand : (size_t) nacc() * nCand) + 1; }
};
namespace { struct EstScratch { DevBuf<double> part; }; PerStream<EstScratch> g_est; }

extern "C" {

dsr_status dsr_binmask_create(int kind, unsigned chanX, int fftLen, float threshold, float alpha, float dEta, float dPowerCoeff, dsr_binmask** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d: 0 BinaryMaskFilter, 1 KimBinaryMaskFilter, 2 IIDBinaryMaskFilter", kind);
    if (fftLen < 4 || (fftLen & 1) || fftLen > 65536) throw Error(DSR_E_DIMENSION, "fftLen %d: an even length in [4, 65536] expected", fftLen);
    dsr_binmask* h = new dsr_binmask(); h->kind = kind; h->chanX = (int) chanX; h->M = fftLen; h->F = fftLen / 2 + 1; h->threshold = threshold; h->alpha = alpha; h->dEta = dEta;
    h->dPowerCoeff = dPowerCoeff;                                          // kept and, as in KimBinaryMaskFilter, never used
    *out = h;
  });
}
void dsr_binmask_destroy(dsr_binmask* h) { delete h; }
dsr_status dsr_binmask_set_threshold(dsr_binmask* h, float threshold) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->threshold = threshold; }); }
double dsr_binmask_threshold(const dsr_binmask* h) { return h ? (double) h->threshold : 0.0; }
dsr_status dsr_binmask_set_thresholds(dsr_binmask* h, const double* thresholds, int n)
{
  return guard([&] {
    if (!h || !thresholds) throw Error(DSR_E_PARAMETER, "null argument");
    if (n < h->F) throw Error(DSR_E_DIMENSION, "%d thresholds for %d bins", n, h->F);
    if (!h->haveThr) { h->thr.assign(h->F, 0.0); h->haveThr = true; }      // the first call only allocates (:79-92); the reference's memory is uninitialised, here zeros
    else for (int f = 1; f < h->F; f++) h->thr[f] = thresholds[f];
    h->dirty = true;
  });
}
dsr_status dsr_binmask_thresholds(const dsr_binmask* h, double* out, int n, int32_t* exists)
{
  return guard([&] {
    if (!h || !out || !exists) throw Error(DSR_E_PARAMETER, "null argument");
    *exists = h->haveThr ? 1 : 0; if (!h->haveThr) return;
    if (n < h->F) throw Error(DSR_E_DIMENSION, "%d doubles for %d bins", n, h->F);
    std::copy(h->thr.begin(), h->thr.end(), out);
  });
}
dsr_status dsr_binmask_carry(dsr_binmask* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->carry = on != 0; }); }
size_t dsr_binmask_state_bytes(const dsr_binmask* h, int U) { return (h && U > 0) ? (size_t) U * h->F * 4 : 0; }
dsr_status dsr_binmask_reset_state(const dsr_binmask* h, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!h || !state_dev || U <= 0) throw Error(DSR_E_PARAMETER, "null argument");
    require_device(); const size_t n = (size_t) U * h->F;
    launch(k_fill_f, dim3(cdiv((long) n, 256)), dim3(256), 0, (hipStream_t) stream, (float*) state_dev, n, 1.0f);
  });
}
dsr_status dsr_binmask_state_init(const dsr_binmask* h, void* state_dev, int U, void* stream) { return dsr_binmask_reset_state(h, state_dev, U, stream); }
dsr_status dsr_binmask_apply(dsr_binmask* h, const float* L_dev, const float* R_dev, const int32_t* nframes_dev, int U, int Tmax, void* out_dev, int outBins,
                             int outIsDouble, float* mu_dev, double* itd_dev, void* state_dev, void* stream)
{
  return guard([&] {
    if (!h || !L_dev || !R_dev || !out_dev || !state_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0 || (outBins != h->F && outBins != h->M)) throw Error(DSR_E_DIMENSION, "outBins %d: fftLen/2+1 = %d or fftLen = %d expected", outBins, h->F, h->M);
    if (U == 0 || Tmax == 0) return;
    require_device(); hipStream_t st = (hipStream_t) stream;
    if (h->haveThr && h->dirty) { h->d_thr.upload(h->thr, st); h->dirty = false; }
    MkPar p{h->kind, h->chanX, U, Tmax, h->F, h->M, outBins, outIsDouble, h->carry, h->threshold, h->alpha, h->dEta};
    if (outBins == h->M) DSR_HIP(hipMemsetAsync(out_dev, 0, (size_t) U * Tmax * outBins * (outIsDouble ? 16 : 8), st));
    launch(k_mask, dim3(cdiv(h->F, 64), U), dim3(64), 0, st, (const float2*) L_dev, (const float2*) R_dev, nframes_dev, h->haveThr ? h->d_thr.p : nullptr,
                       (float*) state_dev, out_dev, mu_dev, itd_dev, p);
    if (h->kind == 2 && h->haveThr) h->threshold = (float) h->thr[h->F - 1];   // the scalar is overwritten bin by bin (:456-457): the last bin's value stays
  });
}
dsr_status dsr_binmask_state_read(const dsr_binmask* h, const void* state_dev, int U, int u, float* host_out, size_t outFloats)
{
  return guard([&] {
    if (!h || !state_dev || !host_out) throw Error(DSR_E_PARAMETER, "null argument");
    if (u < 0 || u >= U) throw Error(DSR_E_INDEX, "utterance %d of %d", u, U);
    if (outFloats < (size_t) h->F) throw Error(DSR_E_DIMENSION, "%zu floats for %d", outFloats, h->F);
    require_device(); DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(host_out, (const float*) state_dev + (size_t) u * h->F, (size_t) h->F * 4, hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_thest_create(int kind, int fftLen, float minThreshold, float maxThreshold, float width, float minFreq, float maxFreq, int sampleRate, float dEta,
                            float dPowerCoeff, dsr_thest** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d: 0 KimITD, 1 IID, 2 FDIID", kind);
    if (fftLen < 4 || (fftLen & 1) || fftLen > 65536) throw Error(DSR_E_DIMENSION, "fftLen %d: an even length in [4, 65536] expected", fftLen);
    std::unique_ptr<dsr_thest> h(new dsr_thest()); h->kind = kind; h->M = fftLen; h->F = fftLen / 2 + 1; h->width = width; h->dEta = dEta; h->dPowerCoeff = dPowerCoeff;
    if (minThreshold == maxThreshold) {                                    // binauralprocessing.cc:251-258, :721-728
      if (kind == 2) { h->minTh = -100000; h->maxTh = 100000; } else { h->minTh = (float) (-0.2 * 16000 / 340); h->maxTh = (float) (0.2 * 16000 / 340); }
    } else { h->minTh = minThreshold; h->maxTh = maxThreshold; }
    if (kind == 2 || minFreq < 0 || maxFreq < 0 || sampleRate < 0) { h->f0 = 1; h->f1 = fftLen / 2 + 1; }
    else if (sampleRate == 0) throw Error(DSR_E_PARAMETER, "sampleRate 0 with a band: the reference divides by it");
    else {                                                                 // :260-267; a quotient the cast cannot hold (NaN, beyond the half spectrum) is refused before it
      const float b0 = fftLen * minFreq / (float) sampleRate, b1 = fftLen * maxFreq / (float) sampleRate;
      if (!(b0 < (float) (h->F + 1)) || !(b1 < (float) (h->F + 1))) throw Error(DSR_E_DIMENSION, "the band %g..%g (bins) leaves the %d bins the snapshots hold", (double) b0, (double) b1, h->F);
      h->f0 = (int) (unsigned) b0; h->f1 = (int) (unsigned) b1;
    }
    if (h->f1 > h->F) throw Error(DSR_E_DIMENSION, "the band ends at bin %d, the snapshots hold %d bins", h->f1, h->F);
    if (!(width > 0)) throw Error(DSR_E_PARAMETER, "width %g: the reference's candidate loop does not end", (double) width);
    const double nc = (double) ((h->maxTh - h->minTh) / width) + 1.5;    // :269: float quotient, then + 1.5
    if (!(nc >= 1.0) || nc > 4194304.0) throw Error(DSR_E_ALLOCATION, "%g candidates", nc);
    h->nCand = (int) nc;
    for (float th = h->minTh; th <= h->maxTh; th += width) {               // the loop of accumStats1 / calcThreshold, in float
      if ((int) h->cand.size() == h->nCand) throw Error(DSR_E_INDEX, "the candidate loop yields more than the %d values its arrays hold (the reference writes past them)", h->nCand);
      if (!h->cand.empty() && !(th > h->cand.back())) throw Error(DSR_E_PARAMETER, "width %g does not advance the threshold at %g", (double) width, (double) th);
      if (h->cand.size() == 1024) throw Error(DSR_E_DIMENSION, "more than 1024 candidates: the device path holds one window of 1024 (the SWIG defaults need 942 and 201)");
      h->cand.push_back(th);
    }
    *out = h.release();
  });
}
void dsr_thest_destroy(dsr_thest* h) { delete h; }
int dsr_thest_kind(const dsr_thest* h) { return h ? h->kind : -1; }
int dsr_thest_n_cand(const dsr_thest* h) { return h ? h->nCand : 0; }
int dsr_thest_n_loop(const dsr_thest* h) { return h ? (int) h->cand.size() : 0; }
dsr_status dsr_thest_candidates(const dsr_thest* h, float* out, int n)
{
  return guard([&] {
    if (!h || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (n < (int) h->cand.size()) throw Error(DSR_E_DIMENSION, "%d floats for %zu candidates", n, h->cand.size());
    std::copy(h->cand.begin(), h->cand.end(), out);
  });
}
dsr_status dsr_thest_bin_range(const dsr_thest* h, int32_t* out2) { return guard([&] { if (!h || !out2) throw Error(DSR_E_PARAMETER, "null argument"); out2[0] = h->f0; out2[1] = h->f1; }); }
size_t dsr_thest_acc_doubles(const dsr_thest* h) { return h ? h->per_u() : 0; }
size_t dsr_thest_state_bytes(const dsr_thest* h, int U) { return (h && U > 0) ? (size_t) U * h->per_u() * 8 : 0; }
dsr_status dsr_thest_reset_state(const dsr_thest* h, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!h || !state_dev || U <= 0) throw Error(DSR_E_PARAMETER, "null argument");
    require_device(); const size_t n = (size_t) U * h->per_u();
    DSR_HIP(hipMemsetAsync(state_dev, 0, n * 8, (hipStream_t) stream));
  });
}
dsr_status dsr_thest_state_init(const dsr_thest* h, void* state_dev, int U, void* stream) { return dsr_thest_reset_state(h, state_dev, U, stream); }
dsr_status dsr_thest_run(dsr_thest* h, const float* L_dev, const float* R_dev, const int32_t* nframes_dev, int U, int Tmax, void* state_dev, void* stream)
{
  return guard([&] {
    if (!h || !L_dev || !R_dev || !state_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "U %d, Tmax %d", U, Tmax);
    if (U == 0 || Tmax == 0) return;
    require_device(); hipStream_t st = (hipStream_t) stream;
    if (!h->uploaded) { h->d_cand.upload(h->cand, st); h->uploaded = true; }
    const int nC = (int) h->cand.size();                                   // the candidates the loop reaches; entries behind them stay zero
    EsPar q{h->kind, U, Tmax, h->F, h->M, h->nCand, nC, h->f0, h->f1, 32, cdiv(Tmax, 32), (double) h->dEta, (double) h->dPowerCoeff};
    const EsPar& p = q;
    if (h->kind == 2) {
      launch(k_est_fd, dim3(h->F - 1, U), dim3(BS), 0, st, (const float2*) L_dev, (const float2*) R_dev, nframes_dev, h->d_cand.p,
                         (double*) state_dev, q, h->per_u());
    } else {
      const int n = h->nacc() * h->nCand;
      EstScratch& sc = g_est.at(st); sc.part.reserve((size_t) U * p.G * n);
      if (nC < h->nCand) DSR_HIP(hipMemsetAsync(sc.part.p, 0, (size_t) U * p.G * n * 8, st));
      if (h->kind == 0) launch(k_est_band<0>, dim3(p.G, U), dim3(BS), 0, st, (const float2*) L_dev, (const float2*) R_dev, nframes_dev, h->d_cand.p, sc.part.p, q);
      else launch(k_est_band<1>, dim3(p.G, U), dim3(BS), 0, st, (const float2*) L_dev, (const float2*) R_dev, nframes_dev, h->d_cand.p, sc.part.p, q);
      launch(k_est_reduce, dim3(cdiv((long) U * (n + 1), 256)), dim3(256), 0, st, sc.part.p, nframes_dev, (double*) state_dev, U, p.G, n, Tmax, h->per_u());
    }
  });
}
dsr_status dsr_thest_state_read(const dsr_thest* h, const void* state_dev, int U, int u, double* host_out, size_t outDoubles)
{
  return guard([&] {
    if (!h || !state_dev || !host_out) throw Error(DSR_E_PARAMETER, "null argument");
    if (u < 0 || u >= U) throw Error(DSR_E_INDEX, "utterance %d of %d", u, U);
    if (outDoubles < h->per_u()) throw Error(DSR_E_DIMENSION, "%zu doubles for %zu", outDoubles, h->per_u());
    require_device(); DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(host_out, (const double*) state_dev + (size_t) u * h->per_u(), h->per_u() * 8, hipMemcpyDeviceToHost));
  });
}
// calcThreshold (binauralprocessing.cc:382-407, :634-662, :873-904) from one utterance's accumulators, on the host.  The reference divides its
// accumulators by the sample count in place, so a second call there differs from the first: inPlace != 0 does the same to acc (the stream
// classes), inPlace == 0 leaves acc as it is (the batch finaliser is pure).
dsr_status dsr_thest_calc_threshold(const dsr_thest* h, double* acc, size_t accDoubles, int inPlace, double* threshold, int32_t* index, double* cost,
                                    size_t costDoubles, double* thresholds, int thresholdsN)
{
  return guard([&] {
    if (!h || !acc || !threshold) throw Error(DSR_E_PARAMETER, "null argument");
    if (accDoubles < h->per_u()) throw Error(DSR_E_DIMENSION, "%zu doubles for %zu", accDoubles, h->per_u());
    const int nC = h->nCand, nL = (int) h->cand.size(); const double nS = acc[h->per_u() - 1];
    const size_t nCost = h->kind == 2 ? (size_t) h->F * nC : (size_t) nC;
    if (cost) { if (costDoubles < nCost) throw Error(DSR_E_DIMENSION, "%zu doubles for %zu cost values", costDoubles, nCost); std::fill(cost, cost + nCost, 0.0); }
    if (thresholds && thresholdsN < h->F) throw Error(DSR_E_DIMENSION, "%d thresholds for %d bins", thresholdsN, h->F);
    std::vector<double> copy; double* w = acc;
    if (!inPlace) { copy.assign(acc, acc + h->per_u()); w = copy.data(); }
    float arg = h->minTh; int argI = 0; double minRho = 1000000;
    if (h->kind == 0) {
      double *cf = w, *mT = w + nC, *mI = w + 2 * nC, *sT = w + 3 * nC, *sI = w + 4 * nC;
      for (int i = 0; i < nL; i++) {
        mT[i] /= nS; mI[i] /= nS;
        sT[i] = (sT[i] / nS) - mT[i] * mT[i]; sI[i] = (sI[i] / nS) - mI[i] * mI[i];
        cf[i] /= nS;
        const double rho = fabs((cf[i] - mT[i] * mI[i]) / (sqrt(sT[i]) * sqrt(sI[i])));
        if (cost) cost[i] = cf[i];
        if (rho < minRho) { arg = h->cand[i]; argI = i; minRho = rho; }
      }
    } else if (h->kind == 1) {
      for (int i = 0; i < nL; i++) {
        for (int q = 0; q < 6; q++) w[(size_t) q * nC + i] /= nS;
        const double sig2 = w[2 * (size_t) nC + i] + w[3 * (size_t) nC + i];
        const double c = (w[4 * (size_t) nC + i] + w[5 * (size_t) nC + i]) - h->beta * sig2 * sig2, rho = -c;
        if (cost) cost[i] = c;
        if (rho < minRho) { arg = h->cand[i]; argI = i; minRho = rho; }
      }
    } else {
      const size_t plane = (size_t) h->F * nC; arg = 0.0f;                 // the scalar starts from the constructor's threshold 0.0 (:705)
      if (thresholds) std::fill(thresholds, thresholds + h->F, 0.0);
      for (int f = 1; f < h->F; f++) {
        double localMin = 1000000;
        for (int i = 0; i < nL; i++) {
          const size_t j = (size_t) f * nC + i;
          w[plane + j] /= nS; w[2 * plane + j] /= nS; w[j] /= nS;
          const double c = w[j] - h->beta * w[2 * plane + j] * w[2 * plane + j], rho = -c;   // _beta is uninitialised there; 3.0 as in IIDThresholdEstimator
          if (cost) cost[j] = c;
          if (rho <= minRho) { arg = h->cand[i]; argI = i; minRho = rho; }
          if (rho <= localMin) { if (thresholds) thresholds[f] = h->cand[i]; localMin = rho; }
        }
      }
    }
    *threshold = (double) arg; if (index) *index = argI;
  });
}

}  // extern "C"
