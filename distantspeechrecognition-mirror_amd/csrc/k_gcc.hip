// csrc/k_gcc.hip -- pairwise time-delay estimation, include/dsr.h section 2e.
//
// Restates the GCC family of btk/localization (localization.h:75-218, localization.cc:1156-1413: NoisePowerSpectrum::add,
// NoiseCrossSpectrum::add, the six calcCrossSpectrumValue forms, GCC::calculate, GCC::findMaximum, getInterpolation :872-894) and CCTDE
// (btk/TDEstimator/CCTDE.cc:146-261).  fp64 throughout, built without FMA contraction.
//
// Kernels:
//   k_gcc_spectrum   a workgroup per (utterance, pair), a thread per bin: walks the frames in order with the smoothed cross-spectrum, the
//                    pair's noise cross-spectrum and its two channels' noise powers and last timestamps in registers; writes the
//                    cross-spectrum of every speech frame.
//   k_gcc_chan       a workgroup per (utterance, channel): the same noise-power recurrence once more, written back to the carried state;
//                    channel 0's workgroup also writes "last speech frame <= t" for the utterance.
//   k_gcc_corr       a workgroup per (utterance, speech frame, pair): half-spectrum pack, inverse real FFT of fftLen as a complex FFT of
//                    fftLen/2 in LDS with the split step, findMaximum as a workgroup reduction, interpolation by one lane.
//   k_gcc_find_state findMaximum over the correlation the state carries (the answer a non-speech frame repeats; the per-call findMaximum).
//   k_gcc_fill       non-speech frames copy the answer of the last speech frame before them (before k_gcc_corr those that repeat the carried
//                    answer, after it the rest), frames past the end get zeros.
//   k_cctde          a workgroup per block pair: Hann window, both real FFTs as one complex FFT, unit-magnitude cross-spectrum, scaled
//                    inverse FFT, nHeldMaxCC rounds of a workgroup arg-max (one lane replays the insertion loop when a tie at the last
//                    held value makes the rounds ambiguous).
//                    fftLen <= 4096 in LDS; longer transforms (allsamples() over a recording) run the same code on a per-workgroup block of
//                    global memory.
// Host side (handle construction, the per-call face, the dsr_gcc_* / dsr_cctde_* entries): csrc/gcc.cpp; what the two share: csrc/gcc.h.
// The FFT itself (fft_tw_init, fft_run, brev, the split step) lives in fft_lds.h, shared with k_conv.hip.
// LDS layout of the FFT: real and imaginary parts in separate fp64 arrays, so a half-wave's 32 consecutive elements fill one 256-byte bank
// row per ds_read_b64; twiddles of the two longest stages come from one table (stride 1 and 2), every shorter stage has a contiguous table
// of its own, because a power-of-two stride into one table would put a half-wave's twiddles on one bank.  The bit-reversed store that loads
// the data is conflicted (DESIGN 4.4j gives its cost).
#include "launch.h"
#include "dev_math.h"
#include "fft_lds.h"
#include "gcc.h"
#include <cmath>

using namespace dsr;

namespace {

struct GState { double* ts; double* hasN; double* Np; double* hasG; double* hasC; double2* Gn; double2* S; double* corr; };
GState gcarve(const dsr_gcc& g, void* base, int U)
{
  const GLayout l = glayout(g, U); double* b = (double*) base;
  return GState{b + l.ts, b + l.hasN, b + l.Np, b + l.hasG, b + l.hasC, (double2*) (b + l.Gn), (double2*) (b + l.S), b + l.corr};
}

struct GPar { int kind, U, C, P, T, len, N, xDouble, smooth, interpolate, active, ac1, ac2; double alpha, beta, q, sampleRate, minDelay, maxDelay; };

__device__ __forceinline__ double2 ldx(const void* X, size_t i, int dbl)
{
  if (dbl) return ((const double2*) X)[i];
  const float2 v = ((const float2*) X)[i]; return make_double2((double) v.x, (double) v.y);
}
// gsl_complex_mul(a, conj(b))
__device__ __forceinline__ double2 mulc(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * (-b.y), a.x * (-b.y) + a.y * b.x); }

// NoisePowerSpectrum::add (localization.cc:1163-1183)
__device__ __forceinline__ void noise_power(double2 x, double stamp, double alpha, double& N, double& has, double& ts)
{
  if (ts != stamp) {
    const double v = hypot(x.x, x.y), a1 = 1.0 - alpha;
    N = has != 0.0 ? alpha * N + a1 * v * v : a1 * v * v;
    has = 1.0; ts = stamp;
  }
}

// calcCrossSpectrumValue (localization.cc:1342-1413)
__device__ __forceinline__ double2 cross_value(int kind, double2 x1, double2 x2, double2 Gn, bool hasG, double N1, bool has1, double N2, bool has2, double q)
{
  const double2 G = mulc(x1, x2);
  if (kind == DSR_GCC_RAW) return G;
  if (kind == DSR_GCC_GNNSUB) return hasG ? make_double2(G.x - Gn.x, G.y - Gn.y) : G;               // the missing estimate is reported by the caller
  if (kind == DSR_GCC_PHAT) {
    const double w = hypot(G.x, G.y);
    return w == 0.0 ? make_double2(0.0, 0.0) : make_double2(G.x / w, G.y / w);
  }
  if (kind == DSR_GCC_GNNSUBPHAT) {
    const double2 D = hasG ? make_double2(G.x - Gn.x, G.y - Gn.y) : G;
    const double w = hypot(D.x, D.y);
    return make_double2(D.x / w, D.y / w);
  }
  const double X1 = hypot(x1.x, x1.y), X12 = X1 * X1, X2 = hypot(x2.x, x2.y), X22 = X2 * X2, q1 = 1.0 - q, q2 = 2.0 * q;
  if (kind == DSR_GCC_MLRRAW) {
    const double w = (has1 && has2) ? X1 * X2 / (q2 * X12 * X22 + q1 * (N2 * X12 + N1 * X22)) : X1 * X2 / (q2 * X12 * X22);
    return make_double2(G.x * w, G.y * w);
  }
  if (hasG && has1 && has2) {
    const double w = X1 * X2 / (q2 * X12 * X22 + q1 * (N2 * X12 + N1 * X22));
    return make_double2((G.x - Gn.x) * w, (G.y - Gn.y) * w);
  }
  const double w = X1 * X2 / (q2 * X12 * X22);
  return make_double2(G.x * w, G.y * w);
}

// GCC::calculate (localization.cc:1263-1295) over the frames of one (utterance, pair); a thread owns the bins tid, tid + blockDim, ...
__global__ __launch_bounds__(256) void k_gcc_spectrum(const void* __restrict__ X, const int* __restrict__ nf, const int* __restrict__ sad,
                                                      const double* __restrict__ stamp, const int* __restrict__ pairs, GPar p, GState s,
                                                      double2* __restrict__ xspec, int* __restrict__ err)
{
  const int u = blockIdx.x / p.P, pr = blockIdx.x % p.P;
  if (u >= p.U || (p.active >= 0 && pr != p.active)) return;
  const int c1 = p.active >= 0 ? p.ac1 : pairs[2 * pr], c2 = p.active >= 0 ? p.ac2 : pairs[2 * pr + 1];
  const int T = clampT(nf, u, p.T);
  const size_t up = (size_t) u * p.P + pr, uc1 = (size_t) u * p.C + c1, uc2 = (size_t) u * p.C + c2;
  const double hasG0 = s.hasG[up], ts10 = s.ts[uc1], ts20 = s.ts[uc2], h10 = s.hasN[uc1], h20 = s.hasN[uc2];
  __syncthreads();                                                                                     // every lane has the flags before lane 0 rewrites them
  const double a1 = 1.0 - p.alpha, b1 = 1.0 - p.beta;
  double hasGEnd = hasG0; bool speech = false;
  for (int f = threadIdx.x; f < p.len; f += blockDim.x) {
    double2 S = s.S[up * p.len + f], Gn = s.Gn[up * p.len + f];
    double hasG = hasG0, N1 = s.Np[uc1 * p.len + f], N2 = s.Np[uc2 * p.len + f], ts1 = ts10, ts2 = ts20, has1 = h10, has2 = h20;
    const size_t x1b = ((size_t) u * p.C + c1) * p.T * p.len + f, x2b = ((size_t) u * p.C + c2) * p.T * p.len + f;
    for (int t = 0; t < T; t++) {
      const double2 x1 = ldx(X, x1b + (size_t) t * p.len, p.xDouble), x2 = ldx(X, x2b + (size_t) t * p.len, p.xDouble);
      if (sad[(size_t) u * p.T + t]) {
        if (p.kind == DSR_GCC_GNNSUB && hasG == 0.0) *err = 1;
        const double2 G = cross_value(p.kind, x1, x2, Gn, hasG != 0.0, N1, has1 != 0.0, N2, has2 != 0.0, p.q);
        S = p.smooth ? make_double2(S.x * p.beta + G.x * b1, S.y * p.beta + G.y * b1) : G;
        xspec[(((size_t) u * p.T + t) * p.P + pr) * p.len + f] = S;
        speech = true;
      } else {
        const double ts = stamp[(size_t) u * p.T + t];
        noise_power(x1, ts, p.alpha, N1, has1, ts1);
        if (c1 == c2) { N2 = N1; has2 = has1; ts2 = ts1; } else noise_power(x2, ts, p.alpha, N2, has2, ts2);
        const double2 v = mulc(x1, x2);                                                               // NoiseCrossSpectrum::add (:1191-1218)
        Gn = hasG != 0.0 ? make_double2(Gn.x * p.alpha + v.x * a1, Gn.y * p.alpha + v.y * a1) : make_double2(v.x * a1, v.y * a1);
        hasG = 1.0;
      }
    }
    s.S[up * p.len + f] = S; s.Gn[up * p.len + f] = Gn; hasGEnd = hasG;
  }
  if (threadIdx.x == 0) { s.hasG[up] = hasGEnd; if (speech) s.hasC[up] = 1.0; }
}

// the carried channel state, and the utterance's "last speech frame <= t" (-1: none yet in this call)
__global__ __launch_bounds__(256) void k_gcc_chan(const void* __restrict__ X, const int* __restrict__ nf, const int* __restrict__ sad,
                                                  const double* __restrict__ stamp, const int* __restrict__ inPair, GPar p, GState s, int* __restrict__ lastSpeech)
{
  const int u = blockIdx.x / p.C, c = blockIdx.x % p.C;
  if (u >= p.U) return;
  const int T = clampT(nf, u, p.T);
  if (c == 0 && threadIdx.x == 0) {
    int last = -1;
    for (int t = 0; t < p.T; t++) { if (t < T && sad[(size_t) u * p.T + t]) last = t; lastSpeech[(size_t) u * p.T + t] = t < T ? last : -2; }
  }
  if (p.active >= 0 ? (c != p.ac1 && c != p.ac2) : !inPair[c]) return;                                 // GCC::calculate never sees this channel
  const size_t uc = (size_t) u * p.C + c;
  const double ts0 = s.ts[uc], h0 = s.hasN[uc];
  __syncthreads();
  double tsEnd = ts0, hEnd = h0;
  for (int f = threadIdx.x; f < p.len; f += blockDim.x) {
    double N = s.Np[uc * p.len + f], ts = ts0, has = h0;
    const size_t xb = uc * p.T * p.len + f;
    for (int t = 0; t < T; t++)
      if (!sad[(size_t) u * p.T + t]) noise_power(ldx(X, xb + (size_t) t * p.len, p.xDouble), stamp[(size_t) u * p.T + t], p.alpha, N, has, ts);
    s.Np[uc * p.len + f] = N; tsEnd = ts; hEnd = has;
  }
  if (threadIdx.x == 0) { s.ts[uc] = tsEnd; s.hasN[uc] = hEnd; }
}

// ---- findMaximum (localization.cc:1297-1340) as a workgroup reduction ---------------------------------------------------------------------
// The strict `>` scan over ascending i keeps the first of equal maxima: order (corr descending, i ascending).  maxCorr2 ends as the largest
// in-window value at any other index: what the running maximum held before the winner, or a later value above it (the two branches).
struct LdsCorr { const double* re; const double* im; __device__ double operator()(int i) const { return (i & 1) ? im[i >> 1] : re[i >> 1]; } };
struct MemCorr { const double* c; __device__ double operator()(int i) const { return c[i]; } };

__device__ __forceinline__ double lag_of(int i, int N, double sr) { return i < N / 2 ? (double) i / sr : -((double) (N - i) / sr); }

template <class Corr> __device__ void find_maximum(Corr corr, const GPar& p, double* rv, double* rs, int* ri, double* out3)
{
  const int N = p.N, tid = threadIdx.x;
  double best = -HUGE_D, sec = -HUGE_D; int bi = 0x7fffffff;
  for (int i = tid; i < N; i += blockDim.x) {
    const double d = lag_of(i, N, p.sampleRate), c = corr(i);
    if (d >= p.minDelay && d <= p.maxDelay) {
      if (c > best) { sec = best; best = c; bi = i; } else if (c > sec) sec = c;
    }
  }
  rv[tid] = best; rs[tid] = sec; ri[tid] = bi;
  for (int o = blockDim.x / 2; o >= 1; o >>= 1) {
    __syncthreads();
    if (tid < o) {
      const double v2 = rv[tid + o], s2 = rs[tid + o]; const int i2 = ri[tid + o];
      double v1 = rv[tid], s1 = rs[tid]; int i1 = ri[tid];
      const bool take2 = v2 > v1 || (v2 == v1 && i2 < i1);
      const double loser = take2 ? v1 : v2;
      double s = s1 > s2 ? s1 : s2; if (loser > s) s = loser;
      if (take2) { v1 = v2; i1 = i2; }
      rv[tid] = v1; rs[tid] = s; ri[tid] = i1;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const double maxCorr = rv[0], maxCorr2 = rs[0]; const int i = ri[0];
    double delay = 0.0; int pos = 0;
    if (i != 0x7fffffff) { delay = lag_of(i, N, p.sampleRate); pos = i < N / 2 ? i + N / 2 : i - N / 2; }
    if (p.interpolate) {                                                                               // getInterpolation (:872-894)
      if (pos == 0) pos = 1; else if (pos == N - 1) pos = N - 2;
      double x[3], y[3];
      for (int k = 0; k < 3; k++) { const int q = pos - 1 + k, j = q >= N / 2 ? q - N / 2 : q + N / 2; x[k] = lag_of(j, N, p.sampleRate); y[k] = corr(j); }
      const double b = (y[1] - y[0]) / (x[1] - x[0]), a = (y[2] - y[1]) / (x[2] - x[1]);
      delay = 0.5 * ((x[0] + x[1]) - b * (x[2] - x[0]) / (a - b));
    }
    out3[0] = delay; out3[1] = maxCorr; out3[2] = maxCorr / maxCorr2;
  }
  __syncthreads();
}

// dynamic LDS: re[n] im[n] twr[tw] twi[tw] rv[B] rs[B] ri[B], n = N/2
__global__ __launch_bounds__(256) void k_gcc_corr(const double2* __restrict__ xspec, const int* __restrict__ nf, const int* __restrict__ lastSpeech, GPar p,
                                                  GState s, double* __restrict__ result, int* __restrict__ valid, double* __restrict__ corrOut, long nItems)
{
  extern __shared__ double lds[];
  const int N = p.N, n = N / 2, logn = 31 - __clz(n), B = blockDim.x, tw = fft_tw_entries(n);
  double* re = lds; double* im = re + n; double* twr = im + n; double* twi = twr + tw; double* rv = twi + tw; double* rs = rv + B; int* ri = (int*) (rs + B);
  fft_tw_init(twr, twi, n);
  const double inv = 1.0 / (double) N;
  for (long it = blockIdx.x; it < nItems; it += gridDim.x) {
    const int u = (int) (it / ((long) p.T * p.P)), t = (int) ((it / p.P) % p.T), pr = (int) (it % p.P);
    if (lastSpeech[(size_t) u * p.T + t] != t || (p.active >= 0 && pr != p.active)) continue;          // uniform over the workgroup
    const double2* Sx = xspec + (size_t) it * p.len;
    __syncthreads();
    // halfComplexPack keeps Re of bins 0 and N/2 only; split step: Z[k] = (X[k] + conj X[n-k]) + i (X[k] - conj X[n-k]) e^{2 pi i k / N}
    for (int k = threadIdx.x; k < n; k += B) {
      double2 A = Sx[k], Bn = Sx[n - k];
      if (k == 0) { A.y = 0.0; Bn.y = 0.0; }
      const double2 z = fft_split_inverse(A, Bn, k, n);
      const int r = brev(k, logn);
      re[r] = z.x; im[r] = z.y;
    }
    fft_run(re, im, twr, twi, n, 1.0);
    for (int k = threadIdx.x; k < n; k += B) { re[k] *= inv; im[k] *= inv; }                           // gsl_fft_halfcomplex_radix2_inverse scales by 1/N
    __syncthreads();
    const LdsCorr corr{re, im};
    find_maximum(corr, p, rv, rs, ri, result + (size_t) it * 3);
    if (threadIdx.x == 0) valid[it] = 1;
    const int T = clampT(nf, u, p.T);
    const bool lastOne = lastSpeech[(size_t) u * p.T + T - 1] == t;                                    // T >= 1 here: frame t < T is a speech frame
    if (lastOne || corrOut)
      for (int i = threadIdx.x; i < N; i += B) {
        const double c = corr(i);
        if (lastOne) s.corr[((size_t) u * p.P + pr) * N + i] = c;
        if (corrOut) corrOut[(size_t) it * N + i] = c;
      }
  }
}

// findMaximum over the carried correlation of every (utterance, pair); valid = 0 and zeros before the first speech frame
__global__ __launch_bounds__(256) void k_gcc_find_state(GPar p, GState s, double* __restrict__ result, int* __restrict__ valid)
{
  __shared__ double rv[256], rs[256]; __shared__ int ri[256];
  const size_t up = blockIdx.x;
  if (s.hasC[up] == 0.0) {
    if (threadIdx.x == 0) { result[up * 3] = 0.0; result[up * 3 + 1] = 0.0; result[up * 3 + 2] = 0.0; valid[up] = 0; }
    return;
  }
  const MemCorr corr{s.corr + up * p.N};
  find_maximum(corr, p, rv, rs, ri, result + up * 3);
  if (threadIdx.x == 0) valid[up] = 1;
}

// a thread per (utterance, frame, pair): what a non-speech frame repeats, zeros past the end
__global__ void k_gcc_fill(const int* __restrict__ lastSpeech, GPar p, const double* __restrict__ prevRes, const int* __restrict__ prevValid,
                           double* __restrict__ result, int* __restrict__ valid, double* __restrict__ corrOut, GState s, long nItems, int afterCorr)
{
  const long it = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (it >= nItems) return;
  const int u = (int) (it / ((long) p.T * p.P)), t = (int) ((it / p.P) % p.T), pr = (int) (it % p.P);
  const int ls = lastSpeech[(size_t) u * p.T + t];
  if (ls == t || (ls >= 0) != (afterCorr != 0) || (p.active >= 0 && pr != p.active)) return;      // before k_gcc_corr: frames with no speech frame before them; after it: the others
  const size_t up = (size_t) u * p.P + pr;
  double r0 = 0.0, r1 = 0.0, r2 = 0.0; int v = 0;
  const double* src = nullptr;
  if (ls >= 0) {
    const size_t from = ((size_t) u * p.T + ls) * p.P + pr;
    r0 = result[from * 3]; r1 = result[from * 3 + 1]; r2 = result[from * 3 + 2]; v = 1;
    if (corrOut) src = corrOut + from * p.N;
  } else if (ls == -1) {
    r0 = prevRes[up * 3]; r1 = prevRes[up * 3 + 1]; r2 = prevRes[up * 3 + 2]; v = prevValid[up];
    if (corrOut && v) src = s.corr + up * p.N;                                                         // k_gcc_corr has not run yet: still the carried one
  }
  result[it * 3] = r0; result[it * 3 + 1] = r1; result[it * 3 + 2] = r2; valid[it] = v;
  if (corrOut) for (int i = 0; i < p.N; i++) corrOut[(size_t) it * p.N + i] = src ? src[i] : 0.0;
}

__global__ void k_gcc_state_init(double* st, size_t n) { const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; if (i < n) st[i] = 0.0; }

// ---- CCTDE (CCTDE.cc:146-261) ---------------------------------------------------------------------------------------------------------------
// dynamic LDS: re[N] im[N] twr[tw] twi[tw] rv[B] ri[B] for fftLen <= CC_LDS_MAX (115 KB of the 160 KB at 4096).  GLOBAL: only rv, ri are in
// LDS; re im re2 im2 twr twi are the workgroup's block of `work` in global memory (the waves of a workgroup share a CU and its L1, and
// __syncthreads() orders their accesses), and the cross-spectrum goes to the second pair of arrays instead of through registers.
constexpr int CC_LDS_MAX = 4096, CC_MAXK = CC_LDS_MAX / 2 / 256 + 1;                                     // (4096 / 2 + 1) bins over 256 lanes
inline size_t cc_work_doubles(int N) { return (size_t) 4 * N + 2 * (size_t) fft_tw_entries(N); }
__device__ __forceinline__ double2 unit_of(double x, double y)                                          // cos / sin of atan2(y, x); atan2(0, 0) = 0
{
  if (x == 0.0 && y == 0.0) return make_double2(1.0, 0.0);
  const double w = hypot(x, y); return make_double2(x / w, y / w);
}
// the unit-magnitude cross-spectrum at bin k from Z = FFT(a + i b): A = Z[k] + conj Z[N-k], B = -i (Z[k] - conj Z[N-k]) (the common factor 1/2 drops out)
__device__ __forceinline__ double2 cc_bin(const double* re, const double* im, int k, int N)
{
  const int kk = (N - k) & (N - 1);
  const double zr = re[k], zi = im[k], yr = re[kk], yi = -im[kk];
  const double2 ua = unit_of(zr + yr, zi + yi), ub = unit_of(zi - yi, -(zr - yr));
  return make_double2(ua.x * ub.x + ua.y * ub.y, ua.x * ub.y - ua.y * ub.x);                           // conj(ua) ub = e^{i (phase B - phase A)}
}
__device__ __forceinline__ void cc_store(double* re, double* im, int k, int N, int logn, double2 c)
{
  const int r = brev(k, logn);
  re[r] = c.x; im[r] = c.y;
  if (k > 0 && k < N / 2) { const int r2 = brev(N - k, logn); re[r2] = c.x; im[r2] = -c.y; }
}
template <bool GLOBAL>
__global__ __launch_bounds__(256) void k_cctde(const float* __restrict__ a, const float* __restrict__ b, const double* __restrict__ win, int nItems, int blockLen,
                                               int N, int nHeld, int sampleRate, double* __restrict__ delays, int* __restrict__ args, double* __restrict__ vals,
                                               double* work)
{
  extern __shared__ double lds[];
  const int logn = 31 - __clz(N), B = blockDim.x, tw = fft_tw_entries(N), tid = threadIdx.x;
  double* base = GLOBAL ? work + (size_t) blockIdx.x * ((size_t) 4 * N + 2 * (size_t) tw) : lds;
  double* re = base; double* im = re + N; double* re2 = GLOBAL ? im + N : re; double* im2 = GLOBAL ? re2 + N : im;
  double* twr = im2 + N; double* twi = twr + tw; double* rv = GLOBAL ? lds : twi + tw; int* ri = (int*) (rv + B);
  fft_tw_init(twr, twi, N);
  const double inv = 1.0 / (double) N;
  for (int it = blockIdx.x; it < nItems; it += gridDim.x) {
    __syncthreads();
    for (int k = tid; k < N; k += B) {
      const int r = brev(k, logn);
      const bool in = k < blockLen;
      re[r] = in ? win[k] * (double) a[(size_t) it * blockLen + k] : 0.0;
      im[r] = in ? win[k] * (double) b[(size_t) it * blockLen + k] : 0.0;
    }
    fft_run(re, im, twr, twi, N, -1.0);
    if (GLOBAL) {
      for (int k = tid; k <= N / 2; k += B) cc_store(re2, im2, k, N, logn, cc_bin(re, im, k, N));
      double* t = re; re = re2; re2 = t; t = im; im = im2; im2 = t;                                    // the roles swap with every item
    } else {
      double2 cc[CC_MAXK];
#pragma unroll
      for (int m = 0; m < CC_MAXK; m++) { const int k = tid + m * B; if (k <= N / 2) cc[m] = cc_bin(re, im, k, N); }
      __syncthreads();
#pragma unroll
      for (int m = 0; m < CC_MAXK; m++) { const int k = tid + m * B; if (k <= N / 2) cc_store(re, im, k, N, logn, cc[m]); }
    }
    fft_run(re, im, twr, twi, N, 1.0);
    for (int k = tid; k < N; k += B) { re[k] *= inv; im[k] = 0.0; }                                    // im[] becomes the "taken" flag of the rounds
    double* oD = delays + (size_t) it * nHeld; int* oA = args + (size_t) it * nHeld; double* oV = vals + (size_t) it * nHeld;
    // round r: the largest value not taken yet, the later index among equals (`>=` puts a newcomer above its equals)
    for (int r = 0; r < nHeld; r++) {
      __syncthreads();
      double best = -INFINITY; int bi = -1;
      for (int i = tid; i < N; i += B) { const double c = re[i]; if (im[i] == 0.0 && c >= best && c > -10e10) { best = c; bi = i; } }
      rv[tid] = best; ri[tid] = bi;
      for (int o = B / 2; o >= 1; o >>= 1) {
        __syncthreads();
        if (tid < o) { const double v2 = rv[tid + o]; const int i2 = ri[tid + o]; if (i2 >= 0 && (ri[tid] < 0 || v2 > rv[tid] || (v2 == rv[tid] && i2 > ri[tid]))) { rv[tid] = v2; ri[tid] = i2; } }
      }
      __syncthreads();
      if (tid == 0) { const int i = ri[0]; oA[r] = i; oV[r] = i >= 0 ? rv[0] : -10e10; if (i >= 0) im[i] = 1.0; }
    }
    __syncthreads();
    // a value equal to the last held one that was left out: which of the equals survive depends on the arrival order, replay the loop (:214-236)
    const double vLast = rv[0]; const int iLast = ri[0];
    __syncthreads();
    int tie = 0;
    if (iLast >= 0) for (int i = tid; i < N; i += B) if (im[i] == 0.0 && re[i] == vLast) tie = 1;
    ri[tid] = tie;
    for (int o = B / 2; o >= 1; o >>= 1) { __syncthreads(); if (tid < o) ri[tid] |= ri[tid + o]; }
    __syncthreads();
    if (tid == 0) {
      if (ri[0]) {
        oA[0] = 0; oV[0] = re[0];
        for (int k = 1; k < nHeld; k++) { oA[k] = -1; oV[k] = -10e10; }
        for (int i = 1; i < N; i++) {
          const double c = re[i];
          if (c > oV[nHeld - 1])
            for (int k = 0; k < nHeld; k++)
              if (c >= oV[k]) { for (int j = nHeld - 1; j > k; j--) { oV[j] = oV[j - 1]; oA[j] = oA[j - 1]; } oV[k] = c; oA[k] = i; break; }
        }
      }
      for (int k = 0; k < nHeld; k++) {                                                                // :240-252, through float as there
        const unsigned arg = (unsigned) oA[k]; float td;
        if (arg < (unsigned) N / 2) td = (float) (arg * 1.0 / sampleRate);
        else td = (float) (-((float) N - (float) arg) * 1.0 / sampleRate);
        oD[k] = (double) td;
      }
    }
  }
}

struct GScratch { DevBuf<double> xspec, prevRes, win, work; DevBuf<int> last, prevValid, err; };
PerStream<GScratch> g_scratch;

void gcc_upload(dsr_gcc* g)
{
  if (g->uploaded) return;
  g->d_pairs.upload(g->pairs); g->d_inPair.upload(g->inPair); g->uploaded = true;
}
// active >= 0: one calculate() call -- that pair alone, bound to the channels (ac1, ac2) for this call
GPar gpar(const dsr_gcc& g, int U, int T, int xDouble, int smooth, double minDelay, double maxDelay, int active = -1, int ac1 = -1, int ac2 = -1)
{ return GPar{g.kind, U, g.C, g.P, T, g.len, g.N, xDouble, smooth, g.interpolate, active, ac1, ac2, g.alpha, g.beta, g.q, g.sampleRate, minDelay, maxDelay}; }

}  // namespace

namespace dsr {

void gcc_launch_run(dsr_gcc* g, const void* X_dev, int xIsDouble, const int32_t* nframes_dev, const int32_t* sad_dev, const double* timestamp_dev, int smooth,
                    double minDelay, double maxDelay, int U, int Tmax, void* state_dev, double* result_dev, int32_t* valid_dev, double* corr_dev,
                    void* xspec_dev, hipStream_t st, int active, int ac1, int ac2)
{
  gcc_upload(g);
  GScratch& sc = g_scratch.at(st);
  const long items = (long) U * Tmax * g->P;
  double2* xs = (double2*) xspec_dev;
  if (!xs) { sc.xspec.reserve((size_t) items * g->len * 2); xs = (double2*) sc.xspec.p; }
  sc.prevRes.reserve((size_t) U * g->P * 3); sc.prevValid.reserve((size_t) U * g->P); sc.last.reserve((size_t) U * Tmax); sc.err.reserve(1);
  const GState s = gcarve(*g, state_dev, U);
  const GPar p = gpar(*g, U, Tmax, xIsDouble != 0, smooth != 0, minDelay, maxDelay, active, ac1, ac2);
  DSR_HIP(hipMemsetAsync(sc.err.p, 0, sizeof(int), st));
  // the answer this call's leading non-speech frames repeat, from the carried correlation, before anything rewrites it
  launch(k_gcc_find_state, dim3(U * g->P), dim3(256), 0, st, p, s, sc.prevRes.p, sc.prevValid.p);
  const int bs = g->len >= 256 ? 256 : ((g->len + 63) / 64) * 64;
  g->tm.mark(0, st);
  launch(k_gcc_spectrum, dim3(U * g->P), dim3(bs), 0, st, X_dev, nframes_dev, sad_dev, timestamp_dev, g->d_pairs.p, p, s, xs, sc.err.p);
  g->tm.mark(1, st);
  launch(k_gcc_chan, dim3(U * g->C), dim3(bs), 0, st, X_dev, nframes_dev, sad_dev, timestamp_dev, g->d_inPair.p, p, s, sc.last.p);
  const int n = g->N / 2, B = fft_block(n / 2);
  const size_t ldsBytes = ((size_t) 2 * n + 2 * fft_tw_entries(n) + 2 * B) * 8 + (size_t) B * 4;
  const int grid = (int) (items < 16384 ? items : 16384);
  launch(k_gcc_fill, dim3(cdiv(items, 256)), dim3(256), 0, st, sc.last.p, p, sc.prevRes.p, sc.prevValid.p, result_dev, valid_dev, corr_dev, s, items, 0);
  g->tm.mark(2, st);
  launch(k_gcc_corr, dim3(grid), dim3(B), ldsBytes, st, xs, nframes_dev, sc.last.p, p, s, result_dev, valid_dev, corr_dev, items);
  g->tm.mark(3, st);
  launch(k_gcc_fill, dim3(cdiv(items, 256)), dim3(256), 0, st, sc.last.p, p, sc.prevRes.p, sc.prevValid.p, result_dev, valid_dev, corr_dev, s, items, 1);
  if (g->kind == DSR_GCC_GNNSUB) {                                                                    // the reference dereferences a null noise cross-spectrum here
    int e = 0; DSR_HIP(hipMemcpyAsync(&e, sc.err.p, sizeof(int), hipMemcpyDeviceToHost, st)); DSR_HIP(hipStreamSynchronize(st));
    if (e) throw Error(DSR_E_ERROR, "GCCGnnSub: a speech frame came before any noise frame of its pair (no noise cross-spectrum to subtract)");
  }
}

void gcc_launch_find_maximum(const dsr_gcc& g, double minDelay, double maxDelay, int U, void* state_dev, double* result_dev, int32_t* valid_dev, hipStream_t st)
{
  launch(k_gcc_find_state, dim3(U * g.P), dim3(256), 0, st, gpar(g, U, 1, 0, 0, minDelay, maxDelay), gcarve(g, state_dev, U), result_dev, valid_dev);
}

void gcc_launch_state_init(double* state_dev, size_t n, hipStream_t st)
{
  launch(k_gcc_state_init, dim3(cdiv((long) n, 256)), dim3(256), 0, st, state_dev, n);
}

void cctde_launch(const float* a_dev, const float* b_dev, int nItems, int blockLen, int fftLen, int nHeldMaxCC, int sampleRate, double* delays_dev,
                  int32_t* args_dev, double* values_dev, hipStream_t st)
{
  GScratch& sc = g_scratch.at(st);
  std::vector<double> w(fftLen);                                                                     // getWindow(2, fftLen) (modulated.cc:82-87)
  for (int i = 0; i < fftLen; i++) w[i] = 0.5 * (1 - std::cos((2.0 * M_PI * i) / (double) (fftLen - 1)));
  sc.win.reserve(fftLen);
  DSR_HIP(hipMemcpyAsync(sc.win.p, w.data(), sizeof(double) * fftLen, hipMemcpyHostToDevice, st)); DSR_HIP(hipStreamSynchronize(st));
  const int B = fft_block(fftLen / 2);
  if (fftLen <= CC_LDS_MAX) {
    const size_t ldsBytes = ((size_t) 2 * fftLen + 2 * fft_tw_entries(fftLen) + B) * 8 + (size_t) B * 4;
    const int grid = nItems < 16384 ? nItems : 16384;
    launch(k_cctde<false>, dim3(grid), dim3(B), ldsBytes, st, a_dev, b_dev, sc.win.p, nItems, blockLen, fftLen, nHeldMaxCC, sampleRate, delays_dev, args_dev,
                       values_dev, (double*) nullptr);
  } else {                                                                                           // a recording at once (allsamples): few items, long transforms
    const int grid = nItems < 8 ? nItems : 8;
    sc.work.reserve(cc_work_doubles(fftLen) * grid);
    launch(k_cctde<true>, dim3(grid), dim3(B), (size_t) B * 12, st, a_dev, b_dev, sc.win.p, nItems, blockLen, fftLen, nHeldMaxCC, sampleRate, delays_dev,
                       args_dev, values_dev, sc.work.p);
  }
}

}  // namespace dsr
