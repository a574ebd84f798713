// csrc/k_specsub.hip -- single-channel noise suppression on subband snapshots (include/dsr.h section 6a-2):
// averagePSDEstimator, SpectralSubtractor and WienerFilter of btk/postfilter/spectralsubtraction.{h,cc}.
//
// Shapes.  Snapshots are [U][C][Tmax][F] complex64, F = fftLen/2+1; all arithmetic is fp64 as in the reference.
//   k_ss_train   one lane per (utterance, bin), frames in order: the recursive noise estimate (alpha >= 0) is a recursion along
//                time, so the lanes run across bins and every load of a frame row is coalesced.
//   k_ss_apply   training off: nothing is carried from frame to frame, one lane per (utterance, frame, bin).
//   k_wiener     one lane per (utterance, bin), frames in order (both PSD memories are first-order recursions).
// Traffic is 8 B in per channel and bin and 8 B (16 B for the stream face) out.  Measured: the two frame-serial kernels are bound
// by their dependent chain per frame (k_wiener's time does not move when the bins double; k_ss_train pays 0.65 us per frame and channel for the
// read-modify-write of its estimates), k_ss_apply by the fp64 atan2/sincos/sqrt per channel and bin at 1.0-1.2 TB/s on the snapshots.
// Built with -ffp-contract=off: the reference's expressions are evaluated as written.
#include "launch.h"
#include <cmath>

using namespace dsr;

namespace {

struct SsPar { int U, C, Tmax, F, M, outBins, outIsDouble, training, subtract; double ft, floorV; };

// per utterance and channel: est[F], sum[F], cnt, seen  (the estimate; the running sum and the number of the samples addSample stored
// while alpha < 0; whether the recursive average has seen its first sample)
__host__ __device__ inline size_t ss_chan_doubles(int F) { return 2 * (size_t) F + 2; }

// one channel's share of one bin of one frame (spectralsubtraction.cc:206-261): returns the addend of _vector[f]
__device__ __forceinline__ double2 ss_bin(float2 x, double est, const SsPar& p)
{
  const double re = x.x, im = x.y;
  if (!p.subtract) return make_double2(re, im);
  const double th = atan2(im, re), X2 = re * re + im * im;
  double S2 = X2 - p.ft * est;
  if (S2 <= p.floorV) S2 = p.floorV;
  const double r = sqrt(S2);
  return make_double2(r * cos(th), r * sin(th));
}

// the row's upper half as SpectralSubtractor::next leaves it: conj mirror for 0 < f < M/2, the rest zero; for the plain average the
// mirror is that of the analysis bank's own frame
__device__ __forceinline__ void ss_store(void* out, size_t row, int f, double2 v, const SsPar& p)
{
  store_c(out, row * p.outBins + f, v.x, v.y, p.outIsDouble);
  if (p.outBins == p.M && f > 0 && f < p.M / 2) store_c(out, row * p.outBins + (p.M - f), v.x, -v.y, p.outIsDouble);
}

__global__ void __launch_bounds__(64) k_ss_train(const float2* __restrict__ X, const int* __restrict__ nframes, const double* __restrict__ alphas,
                                                  double* __restrict__ state, void* __restrict__ out, SsPar p)
{
  const int f = blockIdx.x * 64 + threadIdx.x, u = blockIdx.y;
  if (f >= p.F) return;
  int nf = nframes ? nframes[u] : p.Tmax; nf = nf < 0 ? 0 : nf > p.Tmax ? p.Tmax : nf;
  const double inv = 1.0 / (double) p.C;
  for (int t = 0; t < p.Tmax; t++) {
    const size_t row = (size_t) u * p.Tmax + t;
    if (t >= nf) { if (out) ss_store(out, row, f, make_double2(0.0, 0.0), p); continue; }
    double2 acc = make_double2(0.0, 0.0);
    for (int c = 0; c < p.C; c++) {
      double* s = state + ((size_t) u * p.C + c) * ss_chan_doubles(p.F);
      const float2 x = X[(((size_t) u * p.C + c) * p.Tmax + t) * p.F + f];
      const double a = alphas[c], X2 = (double) x.x * (double) x.x + (double) x.y * (double) x.y;
      if (a < 0) { s[p.F + f] += X2; if (f == 0) s[2 * p.F] += 1.0; }
      else if (s[2 * p.F + 1] == 0.0 && t == 0) s[f] = X2;                 // the first sample is copied (:104-107); `seen` is set after the call's first frame
      else s[f] = s[f] * a + X2 * (1.0 - a);
      if (out) { const double2 v = ss_bin(x, s[f], p); acc.x = v.x + acc.x; acc.y = v.y + acc.y; }
    }
    if (out) ss_store(out, row, f, make_double2(acc.x * inv, acc.y * inv), p);
  }
}
// after k_ss_train: every recursive channel of an utterance with at least one frame has seen its first sample
__global__ void k_ss_seen(const int* __restrict__ nframes, const double* __restrict__ alphas, double* __restrict__ state, SsPar p)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x; if (i >= p.U * p.C) return;
  const int u = i / p.C, c = i % p.C; const int nf = nframes ? nframes[u] : p.Tmax;
  if (nf > 0 && p.Tmax > 0 && alphas[c] >= 0) state[(size_t) i * ss_chan_doubles(p.F) + 2 * p.F + 1] = 1.0;
}

__global__ void __launch_bounds__(256) k_ss_apply(const float2* __restrict__ X, const int* __restrict__ nframes, const double* __restrict__ state,
                                                   void* __restrict__ out, SsPar p)
{
  const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x, n = (size_t) p.U * p.Tmax * p.F;
  if (i >= n) return;
  const int f = (int) (i % p.F); const size_t row = i / p.F; const int t = (int) (row % p.Tmax), u = (int) (row / p.Tmax);
  int nf = nframes ? nframes[u] : p.Tmax; nf = nf > p.Tmax ? p.Tmax : nf;
  double2 acc = make_double2(0.0, 0.0);
  if (t < nf) {
    for (int c = 0; c < p.C; c++) {
      const double est = state[((size_t) u * p.C + c) * ss_chan_doubles(p.F) + f];
      const double2 v = ss_bin(X[(((size_t) u * p.C + c) * p.Tmax + t) * p.F + f], est, p); acc.x = v.x + acc.x; acc.y = v.y + acc.y;
    }
    const double inv = 1.0 / (double) p.C; acc.x *= inv; acc.y *= inv;
  }
  ss_store(out, row, f, acc, p);
}
// rows of outBins == M: the bins ss_store does not reach (M/2 < f < M of frames past nframes are covered by the mirror of zeros; the
// Nyquist mirror does not exist) need no pass of their own; a zeroing memset runs before the kernels instead.

// what: 0 = stopTraining's average() (est = sum * (1/cnt) where alpha < 0), 1 = clearSamples (sum, cnt), 2 = clear (also `seen`),
// 3 = whole state to zero
__global__ void k_ss_state_op(double* __restrict__ state, const double* __restrict__ alphas, int UC, int C, int F, int what)
{
  const size_t per = ss_chan_doubles(F); const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x; if (i >= (size_t) UC * per) return;
  const int j = (int) (i % per); double* s = state + (i / per) * per; const int c = (int) ((i / per) % C);
  if (what == 3) { s[j] = 0.0; return; }
  if (what == 0) { if (j < F && alphas[c] < 0) s[j] = s[F + j] * (1.0 / s[2 * F]); return; }
  if ((j >= F && j <= 2 * F) || (what == 2 && j == 2 * F + 1)) s[j] = 0.0;
}

struct WnPar { int U, Tmax, F, M, outBins, outIsDouble, carry, update; double alpha, floorV, beta; };

// per utterance: PSDs[F], PSDn[F], cnt[F] (frames the object has seen; every bin's lane keeps its own copy, so no lane reads what another writes)
__global__ void __launch_bounds__(64) k_wiener(const float2* __restrict__ S, const float2* __restrict__ N, const int* __restrict__ nframes,
                                                double* __restrict__ state, void* __restrict__ out, WnPar p)
{
  const int f = blockIdx.x * 64 + threadIdx.x, u = blockIdx.y;
  if (f >= p.F) return;
  int nf = nframes ? nframes[u] : p.Tmax; nf = nf < 0 ? 0 : nf > p.Tmax ? p.Tmax : nf;
  double* st = state + (size_t) u * 3 * (size_t) p.F;
  double prevS = p.carry ? st[f] : 0.0, prevN = p.carry ? st[p.F + f] : 0.0;
  const long cnt0 = p.carry ? (long) st[2 * p.F + f] : 0;
  for (int t = 0; t < p.Tmax; t++) {
    const size_t row = (size_t) u * p.Tmax + t;
    double re = 0.0, im = 0.0;
    if (t < nf) {
      const float2 s = S[row * p.F + f];
      if (f == 0) { re = s.x; im = s.y; }
      else {
        const double a = (cnt0 + t) >= 2 ? p.alpha : 0.0;                  // _frameX > 0 (:302-305): -1 and 0 are the object's first two frames
        const double curS = (double) s.x * (double) s.x + (double) s.y * (double) s.y;
        const double PSDs = a * prevS + (1 - a) * curS;
        double PSDn = prevN;
        if (p.update) {
          const float2 n = N[row * p.F + f];
          double curN = (double) n.x * (double) n.x + (double) n.y * (double) n.y;
          if (curN < p.floorV) curN = p.floorV;
          PSDn = a * prevN + (1 - a) * curN; prevN = PSDn;
        }
        const double H = PSDs / (PSDs + p.beta * PSDn);
        re = (double) s.x * H; im = (double) s.y * H; prevS = PSDs;
        if (f == p.M / 2) im = -im;                                        // the only mirror written lands on the Nyquist bin itself (:330-331)
      }
    }
    store_c(out, row * p.outBins + f, re, im, p.outIsDouble);
  }
  if (nf > 0) { st[f] = prevS; st[p.F + f] = prevN; st[2 * p.F + f] = (double) (cnt0 + nf); }
}

void check_fft(int fftLen)
{
  if (fftLen < 4 || (fftLen & 1) || fftLen > 65536) throw Error(DSR_E_DIMENSION, "fftLen %d: an even length in [4, 65536] expected", fftLen);
}
size_t out_bytes(int U, int Tmax, int outBins, int isDouble) { return (size_t) U * Tmax * outBins * (isDouble ? 16 : 8); }

}  // namespace

struct dsr_specsub {
  int M = 0, F = 0, halfBandShift = 0; float ft = 1.0f, floorV = 0.001f; bool training = true, subtract = false;
  std::vector<double> alphas; DevBuf<double> d_alphas; bool dirty = true;
  void sync_alphas() { if (dirty) { require_device(); d_alphas.upload(alphas); dirty = false; } }
};
struct dsr_wiener {
  int M = 0, F = 0, halfBandShift = 0; float alpha = 0.0f, floorV = 0.001f, beta = 1.0f; bool update = true, carry = false;
};

extern "C" {

dsr_status dsr_psd_file_write(const char* fn, const double* est, int n)
{
  return guard([&] {
    if (!fn || !est || n < 0) throw Error(DSR_E_PARAMETER, "null argument");
    FILE* fp = fopen(fn, "w"); if (!fp) throw Error(DSR_E_IO, "could not write %s", fn);
    for (int i = 0; i < n; i++) fprintf(fp, "%lf\n", est[i]);
    fclose(fp);
  });
}
dsr_status dsr_psd_file_read(const char* fn, double* est, int n)
{
  return guard([&] {
    if (!fn || !est || n < 0) throw Error(DSR_E_PARAMETER, "null argument");
    FILE* fp = fopen(fn, "r"); if (!fp) throw Error(DSR_E_IO, "could not read %s", fn);
    for (int i = 0; i < n; i++) { double v = 0.0; if (fscanf(fp, "%lf\n", &v) != 1) v = i ? est[i - 1] : 0.0; est[i] = v; }   // a short file repeats the last value, as the reference's unset `val` does
    fclose(fp);
  });
}

dsr_status dsr_specsub_create(int fftLen, int halfBandShift, float ft, float flooringV, dsr_specsub** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    check_fft(fftLen);
    dsr_specsub* h = new dsr_specsub(); h->M = fftLen; h->F = fftLen / 2 + 1; h->halfBandShift = halfBandShift; h->ft = ft; h->floorV = flooringV; *out = h;
  });
}
void dsr_specsub_destroy(dsr_specsub* h) { delete h; }
dsr_status dsr_specsub_set_channel(dsr_specsub* h, double alpha)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->alphas.push_back(alpha); h->dirty = true; }); }
int dsr_specsub_chan_n(const dsr_specsub* h) { return h ? (int) h->alphas.size() : 0; }
int dsr_specsub_fft_len(const dsr_specsub* h) { return h ? h->M : 0; }
dsr_status dsr_specsub_set_noise_over_estimation_factor(dsr_specsub* h, float ft)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->ft = ft; }); }
dsr_status dsr_specsub_start_training(dsr_specsub* h) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->training = true; }); }
dsr_status dsr_specsub_set_noise_subtraction(dsr_specsub* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->subtract = on != 0; }); }
int dsr_specsub_is_training(const dsr_specsub* h) { return h && h->training; }
int dsr_specsub_is_subtracting(const dsr_specsub* h) { return h && h->subtract; }
size_t dsr_specsub_state_bytes(const dsr_specsub* h, int U) { return (h && U > 0) ? (size_t) U * h->alphas.size() * ss_chan_doubles(h->F) * 8 : 0; }

static void ss_state_op(dsr_specsub* h, void* state_dev, int U, int what, void* stream)
{
  if (!h || !state_dev || U <= 0) throw Error(DSR_E_PARAMETER, "null argument");
  const int C = (int) h->alphas.size(); if (C == 0) return;
  h->sync_alphas();
  const size_t n = (size_t) U * C * ss_chan_doubles(h->F);
  launch(k_ss_state_op, dim3(cdiv((long) n, 256)), dim3(256), 0, (hipStream_t) stream, (double*) state_dev, h->d_alphas.p, U * C, C, h->F, what);
}
dsr_status dsr_specsub_state_init(dsr_specsub* h, void* state_dev, int U, void* stream) { return guard([&] { ss_state_op(h, state_dev, U, 3, stream); }); }
dsr_status dsr_specsub_clear_noise_samples(dsr_specsub* h, void* state_dev, int U, void* stream) { return guard([&] { ss_state_op(h, state_dev, U, 1, stream); }); }
dsr_status dsr_specsub_clear(dsr_specsub* h, void* state_dev, int U, void* stream) { return guard([&] { ss_state_op(h, state_dev, U, 2, stream); }); }
dsr_status dsr_specsub_stop_training(dsr_specsub* h, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    h->training = false;                                                   // spectralsubtraction.h:87-91
    if (!state_dev || U <= 0) return;                                      // no state: the flag alone
    const int C = (int) h->alphas.size(); const size_t per = ss_chan_doubles(h->F);
    bool any = false; for (double a : h->alphas) any = any || a < 0; if (!any) return;
    require_device();
    DSR_HIP(hipStreamSynchronize((hipStream_t) stream));
    std::vector<double> cnts((size_t) U * C, 0.0);                           // one strided copy: the count of every (utterance, channel)
    DSR_HIP(hipMemcpy2D(cnts.data(), 8, (const double*) state_dev + 2 * h->F, per * 8, 8, (size_t) U * C, hipMemcpyDeviceToHost));
    for (int i = 0; i < U * C; i++) {
      if (h->alphas[i % C] >= 0) continue;
      if (cnts[i] == 0.0) throw Error(DSR_E_ARITHMETIC, "stopTraining: channel %d of utterance %d has no noise sample to average (the reference divides 0 by 0); the estimates are unchanged", i % C, i / C);
    }
    ss_state_op(h, state_dev, U, 0, stream);
  });
}
dsr_status dsr_specsub_apply(dsr_specsub* h, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, void* out_dev, int outBins, int outIsDouble,
                             void* state_dev, void* stream)
{
  return guard([&] {
    if (!h || !X_dev || !state_dev) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = (int) h->alphas.size();
    if (C < 1) throw Error(DSR_E_ERROR, "setChannel() has not been called");
    if (U < 0 || Tmax < 0 || (out_dev && outBins != h->F && outBins != h->M)) throw Error(DSR_E_DIMENSION, "outBins %d: fftLen/2+1 = %d or fftLen = %d expected", outBins, h->F, h->M);
    if (!out_dev && !h->training) return;
    if (U == 0 || Tmax == 0) return;
    require_device(); h->sync_alphas();
    hipStream_t st = (hipStream_t) stream;
    SsPar p{U, C, Tmax, h->F, h->M, out_dev ? outBins : h->F, outIsDouble, h->training, h->subtract, (double) h->ft, (double) h->floorV};
    if (out_dev && outBins == h->M) DSR_HIP(hipMemsetAsync(out_dev, 0, out_bytes(U, Tmax, outBins, outIsDouble), st));
    if (h->training) {
      launch(k_ss_train, dim3(cdiv(h->F, 64), U), dim3(64), 0, st, (const float2*) X_dev, nframes_dev, h->d_alphas.p, (double*) state_dev, out_dev, p);
      launch(k_ss_seen, dim3(cdiv(U * C, 64)), dim3(64), 0, st, nframes_dev, h->d_alphas.p, (double*) state_dev, p);
    } else
      launch(k_ss_apply, dim3(cdiv((long) U * Tmax * h->F, 256)), dim3(256), 0, st, (const float2*) X_dev, nframes_dev, (const double*) state_dev, out_dev, p);
  });
}
dsr_status dsr_specsub_state_read(const dsr_specsub* h, const void* state_dev, int U, int what, int u, int chan, double* host_out, size_t outDoubles)
{
  return guard([&] {
    if (!h || !state_dev || !host_out) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = (int) h->alphas.size();
    if (u < 0 || u >= U || chan < 0 || chan >= C) throw Error(DSR_E_INDEX, "utterance %d of %d, channel %d of %d", u, U, chan, C);
    if (what < 0 || what > 2) throw Error(DSR_E_PARAMETER, "what %d", what);
    const size_t n = what == 2 ? 2 : h->F; if (outDoubles < n) throw Error(DSR_E_DIMENSION, "%zu doubles for %zu", outDoubles, n);
    require_device(); DSR_HIP(hipDeviceSynchronize());
    const double* s = (const double*) state_dev + ((size_t) u * C + chan) * ss_chan_doubles(h->F);
    DSR_HIP(hipMemcpy(host_out, s + (what == 0 ? 0 : what == 1 ? h->F : 2 * h->F), n * 8, hipMemcpyDeviceToHost));
  });
}
dsr_status dsr_specsub_state_write_estimate(dsr_specsub* h, void* state_dev, int U, int u, int chan, const double* est)
{
  return guard([&] {
    if (!h || !state_dev || !est) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = (int) h->alphas.size();
    if (u < -1 || u >= U || chan < 0 || chan >= C) throw Error(DSR_E_INDEX, "utterance %d of %d, channel %d of %d", u, U, chan, C);   // vector::at (spectralsubtraction.h:113)
    require_device(); DSR_HIP(hipDeviceSynchronize());
    for (int v = (u < 0 ? 0 : u); v < (u < 0 ? U : u + 1); v++)
      DSR_HIP(hipMemcpy((double*) state_dev + ((size_t) v * C + chan) * ss_chan_doubles(h->F), est, (size_t) h->F * 8, hipMemcpyHostToDevice));
  });
}
dsr_status dsr_specsub_read_noise_file(dsr_specsub* h, const char* fn, int idx, void* state_dev, int U)
{
  if (h) h->training = false;                                              // before the file is opened (spectralsubtraction.h:111-114)
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    if (idx < 0 || idx >= (int) h->alphas.size()) throw Error(DSR_E_INDEX, "noise estimator %d of %zu", idx, h->alphas.size());
    std::vector<double> est(h->F, 0.0);
    dsr_status s = dsr_psd_file_read(fn, est.data(), h->F); if (s) throw Error(s, "%s", dsr_last_error());
    s = dsr_specsub_state_write_estimate(h, state_dev, U, -1, idx, est.data()); if (s) throw Error(s, "%s", dsr_last_error());
  });
}
dsr_status dsr_specsub_write_noise_file(const dsr_specsub* h, const char* fn, int idx, const void* state_dev, int U, int u)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    std::vector<double> est(h->F, 0.0);
    dsr_status s = dsr_specsub_state_read(h, state_dev, U, 0, u, idx, est.data(), est.size()); if (s) throw Error(s, "%s", dsr_last_error());
    s = dsr_psd_file_write(fn, est.data(), h->F); if (s) throw Error(s, "%s", dsr_last_error());
  });
}

dsr_status dsr_wiener_create(int fftLen, int noiseLen, int halfBandShift, float alpha, float flooringV, double beta, dsr_wiener** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    check_fft(fftLen);
    if (fftLen != noiseLen) throw Error(DSR_E_DIMENSION, "Input block length (%d) != fftLen (%d)", fftLen, noiseLen);   // spectralsubtraction.cc:278-281
    dsr_wiener* h = new dsr_wiener(); h->M = fftLen; h->F = fftLen / 2 + 1; h->halfBandShift = halfBandShift; h->alpha = alpha; h->floorV = flooringV;
    h->beta = (float) beta;                                                // the member is a float (spectralsubtraction.h:162)
    *out = h;
  });
}
void dsr_wiener_destroy(dsr_wiener* h) { delete h; }
dsr_status dsr_wiener_set_noise_amplification_factor(dsr_wiener* h, double beta) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->beta = (float) beta; }); }
dsr_status dsr_wiener_set_updating_noise_psd(dsr_wiener* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->update = on != 0; }); }
dsr_status dsr_wiener_carry(dsr_wiener* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->carry = on != 0; }); }
size_t dsr_wiener_state_bytes(const dsr_wiener* h, int U) { return (h && U > 0) ? (size_t) U * 3 * (size_t) h->F * 8 : 0; }
dsr_status dsr_wiener_reset_state(const dsr_wiener* h, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!h || !state_dev || U <= 0) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    const size_t n = (size_t) U * 3 * (size_t) h->F;
    DSR_HIP(hipMemsetAsync(state_dev, 0, n * 8, (hipStream_t) stream));
  });
}
dsr_status dsr_wiener_state_init(const dsr_wiener* h, void* state_dev, int U, void* stream) { return dsr_wiener_reset_state(h, state_dev, U, stream); }
dsr_status dsr_wiener_apply(dsr_wiener* h, const float* S_dev, const float* N_dev, const int32_t* nframes_dev, int U, int Tmax, void* out_dev, int outBins,
                            int outIsDouble, void* state_dev, void* stream)
{
  return guard([&] {
    if (!h || !S_dev || !out_dev || !state_dev || (h->update && !N_dev)) throw Error(DSR_E_PARAMETER, "null argument");
    if (h->halfBandShift) throw Error(DSR_E_ERROR, "WienerFilter::next() for the half band shift is not implemented");            // spectralsubtraction.cc:334-337
    if (U < 0 || Tmax < 0 || (outBins != h->F && outBins != h->M)) throw Error(DSR_E_DIMENSION, "outBins %d: fftLen/2+1 = %d or fftLen = %d expected", outBins, h->F, h->M);
    if (U == 0 || Tmax == 0) return;
    require_device();
    hipStream_t st = (hipStream_t) stream;
    WnPar p{U, Tmax, h->F, h->M, outBins, outIsDouble, h->carry, h->update, (double) h->alpha, (double) h->floorV, (double) h->beta};
    if (outBins == h->M) DSR_HIP(hipMemsetAsync(out_dev, 0, out_bytes(U, Tmax, outBins, outIsDouble), st));
    launch(k_wiener, dim3(cdiv(h->F, 64), U), dim3(64), 0, st, (const float2*) S_dev, (const float2*) N_dev, nframes_dev, (double*) state_dev, out_dev, p);
  });
}
dsr_status dsr_wiener_state_read(const dsr_wiener* h, const void* state_dev, int U, int what, int u, double* host_out, size_t outDoubles)
{
  return guard([&] {
    if (!h || !state_dev || !host_out) throw Error(DSR_E_PARAMETER, "null argument");
    if (u < 0 || u >= U) throw Error(DSR_E_INDEX, "utterance %d of %d", u, U);
    if (what < 0 || what > 2) throw Error(DSR_E_PARAMETER, "what %d", what);
    const size_t n = what == 2 ? 1 : h->F; if (outDoubles < n) throw Error(DSR_E_DIMENSION, "%zu doubles for %zu", outDoubles, n);
    require_device(); DSR_HIP(hipDeviceSynchronize());
    const double* s = (const double*) state_dev + (size_t) u * 3 * (size_t) h->F;
    DSR_HIP(hipMemcpy(host_out, s + (size_t) what * h->F, n * 8, hipMemcpyDeviceToHost));
  });
}

}  // extern "C"
