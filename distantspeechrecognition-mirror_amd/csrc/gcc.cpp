// csrc/gcc.cpp -- host side of pairwise time-delay estimation, include/dsr.h section 2e (kernels: csrc/k_gcc.hip; what the two share: csrc/gcc.h):
// handle construction, the per-call face (GCC::calculate / findMaximum / the getters on the handle's own one-utterance state), the state readers,
// the channel delays from the pair delays, and the dsr_gcc_* / dsr_cctde_* entries.
#include "gcc.h"
#include <cmath>

using namespace dsr;

namespace {

// dsr_gcc_run and dsr_gcc_calculate: the checks, then the launches
void gcc_run(dsr_gcc* g, const void* X_dev, int xIsDouble, const int32_t* nframes_dev, const int32_t* sad_dev, const double* timestamp_dev, int smooth,
             double minDelay, double maxDelay, int U, int Tmax, void* state_dev, double* result_dev, int32_t* valid_dev, double* corr_dev,
             void* xspec_dev, void* stream, int active, int ac1, int ac2)
{
  if (!g || !X_dev || !sad_dev || !timestamp_dev || !state_dev || !result_dev || !valid_dev) throw Error(DSR_E_PARAMETER, "null argument");
  if (U < 1 || Tmax < 0) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d Tmax=%d", U, Tmax);
  require_device();
  if (Tmax == 0) return;
  gcc_launch_run(g, X_dev, xIsDouble, nframes_dev, sad_dev, timestamp_dev, smooth, minDelay, maxDelay, U, Tmax, state_dev, result_dev, valid_dev, corr_dev, xspec_dev,
                 (hipStream_t) stream, active, ac1, ac2);
}

void own_state(dsr_gcc* g)
{
  if (g->ownReady) return;
  require_device();
  const size_t n = glayout(*g, 1).doubles;
  g->ownState.reserve(n); g->ownX.reserve((size_t) g->C * g->len * 2); g->ownTs.reserve(1); g->ownSad.reserve(1); g->ownRes.reserve((size_t) g->P * 3); g->ownValid.reserve(g->P);
  DSR_HIP(hipMemset(g->ownState.p, 0, n * 8)); DSR_HIP(hipMemset(g->ownX.p, 0, (size_t) g->C * g->len * 16));
  g->ownReady = true;
}

}  // namespace

extern "C" {

dsr_status dsr_gcc_create(int kind, double sampleRate, int fftLen, int chanN, const int32_t* pairs, int pairsN, double alpha, double beta, double q,
                          int interpolate, int noisereduction, dsr_gcc** out)
{
  return guard([&] {
    if (!out || !pairs) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < DSR_GCC_RAW || kind > DSR_GCC_MLRGNNSUB) throw Error(DSR_E_PARAMETER, "unknown GCC kind %d", kind);
    if (fftLen < 8 || fftLen > 4096 || !is_pow2((unsigned) fftLen)) throw Error(DSR_E_DIMENSION, "fftLen %d: a power of two in [8, 4096] is needed", fftLen);
    if (chanN < 1 || pairsN < 1) throw Error(DSR_E_DIMENSION, "chanN %d, pairs %d: at least one of each is needed", chanN, pairsN);
    if (!(sampleRate > 0.0)) throw Error(DSR_E_PARAMETER, "sampleRate %g", sampleRate);
    dsr_gcc* g = new dsr_gcc(); std::unique_ptr<dsr_gcc> hold(g);
    g->kind = kind; g->N = fftLen; g->len = fftLen / 2 + 1; g->C = chanN; g->P = pairsN; g->interpolate = interpolate != 0; g->noisereduction = noisereduction != 0;
    g->sampleRate = sampleRate; g->alpha = alpha; g->beta = beta; g->q = q;
    g->pairs.assign(pairs, pairs + 2 * (size_t) pairsN); g->inPair.assign(chanN, 0);
    for (int i = 0; i < 2 * pairsN; i++) {
      if (pairs[i] < 0 || pairs[i] >= chanN) throw Error(DSR_E_INDEX, "pair %d names channel %d of %d", i / 2, pairs[i], chanN);
      g->inPair[pairs[i]] = 1;
    }
    *out = hold.release();
  });
}
void dsr_gcc_destroy(dsr_gcc* g) { delete g; }
dsr_status dsr_gcc_set_alpha(dsr_gcc* g, double alpha) { return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->alpha = alpha; }); }
double dsr_gcc_alpha(const dsr_gcc* g) { return g ? g->alpha : 0.0; }
dsr_status dsr_gcc_set_timing(dsr_gcc* g, int on)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null argument");
    g->tm.enable(on != 0);
  });
}
dsr_status dsr_gcc_kernel_ms(const dsr_gcc* g, double* ms2)
{
  return guard([&] {
    if (!g || !ms2 || !g->tm.on) throw Error(DSR_E_PARAMETER, "timing is off");
    g->tm.wait(3); ms2[0] = g->tm.ms(0, 1); ms2[1] = g->tm.ms(2, 3);
  });
}
int dsr_gcc_fft_len(const dsr_gcc* g) { return g ? g->N : 0; }
int dsr_gcc_pairs_n(const dsr_gcc* g) { return g ? g->P : 0; }
int dsr_gcc_chan_n(const dsr_gcc* g) { return g ? g->C : 0; }

size_t dsr_gcc_state_bytes(const dsr_gcc* g, int U) { return (g && U > 0) ? glayout(*g, U).doubles * 8 : 0; }

dsr_status dsr_gcc_state_init(const dsr_gcc* g, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!g || !state_dev || U < 1) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    gcc_launch_state_init((double*) state_dev, glayout(*g, U).doubles, (hipStream_t) stream);
  });
}

dsr_status dsr_gcc_find_maximum(dsr_gcc* g, double minDelay, double maxDelay, int U, const void* state_dev, double* result_dev, int32_t* valid_dev, void* stream)
{
  return guard([&] {
    if (!g || !state_dev || !result_dev || !valid_dev || U < 1) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    gcc_launch_find_maximum(*g, minDelay, maxDelay, U, (void*) state_dev, result_dev, valid_dev, (hipStream_t) stream);
  });
}

dsr_status dsr_gcc_run(dsr_gcc* g, const void* X_dev, int xIsDouble, const int32_t* nframes_dev, const int32_t* sad_dev, const double* timestamp_dev, int smooth,
                       double minDelay, double maxDelay, int U, int Tmax, void* state_dev, double* result_dev, int32_t* valid_dev, double* corr_dev,
                       void* xspec_dev, void* stream)
{
  return guard([&] {
    gcc_run(g, X_dev, xIsDouble, nframes_dev, sad_dev, timestamp_dev, smooth, minDelay, maxDelay, U, Tmax, state_dev, result_dev, valid_dev, corr_dev, xspec_dev,
            stream, -1, -1, -1);
  });
}

// ---- the per-call face: GCC::calculate / findMaximum / the getters on the handle's own one-utterance state, host data in and out ----------
dsr_status dsr_gcc_calculate(dsr_gcc* g, const double* spec1, int n1, int chan1, const double* spec2, int n2, int chan2, int pair, double timestamp, int sad, int smooth)
{
  return guard([&] {
    if (!g || !spec1 || !spec2) throw Error(DSR_E_PARAMETER, "null argument");
    if (pair < 0 || pair >= g->P) throw Error(DSR_E_INDEX, "pair %d of %d", pair, g->P);
    if (chan1 < 0 || chan1 >= g->C || chan2 < 0 || chan2 >= g->C) throw Error(DSR_E_INDEX, "pair %d names channels %d, %d of %d", pair, chan1, chan2, g->C);
    if (sad && n1 != g->N) throw Error(DSR_E_DIMENSION, "FFT length of spectralSample1 (%d) does not match %d.", n1, g->N);     // localization.cc:1266-1269
    if (n1 < g->len || n2 < g->len) throw Error(DSR_E_DIMENSION, "a spectrum of %d and one of %d bins, %d are needed", n1, n2, g->len);
    own_state(g);
    const size_t row = (size_t) g->len * 2;
    DSR_HIP(hipMemcpy(g->ownX.p + chan1 * row, spec1, row * 8, hipMemcpyHostToDevice));
    if (chan2 != chan1) DSR_HIP(hipMemcpy(g->ownX.p + chan2 * row, spec2, row * 8, hipMemcpyHostToDevice));
    const int s01 = sad != 0;
    DSR_HIP(hipMemcpy(g->ownSad.p, &s01, sizeof(int), hipMemcpyHostToDevice)); DSR_HIP(hipMemcpy(g->ownTs.p, &timestamp, 8, hipMemcpyHostToDevice));
    gcc_run(g, g->ownX.p, 1, nullptr, g->ownSad.p, g->ownTs.p, smooth, -HUGE_D, HUGE_D, 1, 1, g->ownState.p, g->ownRes.p, g->ownValid.p, nullptr, nullptr, nullptr,
            pair, chan1, chan2);
    DSR_HIP(hipStreamSynchronize(nullptr));
  });
}

dsr_status dsr_gcc_peak(dsr_gcc* g, int pair, double minDelay, double maxDelay, double* out3, int32_t* valid)
{
  return guard([&] {
    if (!g || !out3) throw Error(DSR_E_PARAMETER, "null argument");
    if (pair < 0 || pair >= g->P) throw Error(DSR_E_INDEX, "pair %d of %d", pair, g->P);
    own_state(g);
    const dsr_status st = dsr_gcc_find_maximum(g, minDelay, maxDelay, 1, g->ownState.p, g->ownRes.p, g->ownValid.p, nullptr);
    if (st != DSR_OK) throw Error(st, "%s", dsr_last_error());
    int v = 0;
    DSR_HIP(hipMemcpy(out3, g->ownRes.p + (size_t) pair * 3, 24, hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(&v, g->ownValid.p + pair, sizeof(int), hipMemcpyDeviceToHost));
    if (valid) *valid = v;
  });
}

dsr_status dsr_gcc_get(dsr_gcc* g, int what, int index, double* host_out, size_t outDoubles, int32_t* exists)
{
  if (!g) return guard([&] { throw Error(DSR_E_PARAMETER, "null argument"); });
  const dsr_status st = guard([&] { own_state(g); });
  return st != DSR_OK ? st : dsr_gcc_state_read(g, g->ownState.p, 1, what, 0, index, host_out, outDoubles, exists);
}

dsr_status dsr_gcc_state_read(const dsr_gcc* g, const void* state_dev, int U, int what, int u, int index, double* host_out, size_t outDoubles, int32_t* exists)
{
  return guard([&] {
    if (!g || !state_dev || !host_out || U < 1) throw Error(DSR_E_PARAMETER, "null argument");
    if (u < 0 || u >= U) throw Error(DSR_E_INDEX, "utterance %d of %d", u, U);
    const bool chan = what == DSR_GCC_STATE_NOISE_POWER;
    if (what < DSR_GCC_STATE_NOISE_POWER || what > DSR_GCC_STATE_CORRELATION) throw Error(DSR_E_PARAMETER, "unknown state part %d", what);
    if (index < 0 || index >= (chan ? g->C : g->P)) throw Error(DSR_E_INDEX, "%s %d of %d", chan ? "channel" : "pair", index, chan ? g->C : g->P);
    const GLayout l = glayout(*g, U); const size_t len = (size_t) g->len, N = (size_t) g->N;
    const size_t uc = (size_t) u * g->C + index, up = (size_t) u * g->P + index;
    size_t off, n, flag;
    switch (what) {
      case DSR_GCC_STATE_NOISE_POWER: off = l.Np + uc * len; n = len; flag = l.hasN + uc; break;
      case DSR_GCC_STATE_NOISE_CROSS: off = l.Gn + up * len * 2; n = len * 2; flag = l.hasG + up; break;
      case DSR_GCC_STATE_CROSS: off = l.S + up * len * 2; n = len * 2; flag = l.hasC + up; break;
      default: off = l.corr + up * N; n = N; flag = l.hasC + up; break;
    }
    if (outDoubles < n) throw Error(DSR_E_DIMENSION, "state part %d needs %zu doubles, the buffer holds %zu", what, n, outDoubles);
    require_device();
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(host_out, (const double*) state_dev + off, n * 8, hipMemcpyDeviceToHost));
    double f = 0.0; DSR_HIP(hipMemcpy(&f, (const double*) state_dev + flag, 8, hipMemcpyDeviceToHost));
    if (exists) *exists = f != 0.0;
  });
}

// tau with tau_0 = 0 from d_p = tau_c1 - tau_c2: the normal equations of the pair graph (its Laplacian without row and column 0)
dsr_status dsr_gcc_channel_delays(const dsr_gcc* g, const double* pairDelays, double* delays)
{
  return guard([&] {
    if (!g || !pairDelays || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = g->C, P = g->P, n = C - 1;
    std::vector<int> comp(C); for (int c = 0; c < C; c++) comp[c] = c;
    auto root = [&](int c) { while (comp[c] != c) c = comp[c] = comp[comp[c]]; return c; };
    for (int p = 0; p < P; p++) comp[root(g->pairs[2 * p])] = root(g->pairs[2 * p + 1]);
    for (int c = 1; c < C; c++) if (root(c) != root(0)) throw Error(DSR_E_PARAMETER, "the pair graph is not connected: channel %d cannot be reached from channel 0", c);
    delays[0] = 0.0; if (n == 0) return;
    std::vector<double> A((size_t) n * n, 0.0), b(n, 0.0);
    for (int p = 0; p < P; p++) {
      const int i = g->pairs[2 * p] - 1, j = g->pairs[2 * p + 1] - 1; const double d = pairDelays[p];
      if (i == j) continue;
      if (i >= 0) { A[(size_t) i * n + i] += 1.0; b[i] += d; }
      if (j >= 0) { A[(size_t) j * n + j] += 1.0; b[j] -= d; }
      if (i >= 0 && j >= 0) { A[(size_t) i * n + j] -= 1.0; A[(size_t) j * n + i] -= 1.0; }
    }
    for (int k = 0; k < n; k++) {                                                                      // Gaussian elimination, partial pivoting
      int piv = k; for (int r = k + 1; r < n; r++) if (std::fabs(A[(size_t) r * n + k]) > std::fabs(A[(size_t) piv * n + k])) piv = r;
      if (A[(size_t) piv * n + k] == 0.0) throw Error(DSR_E_NUMERIC, "singular pair graph");
      if (piv != k) { for (int c = 0; c < n; c++) std::swap(A[(size_t) k * n + c], A[(size_t) piv * n + c]); std::swap(b[k], b[piv]); }
      for (int r = k + 1; r < n; r++) {
        const double m = A[(size_t) r * n + k] / A[(size_t) k * n + k]; if (m == 0.0) continue;
        for (int c = k; c < n; c++) A[(size_t) r * n + c] -= m * A[(size_t) k * n + c];
        b[r] -= m * b[k];
      }
    }
    for (int k = n - 1; k >= 0; k--) { double v = b[k]; for (int c = k + 1; c < n; c++) v -= A[(size_t) k * n + c] * delays[c + 1]; delays[k + 1] = v / A[(size_t) k * n + k]; }
  });
}

dsr_status dsr_cctde_check(int fftLen, int nHeldMaxCC)
{
  return guard([&] {
    if (fftLen < 8 || fftLen > CC_FFT_MAX || !is_pow2((unsigned) fftLen)) throw Error(DSR_E_DIMENSION, "fftLen %d: a power of two in [8, %d] is needed", fftLen, CC_FFT_MAX);
    if (nHeldMaxCC < 1 || nHeldMaxCC >= fftLen)
      throw Error(DSR_E_DIMENSION, "The number of the held cross-correlation coefficients should be less than the FFT length but %d > %d", nHeldMaxCC, fftLen);
  });
}

dsr_status dsr_cctde_run(const float* a_dev, const float* b_dev, int nItems, int blockLen, int fftLen, int nHeldMaxCC, int sampleRate, double* delays_dev,
                         int32_t* args_dev, double* values_dev, void* stream)
{
  return guard([&] {
    if (!a_dev || !b_dev || !delays_dev || !args_dev || !values_dev) throw Error(DSR_E_PARAMETER, "null argument");
    const dsr_status cs = dsr_cctde_check(fftLen, nHeldMaxCC); if (cs != DSR_OK) throw Error(cs, "%s", dsr_last_error());
    if (blockLen < 1 || blockLen > fftLen) throw Error(DSR_E_DIMENSION, "block length %d outside [1, fftLen = %d]", blockLen, fftLen);
    if (sampleRate <= 0 || nItems < 0) throw Error(DSR_E_PARAMETER, "sampleRate %d, %d block pairs", sampleRate, nItems);
    require_device();
    if (nItems == 0) return;
    cctde_launch(a_dev, b_dev, nItems, blockLen, fftLen, nHeldMaxCC, sampleRate, delays_dev, args_dev, values_dev, (hipStream_t) stream);
  });
}

}  // extern "C"
