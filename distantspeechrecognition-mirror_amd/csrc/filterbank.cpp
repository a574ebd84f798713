// csrc/filterbank.cpp -- host side of the filter banks: plan construction, the state a bank carries between the blocks of a stream, and the
// dsr_fb_* / dsr_fb_state_* / dsr_prfb_* / dsr_stft_* entries (include/dsr.h).  Kernels, launch arithmetic and dispatch: k_filterbank.hip.
#include "filterbank.h"
#include "beamformer.h"
#include <cmath>

using namespace dsr;

struct dsr_fb : FbPlan {};
struct dsr_prfb : PrPlan {};
struct dsr_stft : StftPlan {};
// state a filter bank carries from one block of a stream to the next (dsr_fb_analysis_block / dsr_fb_synthesis_block)
struct dsr_fb_state { int U = 0, C = 0, H = 0, rowLen = 1; bool synthesis = false, started = false; long emitted = 0; int cur = 0; DevBuf<float> hist[2]; };

// tw[k] = e^{+2 pi j k / M}, computed in double
static std::vector<float2> twiddles(int M)
{
  std::vector<float2> tw(M);
  for (int k = 0; k < M; k++) { const double a = 2.0 * M_PI * (double) k / (double) M; tw[k] = make_float2((float) cos(a), (float) sin(a)); }
  return tw;
}

// a block is through the bank: the last H items of (history ++ block) go to the other buffer of the pair, which the next block reads
static void hand_over(dsr_fb_state* s, const float* blk, const int32_t* n, long blkRowStride, hipStream_t st)
{
  if (s->H > 0) {
    fb_hist_update(s->hist[s->cur].p, s->hist[s->cur ^ 1].p, blk, n, s->U * s->C, s->C, blkRowStride, s->H, s->rowLen, s->started, s->synthesis ? 64 : 0, st);
    s->cur ^= 1;
  }
  s->started = true;
}

extern "C" {

// PerfectReconstructionFFTAnalysisBank / SynthesisBank (modulated.cc:686-970)
dsr_status dsr_prfb_create(const double* prototype, int M, int m, int r, dsr_prfb** out)
{
  return guard([&] {
    if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    if (!is_pow2((unsigned) M) || M < 8 || M > 1024) throw Error(DSR_E_DIMENSION, "M=%d must be a power of two in [8,1024]", M);
    if (m < 1 || r < 0 || (M >> r) < 1) throw Error(DSR_E_DIMENSION, "bad m=%d r=%d", m, r);
    require_device();
    dsr_prfb* p = new dsr_prfb(); p->M = M; p->m = m; p->r = r; p->D = M >> r;
    const int M2 = 2 * M;
    std::vector<float> h((size_t) M2 * m); for (size_t i = 0; i < h.size(); i++) h[i] = (float) prototype[i];
    std::vector<float2> wA(M2), wS(M2);
    for (int i = 0; i < M2; i++) {
      const double b = M_PI * (double) i / (double) M2;
      wA[i] = make_float2((float) cos(b), (float) -sin(b)); wS[i] = make_float2((float) cos(b), (float) sin(b));
    }
    p->h.upload(h); p->tw.upload(twiddles(M2)); p->wA.upload(wA); p->wS.upload(wS);
    *out = p;
  });
}
void dsr_prfb_destroy(dsr_prfb* p) { delete p; }
int dsr_prfb_fft_len(const dsr_prfb* p) { return p ? 2 * p->M : 0; }
int dsr_prfb_block_len(const dsr_prfb* p) { return p ? p->D : 0; }
int dsr_prfb_analysis_frames(const dsr_prfb* p, int nsamp) { return p ? (nsamp + p->D - 1) / p->D + 2 * p->m - 1 : 0; }
int dsr_prfb_synthesis_blocks(const dsr_prfb* p, int nframes) { return (p && nframes > 2 * p->m - 1) ? nframes - (2 * p->m - 1) : 0; }
dsr_status dsr_prfb_analysis(const dsr_prfb* p, const float* x, const int32_t* nsamp_dev, int U, int C, int64_t sampStride, int Tmax, float* X, void* stream)
{
  return guard([&] {
    if (!p || !x || !nsamp_dev || !X) throw Error(DSR_E_PARAMETER, "null argument");
    if (U <= 0 || C <= 0 || Tmax <= 0) return;
    fb_pr_analysis(*p, x, nsamp_dev, U, C, (long) sampStride, Tmax, X, (hipStream_t) stream);
  });
}
dsr_status dsr_prfb_synthesis(dsr_prfb* p, const float* Y, const int32_t* nframes_dev, int U, int Tmax, int64_t outStride, float* y, void* stream)
{
  return guard([&] {
    if (!p || !Y || !nframes_dev || !y) throw Error(DSR_E_PARAMETER, "null argument");
    if (U <= 0 || Tmax <= 0 || outStride <= 0) return;
    fb_pr_synthesis(*p, Y, nframes_dev, U, Tmax, (long) outStride, y, (hipStream_t) stream);
  });
}

// NormalFFTAnalysisBank (modulated.cc:121-257): windowType 0 rectangle, 1 Hamming (default), 2 Hanning (getWindow, :72-97)
dsr_status dsr_stft_create(int M, int r, int windowType, dsr_stft** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (!is_pow2((unsigned) M) || M < 16 || M > 2048) throw Error(DSR_E_DIMENSION, "M=%d must be a power of two in [16,2048]", M);
    if (r < 0 || (M >> r) < 1) throw Error(DSR_E_DIMENSION, "bad r=%d", r);
    require_device();
    dsr_stft* p = new dsr_stft(); p->M = M; p->r = r; p->D = M >> r; p->winType = windowType;
    std::vector<float> w(M);
    for (int i = 0; i < M; i++) {
      double v;
      switch (windowType) {
      case 0: v = 1.0; break;
      case 2: v = 0.5 * (1 - cos((2.0 * M_PI * i) / (double) (M - 1))); break;
      default: { const double temp = 2. * M_PI / (double) (M - 1); v = 0.54 - 0.46 * cos(temp * i); } break;
      }
      w[i] = (float) v;
    }
    p->win.upload(w); p->tw.upload(twiddles(M));
    *out = p;
  });
}
void dsr_stft_destroy(dsr_stft* p) { delete p; }
int dsr_stft_frames(const dsr_stft* p, int nsamp) { return p ? (nsamp + p->D - 1) / p->D + 1 : 0; }
int dsr_stft_block_len(const dsr_stft* p) { return p ? p->D : 0; }
dsr_status dsr_stft_analysis(const dsr_stft* p, const float* x, const int32_t* nsamp_dev, int U, int C, int64_t sampStride, int Tmax,
                             float* X, void* stream)
{
  return guard([&] {
    if (!p || !x || !nsamp_dev || !X) throw Error(DSR_E_PARAMETER, "null argument");
    if (U <= 0 || C <= 0 || Tmax <= 0) return;
    fb_normal_fft(*p, x, nsamp_dev, U, C, (long) sampStride, Tmax, X, (hipStream_t) stream);
  });
}

dsr_status dsr_fb_create(const double* prototype, int M, int m, int r, int synthesis, int dctype, int gain, dsr_fb** out)
{
  return guard([&] {
    if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    if (!is_pow2((unsigned) M) || M < 16 || M > 2048) throw Error(DSR_E_DIMENSION, "M=%d must be a power of two in [16,2048]", M);
    if (m < 1 || r < 0 || (M >> r) < 1) throw Error(DSR_E_DIMENSION, "bad m=%d r=%d", m, r);
    require_device();
    dsr_fb* p = new dsr_fb();
    p->M = M; p->m = m; p->r = r; p->R = 1 << r; p->D = M >> r; p->synthesis = synthesis; p->dctype = dctype; p->gain = gain;
    // modulated.cc:279-296
    p->laN = 0;
    switch (dctype) {
    case 1: p->pd = m * p->R - 1; break;
    case 2: if (synthesis) p->pd = m * p->R / 2; else { p->pd = m * p->R - 1; p->laN = m * p->R / 2 - 1; } break;
    default: p->pd = 2 * m - 1; break;
    }
    p->proto.assign(prototype, prototype + (size_t) m * M);
    std::vector<float> pf((size_t) m * M); for (size_t i = 0; i < pf.size(); i++) pf[i] = (float) prototype[i];
    p->d_proto.upload(pf); p->d_tw.upload(twiddles(M));
    *out = p;
  });
}
void dsr_fb_destroy(dsr_fb* p) { delete p; }
int dsr_fb_analysis_frames(const dsr_fb* p, int nsamp) { return fb_frames(nsamp, p->D, p->laN, p->pd); }
int dsr_fb_synthesis_blocks(const dsr_fb* p, int nframes) { return nframes - p->pd > 0 ? nframes - p->pd : 0; }
int dsr_fb_processing_delay(const dsr_fb* p) { return p->pd; }
int dsr_fb_block_len(const dsr_fb* p) { return p->D; }

dsr_status dsr_fb_analysis(const dsr_fb* p, const float* x, const int32_t* nsamp, int U, int C, int64_t sampStride,
                           int Tmax, float* X, void* stream)
{
  return guard([&] {
    if (!p || !x || !nsamp || !X) throw Error(DSR_E_PARAMETER, "null argument");
    if (p->synthesis) throw Error(DSR_E_CONSISTENCY, "plan was created for synthesis");
    if (U <= 0 || C <= 0 || Tmax <= 0) return;
    if (C > 65535 || U > 65535) throw Error(DSR_E_DIMENSION, "U and C must be <= 65535 per call");
    const FbCall k = { p->pd, p->laN, nullptr, 0, 0 };
    fb_analysis(*p, k, x, nsamp, U, C, (long) sampStride, Tmax, X, (hipStream_t) stream);
  });
}
int dsr_fb_analysis_beamform_supported(const dsr_fb* p, const dsr_bf* bf)
{
  if (!p || !bf || p->synthesis || getenv("DSR_FB_GENERIC") || getenv("DSR_FB_WAVE") || getenv("DSR_FB_NOFUSE")) return 0;
  if (!(p->M == 256 && p->r == 1 && (p->m == 2 || p->m == 4))) return 0;
  const int C = dsr_bf_chan_n(bf);
  return (dsr_bf_fft_len(bf) == p->M && !dsr_bf_half_band_shift(bf) && !dsr_bf_is_adaptive(bf) && C >= 1 && C <= 16) ? 1 : 0;
}
dsr_status dsr_fb_analysis_beamform(const dsr_fb* p, dsr_bf* bf, const float* x, const int32_t* nsamp, int U, int C, int64_t sampStride,
                                    int Tmax, float* Y, void* stream)
{
  return guard([&] {
    if (!p || !bf || !x || !nsamp || !Y) throw Error(DSR_E_PARAMETER, "null argument");
    if (!dsr_fb_analysis_beamform_supported(p, bf)) throw Error(DSR_E_PARAMETER, "analysis + beamformer in one pass needs M = 256, r = 1, m in {2, 4}, at most 16 channels and fixed weights");
    if (C != dsr_bf_chan_n(bf)) throw Error(DSR_E_DIMENSION, "beamformer has %d channels, input has %d", dsr_bf_chan_n(bf), C);
    if (U <= 0 || Tmax <= 0) return;
    if (U > 65535) throw Error(DSR_E_DIMENSION, "U must be <= 65535 per call");
    const float2* W = bf_fixed_weights_dev(bf);
    if (!W) throw Error(DSR_E_CONSISTENCY, "the beamformer has no fixed weights");
    fb_analysis_beamform(*p, W, x, nsamp, U, C, (long) sampStride, Tmax, Y, (hipStream_t) stream);
  });
}
dsr_status dsr_fb_synthesis(const dsr_fb* p, const float* Y, const int32_t* nframes, int U, int Tmax,
                            int64_t outStride, float* y, void* stream)
{
  return guard([&] {
    if (!p || !Y || !nframes || !y) throw Error(DSR_E_PARAMETER, "null argument");
    if (!p->synthesis) throw Error(DSR_E_CONSISTENCY, "plan was created for analysis");
    if (U <= 0 || Tmax <= 0 || outStride <= 0) return;
    if (U > 65535) throw Error(DSR_E_DIMENSION, "U must be <= 65535 per call");
    const FbCall k = { p->pd, 0, nullptr, 0, 0 };
    fb_synthesis(*p, k, Y, nframes, U, Tmax, (long) outStride, y, (hipStream_t) stream);
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Block-wise processing of long streams (BASELINE configs[4]: 10-minute streams in 10-second blocks).  The reference operators keep ring buffers
// of the last m*M samples (analysis, modulated.h:79-163, modulated.cc:400-452) and of the last R*m subband frames (synthesis, :586-664); here
// a state object carries exactly those between calls: m*M - D samples per (stream, channel), R*m - 1 subband frames per stream.
dsr_status dsr_fb_state_create(const dsr_fb* p, int U, int C, dsr_fb_state** out)
{
  return guard([&] {
    if (!p || !out || U < 1 || (!p->synthesis && C < 1)) throw Error(DSR_E_PARAMETER, "bad argument");
    require_device();
    dsr_fb_state* s = new dsr_fb_state(); s->U = U; s->synthesis = p->synthesis != 0;
    if (p->synthesis) { s->C = 1; s->H = p->R * p->m - 1; s->rowLen = 2 * (p->M / 2 + 1); }
    else { s->C = C; s->H = p->m * p->M - p->D; s->rowLen = 1; }
    const size_t n = (size_t) U * s->C * (s->H > 0 ? s->H : 1) * s->rowLen;
    s->hist[0].reserve(n); s->hist[1].reserve(n);
    *out = s;
  });
}
void dsr_fb_state_destroy(dsr_fb_state* s) { delete s; }
dsr_status dsr_fb_state_reset(dsr_fb_state* s)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->started = false; s->emitted = 0; }); }

// frames a block of nsampBlock new samples yields: the stream's first block spends the look-ahead (laN source blocks, delayCompensationType 2,
// modulated.cc:467-474), its last one adds the processingDelay zero-input frames (:493-501)
int dsr_fb_analysis_block_frames(const dsr_fb* p, const dsr_fb_state* s, int nsampBlock, int last)
{
  if (!p || !s) return 0;
  return fb_frames(nsampBlock, p->D, s->started ? 0 : p->laN, last ? p->pd : 0);
}
dsr_status dsr_fb_analysis_block(const dsr_fb* p, dsr_fb_state* s, const float* x, const int32_t* nsamp_dev, int U, int C, int64_t sampStride,
                                 int last, int Tmax, float* X, void* stream)
{
  return guard([&] {
    if (!p || !s || !x || !nsamp_dev || !X) throw Error(DSR_E_PARAMETER, "null argument");
    if (p->synthesis || s->synthesis) throw Error(DSR_E_CONSISTENCY, "plan / state were created for synthesis");
    if (U != s->U || C != s->C) throw Error(DSR_E_DIMENSION, "state holds %d x %d rows, call has %d x %d", s->U, s->C, U, C);
    if (s->H != p->m * p->M - p->D) throw Error(DSR_E_CONSISTENCY, "state belongs to another filter bank");
    if (Tmax <= 0) return;
    hipStream_t st = (hipStream_t) stream;
    const FbCall k = { last ? p->pd : 0, s->started ? 0 : p->laN, s->started ? s->hist[s->cur].p : nullptr, s->H, 0 };
    fb_analysis(*p, k, x, nsamp_dev, U, C, (long) sampStride, Tmax, X, st);
    hand_over(s, x, nsamp_dev, (long) sampStride, st);
  });
}
// output blocks a call with nframesBlock new subband frames yields: the first call keeps processingDelay frames of look-ahead back (modulated.cc:631-634)
int dsr_fb_synthesis_block_blocks(const dsr_fb* p, const dsr_fb_state* s, int nframesBlock)
{
  if (!p || !s) return 0;
  if (s->started) return nframesBlock;
  return nframesBlock - p->pd > 0 ? nframesBlock - p->pd : 0;
}
dsr_status dsr_fb_synthesis_block(const dsr_fb* p, dsr_fb_state* s, const float* Y, const int32_t* nframes_dev, int nframesHostMax, int U, int Tmax,
                                  int64_t outStride, float* y, void* stream)
{
  return guard([&] {
    if (!p || !s || !Y || !nframes_dev || !y) throw Error(DSR_E_PARAMETER, "null argument");
    if (!p->synthesis || !s->synthesis) throw Error(DSR_E_CONSISTENCY, "plan / state were created for analysis");
    if (U != s->U) throw Error(DSR_E_DIMENSION, "state holds %d streams, call has %d", s->U, U);
    if (s->H != p->R * p->m - 1) throw Error(DSR_E_CONSISTENCY, "state belongs to another filter bank");
    if (Tmax <= 0 || outStride <= 0) return;
    if (!s->started && nframesHostMax < p->pd + p->R * p->m) throw Error(DSR_E_DIMENSION, "the first block of a stream must hold at least %d subband frames", p->pd + p->R * p->m);
    hipStream_t st = (hipStream_t) stream;
    // later calls: local frame tau = absolute frame minus the frames of the calls before; the look-ahead is already inside the history shift
    const FbCall k = { s->started ? 0 : p->pd, 0, s->started ? s->hist[s->cur].p : nullptr, s->H, s->started ? -(p->R - 1) : 0 };
    fb_synthesis(*p, k, Y, nframes_dev, U, Tmax, (long) outStride, y, st);
    hand_over(s, Y, nframes_dev, (long) Tmax * s->rowLen, st);
  });
}

}  // extern "C"
