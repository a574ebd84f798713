// csrc/streams.cpp -- the stream/feature-operator API (include/dsr.h section 7).
//
// Mirrors FeatureStream<Type,item_type> (btk/stream/stream.h:36-75): reference-counted operators that
// hold their upstream(s), `next(frameX)` / `reset()` / `size()` / `name()` / `current()` / `isEnd()`,
// `frameX == -5` meaning "next", FrameResetX = -1, end of stream signalled as JITERATOR.
//
// The reference pulls one frame at a time through virtual calls; here an operator materialises its whole
// utterance on the device at the first next() after a reset() (every source of the path holds the full
// utterance in memory: SampleFeature::_samples, feature.cc:300-340) and then serves rows of its own
// host-side output buffer.  Compute always runs on the GPU (k_ops.hip / k_filterbank.hip / k_beamform.hip).
#include "common.h"
#include "ops.h"
#include "lattice.h"
#include "srp_common.h"
#include <cmath>

using namespace dsr;

struct dsr_stream {
  int refs = 1; std::string name; int size_ = 0; int type = DSR_T_FLOAT; int frameX = -1; bool endOfSamples = false;
  std::vector<dsr_stream*> ups;
  bool ready = false; int nFrames = 0;
  DevBuf<unsigned char> dev; std::vector<unsigned char> host;
  bool checkOrder = true;            // feature.cc operators throw jindex_error on out-of-order requests
  bool randomAccess = false;         // StorageFeature
  virtual ~dsr_stream() { for (size_t i = 0; i < ups.size(); i++) dsr_stream_release(ups[i]); }
  size_t itemsize() const { return type == DSR_T_CHAR ? 1 : type == DSR_T_SHORT ? 2 : type == DSR_T_FLOAT ? 4 : type == DSR_T_DOUBLE ? 8 : 16; }
  size_t rowBytes() const { return (size_t) size_ * itemsize(); }
  virtual void compute() = 0;        // fills dev (nFrames rows)
  virtual void reset() { frameX = -1; endOfSamples = false; ready = false; for (size_t i = 0; i < ups.size(); i++) ups[i]->reset(); }
  void add_up(dsr_stream* u) { dsr_stream_retain(u); ups.push_back(u); }
  void materialize() {
    if (ready) return;
    require_device();
    for (size_t i = 0; i < ups.size(); i++) ups[i]->materialize();
    compute();
    host.assign((size_t) nFrames * rowBytes() + 16, 0);
    if (nFrames > 0) { DSR_HIP(hipMemcpy(host.data(), dev.p, (size_t) nFrames * rowBytes(), hipMemcpyDeviceToHost)); }
    ready = true;
  }
  const void* row(int t) const { return host.data() + (size_t) t * rowBytes(); }
  virtual const void* next(int fx) {
    if (fx == frameX && frameX >= 0) return row(frameX);
    if (randomAccess && fx >= 0 && fx <= frameX) return row(fx);
    if (checkOrder && fx >= 0 && fx - 1 != frameX) throw Error(DSR_E_INDEX, "Problem in Feature %s: %d != %d", name.c_str(), fx - 1, frameX);
    materialize();
    if (frameX + 1 >= nFrames) { endOfSamples = true; throw Error(DSR_E_ITERATOR, "end of samples!"); }
    frameX++;
    return row(frameX);
  }
  template <class T> T* d() { return reinterpret_cast<T*>(dev.p); }
  void alloc(int T) { nFrames = T; dev.reserve((size_t) (T > 0 ? T : 1) * rowBytes()); }
};

namespace {

hipStream_t S0 = nullptr;

void ok(dsr_status s) { if (s) throw Error(s, "%s", dsr_last_error()); }      // a failed call of the library's own C-ABI: its status and message go on

// the frame count of the shortest of the C upstreams from `first` on (the reference's loops end with the first channel that ends)
int shortest(const dsr_stream* s, int first, int C)
{
  int T = s->ups[first]->nFrames;
  for (int c = 1; c < C; c++) if (s->ups[first + c]->nFrames < T) T = s->ups[first + c]->nFrames;
  return T;
}
// X [C][T][F] complex64: bins 0..F-1 of the first T frames (M bins each) of the C upstreams from `first` on
void pack_channels(const dsr_stream* s, int first, int C, int T, int F, int M, float2* X)
{
  for (int c = 0; c < C; c++) op_pack_bins(s->ups[first + c]->d<double2>(), T, F, M, X + (size_t) c * T * F, S0);
}

struct SampleSrc : dsr_stream {      // SampleFeature (feature.cc:222-689)
  int blockLen, shiftLen, padZeros; std::vector<float> samples; DevBuf<float> dx; int sampleRate = 16000, nChan = 1;
  void compute() override {
    const int n = (int) samples.size(); int T;
    if (padZeros) T = (n + shiftLen - 1) / shiftLen; else { long a = (long) n - blockLen; T = a > 0 ? (int) ((a + shiftLen - 1) / shiftLen) : 0; }
    dx.upload(samples.data(), samples.size() ? samples.size() : 0); if (!dx.p) dx.reserve(1);
    alloc(T); op_frames(dx.p, n, T, blockLen, shiftLen, d<float>(), S0);
  }
};
struct FrameSrc : dsr_stream {       // PyFeatureStream-like source: the caller hands over all frames (pyStream.h:44-130)
  std::vector<unsigned char> frames; int T = 0;
  // PyFeatureStream::reset() calls the Python object's reset() and starts a new iteration (pyStream.h:100-130).  A reset() that reaches this
  // source through a downstream operator's cascade marks the frames stale; the owner's refill callback (it calls the Python reset() and hands
  // the new frames over with dsr_frame_source_set_frames) runs before the next frame is served.
  int (*refill)(void*) = nullptr; void* refillUser = nullptr; bool stale = false, filling = false;
  void reset() override { dsr_stream::reset(); if (!filling) stale = true; }
  void compute() override {
    if (stale && refill) {
      filling = true; const int rc = refill(refillUser); filling = false; stale = false;
      if (rc != 0) throw Error(DSR_E_PYTHON, "the frame source's refill callback failed (%d)", rc);
    }
    stale = false;
    alloc(T); if (T > 0) DSR_HIP(hipMemcpy(dev.p, frames.data(), (size_t) T * rowBytes(), hipMemcpyHostToDevice));
  }
};
struct Preemph : dsr_stream { double mu; void compute() override { alloc(ups[0]->nFrames); op_preemph(ups[0]->d<float>(), nFrames, size_, mu, d<float>(), S0); } };
struct Hamming : dsr_stream {
  DevBuf<double> w;
  void compute() override {
    alloc(ups[0]->nFrames);
    if (ups[0]->type == DSR_T_SHORT) op_hamming_s(ups[0]->d<short>(), nFrames, size_, w.p, d<float>(), S0);
    else op_hamming_f(ups[0]->d<float>(), nFrames, size_, w.p, d<float>(), S0);
  }
};
struct HighPassOp : dsr_stream { int cut = 1; void compute() override { alloc(ups[0]->nFrames); op_highpass(ups[0]->d<double2>(), nFrames, size_, cut, d<double2>(), S0); } };   // highPassFilter (postfilter.cc:1222-1261)
struct FFTOp : dsr_stream { int L; DevBuf<double2> tw; void compute() override { alloc(ups[0]->nFrames); op_fft(ups[0]->d<float>(), nFrames, L, size_, tw.p, d<double2>(), S0); } };
struct PowerOp : dsr_stream { int fftLen; void compute() override { alloc(ups[0]->nFrames); op_power(ups[0]->d<double2>(), nFrames, fftLen, size_, d<double>(), S0); } };
struct VtlnOp : dsr_stream {
  DevBuf<int> s, c, o; DevBuf<double> coef, div; int rf = 0;
  void compute() override { alloc(ups[0]->nFrames); op_vtln(ups[0]->d<double>(), nFrames, size_, s.p, c.p, o.p, coef.p, div.p, rf, d<double>(), S0); }
};
struct MelOp : dsr_stream {
  DevBuf<int> s, c, o; DevBuf<float> coef; int inN;
  void compute() override { alloc(ups[0]->nFrames); op_mel(ups[0]->d<double>(), nFrames, inN, size_, s.p, c.p, o.p, coef.p, d<double>(), S0); }
};
struct LogOp : dsr_stream { double m, a; int sphinx; void compute() override { alloc(ups[0]->nFrames); op_log(ups[0]->d<double>(), (long) nFrames * size_, m, a, sphinx, d<float>(), S0); } };
struct GemvOp : dsr_stream {         // CepstralFeature and LinearTransformFeature
  DevBuf<float> A; std::vector<float> hA;
  void compute() override { alloc(ups[0]->nFrames); op_sgemv(ups[0]->d<float>(), nFrames, ups[0]->size_, size_, A.p, d<float>(), S0); }
};
struct StorageOp : dsr_stream {      // StorageFeature (feature.cc:2992-3085)
  void compute() override {
    if (ups[0]->nFrames > 100000) throw Error(DSR_E_DIMENSION, "Frame %d is greater than maximum number %d.", ups[0]->nFrames, 100000);
    alloc(ups[0]->nFrames); if (nFrames > 0) DSR_HIP(hipMemcpy(dev.p, ups[0]->dev.p, (size_t) nFrames * rowBytes(), hipMemcpyDeviceToDevice));
  }
};
struct LpcOp : dsr_stream {         // WarpMVDR/BurgMVDR/WarpLPC/BurgLPC features (lpc.h:86-195,262-331)
  dsr_lpc* plan = nullptr;
  ~LpcOp() override { if (plan) dsr_lpc_destroy(plan); }
  void compute() override {
    alloc(ups[0]->nFrames);
    if (nFrames > 0) ok(dsr_lpc_run(plan, ups[0]->d<float>(), nFrames, d<double>(), S0));
  }
};
struct WtMvdrOp : dsr_stream {      // WarpedTwiceMVDRFeature (lpc.h:205-246, lpc.cc:409-468)
  dsr_wtmvdr* plan = nullptr;
  ~WtMvdrOp() override { if (plan) dsr_wtmvdr_destroy(plan); }
  void compute() override {
    alloc(ups[0]->nFrames);
    if (nFrames > 0) ok(dsr_wtmvdr_run(plan, ups[0]->d<float>(), nullptr, nFrames, d<double>(), nullptr, nullptr, S0));
  }
};
struct SpecSmoothOp : dsr_stream {  // SpectralSmoothing (lpc.h:342-358, lpc.cc:485-529): ups[0] = adjustTo, ups[1] = adjustFrom
  void compute() override {
    alloc(shortest(this, 0, 2));
    if (nFrames > 0) ok(dsr_specsmooth_run(ups[0]->d<double>(), ups[1]->d<double>(), nFrames, size_, d<double>(), S0));
  }
};
struct ConvOp : dsr_stream {        // OverlapAdd / OverlapSave (convolution.h:40-104): a plan with one response over the source's blocks
  dsr_conv* plan = nullptr; DevBuf<float> state;
  ~ConvOp() override { if (plan) dsr_conv_destroy(plan); }
  void compute() override {
    alloc(ups[0]->nFrames);
    if (nFrames <= 0) return;
    const size_t sb = dsr_conv_state_bytes(plan, 1);                                 // reset() zeroes the buffer (convolution.cc:166-172)
    if (sb) { state.reserve(sb / sizeof(float)); ok(dsr_conv_state_init(plan, state.p, 1, S0)); }
    ok(dsr_conv_apply(plan, ups[0]->d<float>(), nullptr, 1, nFrames, state.p, d<float>(), S0));
  }
};
struct FirOp : dsr_stream {         // FilterFeature (feature.h:1315-1410, feature.cc:3206-3313)
  std::vector<double> a;
  void compute() override {
    const int T = ups[0]->nFrames, lenA = (int) a.size(), Tout = T + (lenA == 1 ? 1 : 0);
    dev.reserve((size_t) (Tout > 0 ? Tout : 1) * rowBytes()); alloc(dsr_fir_frames_count(T, lenA));
    if (Tout > 0) ok(dsr_fir_frames_run(ups[0]->d<float>(), nullptr, a.data(), lenA, 1, T, size_, d<float>(), S0));
  }
};
struct MergeOp : dsr_stream {       // MergeFeature (feature.cc:3318-3350): stat, delta, deltaDelta side by side
  void compute() override {
    alloc(shortest(this, 0, 3));
    size_t off = 0;
    for (int k = 0; k < 3; k++) {
      const size_t w = ups[k]->rowBytes();
      if (nFrames > 0) DSR_HIP(hipMemcpy2DAsync(dev.p + off, rowBytes(), ups[k]->dev.p, w, w, (size_t) nFrames, hipMemcpyDeviceToDevice, S0));
      off += w;
    }
  }
};
// ---- the scalar feature operators of include/dsr.h section 6c (csrc/k_featops.hip), one utterance a call
struct SignalPowerOp : dsr_stream { void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_signal_power_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, d<float>(), S0)); } };
struct ZcrOp : dsr_stream { void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_zcr_hamming_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, d<float>(), S0)); } };
struct YinOp : dsr_stream {
  unsigned sr = 16000; float tr = 0.5f;
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_yin_pitch_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, sr, tr, d<float>(), nullptr, nullptr, S0)); }
};
struct SpikeOp : dsr_stream { int tapN = 3; void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_spike_filter_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, tapN, d<float>(), S0)); } };
struct Spike2Op : dsr_stream {      // SpikeFilter2 (feature.cc:3701-3776): reset() sets _meanslope = _startslope, _count = 0
  unsigned width = 3; float maxslope = 7000.0f, startslope = 100.0f, thresh = 15.0f, alpha = 0.2f; unsigned spikes = 0;
  DevBuf<float> ms; DevBuf<int> cnt;
  void reset() override { dsr_stream::reset(); spikes = 0; }
  void compute() override {
    alloc(ups[0]->nFrames);
    const int zero = 0; ms.upload(&startslope, 1, S0); cnt.upload(&zero, 1, S0);
    if (nFrames <= 0) return;
    ok(dsr_spike_filter2_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, width, maxslope, thresh, alpha, ms.p, cnt.p, d<float>(), S0));
    int c = 0; DSR_HIP(hipMemcpy(&c, cnt.p, sizeof c, hipMemcpyDeviceToHost)); spikes = (unsigned) c;
  }
};
struct MinMaxOp : dsr_stream {      // ALogFeature / NormalizeFeature (feature.cc:1383-1514): (min, max) kept across reset() when runon
  int alog = 0, runon = 0; double p0 = 0.0, p1 = 0.0; bool fresh = true; DevBuf<double> state;
  void compute() override {
    alloc(ups[0]->nFrames);
    state.reserve(2);
    if (fresh || !runon) { ok(dsr_minmax_state_init(state.p, 1, S0)); fresh = false; }
    if (nFrames <= 0) return;
    if (alog) ok(dsr_alog_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, p0, p1, runon, state.p, d<float>(), S0));
    else ok(dsr_normalize_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, p0, p1, runon, state.p, d<float>(), S0));
  }
};
struct ThreshAmpOp : dsr_stream {   // ThresholdFeature (compare -1, 0, 1) and AmplificationFeature (compare 2)
  double value = 0.0, thresh = 1.0; int compare = 1;
  void compute() override {
    alloc(ups[0]->nFrames);
    if (nFrames <= 0) return;
    if (compare == 2) ok(dsr_amplify_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, value, d<float>(), S0));
    else ok(dsr_threshold_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, value, thresh, compare, d<float>(), S0));
  }
};
struct ResampleOp : dsr_stream {
  double ratio = 16.0 / 22.05; int len = 0;
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_spectral_resample_run(ups[0]->d<double>(), nullptr, 1, nFrames, ups[0]->size_, ratio, len, d<double>(), S0)); }
};
struct SphinxMelOp : dsr_stream {
  dsr_sphinx_mel* plan = nullptr;
  ~SphinxMelOp() override { if (plan) dsr_sphinx_mel_destroy(plan); }
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_sphinx_mel_apply(plan, ups[0]->d<double>(), nullptr, 1, nFrames, d<double>(), S0)); }
};
struct CmnOp : dsr_stream {          // MeanSubtractionFeature(src, weight, devNormFactor, runon): ups[1] (optional) = the weight stream, element 0 of each frame
  int mode; double dnf;
  void compute() override {
    int T = ups[0]->nFrames;
    if (ups.size() > 1 && ups[1]->nFrames < T) T = ups[1]->nFrames;           // the weight stream ends first: so does the loop over the frames (feature.cc:2640-2644)
    alloc(T);
    op_cmn(ups[0]->d<float>(), nFrames, size_, mode, dnf, d<float>(), S0, ups.size() > 1 ? ups[1]->d<float>() : nullptr, ups.size() > 1 ? ups[1]->size_ : 0);
  }
};
struct AdjOp : dsr_stream {
  int delta;
  void compute() override { int T = ups[0]->nFrames; if (delta > 0 && T < delta) T = 0; alloc(T); op_adjacent(ups[0]->d<float>(), T, ups[0]->size_, delta, d<float>(), S0); }
};
// The block-fed analysis banks.  The upstream delivers blocks of D samples (blockLen = shiftLen = D, padZeros): concatenate them again, run the
// bank into `bins` complex64 bins a frame, widen to the size_ complex128 subbands of a frame.
struct BlockAnalysisOp : dsr_stream {
  int bins = 0; bool skipEmpty = false; DevBuf<float> x; DevBuf<float2> X; DevBuf<int> ns;
  virtual int frames(int n) = 0;       // frames for n samples
  virtual dsr_status run(int n, int T) = 0;                  // x [n] (ns = n) -> X [T][bins]
  void compute() override {
    dsr_stream* u = ups[0]; const int n = u->nFrames * u->size_;
    const int T = frames(n); alloc(T);
    x.reserve(n > 0 ? n : 1); if (n > 0) DSR_HIP(hipMemcpy(x.p, u->dev.p, (size_t) n * sizeof(float), hipMemcpyDeviceToDevice));
    ns.upload(&n, 1);
    if (skipEmpty && T <= 0) return;
    X.reserve((size_t) T * bins);
    ok(run(n, T));
    op_expand_bins(X.p, T, bins, size_, d<double2>(), S0);
  }
};
struct AnalysisOp : BlockAnalysisOp {  // OverSampledDFTAnalysisBank: M/2+1 bins, nothing to run for an empty utterance
  dsr_fb* fb = nullptr;
  ~AnalysisOp() override { if (fb) dsr_fb_destroy(fb); }
  int frames(int n) override { return dsr_fb_analysis_frames(fb, n); }
  dsr_status run(int n, int T) override { return dsr_fb_analysis(fb, x.p, ns.p, 1, 1, n > 0 ? n : 1, T, (float*) X.p, S0); }
};
struct StftOp : BlockAnalysisOp {      // NormalFFTAnalysisBank (modulated.cc:121-257): all M bins
  dsr_stft* plan = nullptr;
  ~StftOp() override { if (plan) dsr_stft_destroy(plan); }
  int frames(int n) override { return dsr_stft_frames(plan, n); }
  dsr_status run(int n, int T) override { return dsr_stft_analysis(plan, x.p, ns.p, 1, 1, n > 0 ? n : 1, T, (float*) X.p, S0); }
};
struct PrAnalysisOp : BlockAnalysisOp {  // PerfectReconstructionFFTAnalysisBank (modulated.cc:686-818): all 2M bins
  dsr_prfb* fb = nullptr;
  ~PrAnalysisOp() override { if (fb) dsr_prfb_destroy(fb); }
  int frames(int n) override { return dsr_prfb_analysis_frames(fb, n); }
  dsr_status run(int n, int T) override { return dsr_prfb_analysis(fb, x.p, ns.p, 1, 1, n > 0 ? n : 1, T, (float*) X.p, S0); }
};
// The synthesis banks: `bins` complex64 bins of every upstream frame in, blocks of size_ samples out.
struct BlockSynthesisOp : dsr_stream {
  int bins = 0; bool hermitian = false; DevBuf<float2> Y; DevBuf<int> nf;
  virtual int blocks(int Tin) = 0;
  virtual dsr_status run(int Tin, int nb) = 0;               // Y [Tin][bins] (nf = Tin) -> nb blocks
  void compute() override {
    dsr_stream* u = ups[0]; const int Tin = u->nFrames; const int nb = blocks(Tin); alloc(nb);
    if (nb <= 0) return;
    Y.reserve((size_t) Tin * bins);
    if (hermitian) op_pack_hermitian(u->d<double2>(), Tin, u->size_, Y.p, S0);      // frames need not be conjugate-symmetric (SubbandMMI + APAB)
    else op_pack_bins(u->d<double2>(), Tin, bins, u->size_, Y.p, S0);
    nf.upload(&Tin, 1);
    ok(run(Tin, nb));
  }
};
struct SynthesisOp : BlockSynthesisOp {  // OverSampledDFTSynthesisBank
  dsr_fb* fb = nullptr;
  ~SynthesisOp() override { if (fb) dsr_fb_destroy(fb); }
  int blocks(int Tin) override { return dsr_fb_synthesis_blocks(fb, Tin); }
  dsr_status run(int Tin, int nb) override { return dsr_fb_synthesis(fb, (const float*) Y.p, nf.p, 1, Tin, (int64_t) nb * size_, d<float>(), S0); }
};
struct PrSynthesisOp : BlockSynthesisOp {  // PerfectReconstructionFFTSynthesisBank (modulated.cc:820-970)
  dsr_prfb* fb = nullptr;
  ~PrSynthesisOp() override { if (fb) dsr_prfb_destroy(fb); }
  int blocks(int Tin) override { return dsr_prfb_synthesis_blocks(fb, Tin); }
  dsr_status run(int Tin, int nb) override { return dsr_prfb_synthesis(fb, (const float*) Y.p, nf.p, 1, Tin, (int64_t) nb * size_, d<float>(), S0); }
};
struct BfOp : dsr_stream {           // SubbandDS / SubbandGSC / SubbandMVDR as a stream
  dsr_bf* w; int M; DevBuf<float2> X, Y;
  int T = 0, F = 0; DevBuf<int> nf;  // of the operators built on this one that keep the packed utterance
  void compute() override {
    const int C = (int) ups.size();
    if (C == 0 || C != dsr_bf_chan_n(w)) throw Error(DSR_E_DIMENSION, "Number of channels (%d) does not match the weights (%d)", C, dsr_bf_chan_n(w));
    const int T = shortest(this, 0, C);
    alloc(T); if (T <= 0) return;
    const int F = dsr_bf_bins(w); X.reserve((size_t) C * T * F); Y.reserve((size_t) T * F);       // M/2+1 unique bins, or all M with halfBandShift
    pack_channels(this, 0, C, T, F, M, X.p);
    ok(dsr_bf_apply(w, (const float*) X.p, 1, T, (float*) Y.p, S0));
    op_expand_bins(Y.p, T, F, M, d<double2>(), S0);
  }
  void pack_half() {                  // T, F = M/2+1, X [C][T][F] of the channels' frames, nf = T
    const int C = (int) ups.size();
    T = shortest(this, 0, C); F = M / 2 + 1;
    if (T <= 0) return;
    X.reserve((size_t) C * T * F); pack_channels(this, 0, C, T, F, M, X.p); nf.upload(&T, 1);
  }
};

struct MmiOp : BfOp {                // SubbandMMI as a stream (beamformer.cc:1973-2072); channels through dsr_subband_bf_set_channel
  dsr_mmi* mm = nullptr;
  void compute() override {
    const int C = (int) ups.size();
    if (C == 0 || C != dsr_mmi_chan_n(mm)) throw Error(DSR_E_DIMENSION, "Number of channels (%d) does not match the weights (%d)", C, dsr_mmi_chan_n(mm));
    const int T = shortest(this, 0, C);
    alloc(T); if (T <= 0) return;
    const int F = dsr_mmi_bins(mm), Fo = dsr_mmi_out_bins(mm); X.reserve((size_t) C * T * F); Y.reserve((size_t) T * Fo);   // Fo = M: halfBandShift, or APAB's full frames
    pack_channels(this, 0, C, T, F, M, X.p);
    nf.upload(&T, 1);
    ok(dsr_mmi_apply(mm, (const float*) X.p, nf.p, 1, T, (float*) Y.p, S0));
    op_expand_bins(Y.p, T, Fo, M, d<double2>(), S0);
  }
};

// The SRP estimators' stream face: DOAEstimatorSRPDSBLA (beamformer.cc:3188-3283) over a BfOp, DOAEstimatorSRPEB / DOAEstimatorSRPSphDSB
// (modalBeamformer.cc:860-950, :1284-1370) over a SphBfOp; channels through dsr_subband_bf_set_channel.  H names the handle's calls; a binding
// packs the channels (pack_frames: X, nf, T, F) and may add to the re-materialise condition (moved) and note an ungated frame (served).
template <class Base, class H> struct SrpFace : Base {
  typedef H Calls;
  typename H::Handle* est = nullptr; unsigned gen = 0, seenGen = ~0u; int nU = 0;
  std::vector<float> E; std::vector<double> RP; std::vector<float2> Yh;              // the materialised utterance: energy, rp, last unit's bins
  std::vector<double> gth, gph;                                                      // the table's units: (theta, phi)
  // the reference object's observable state
  std::vector<double> acc, rpMat, nbRp, nbDoa, vec; std::vector<int> nbIdx; float energy = 0.f; bool haveAcc = false;
  DevBuf<float> dE; DevBuf<double> dRP, dAcc, dNbR; DevBuf<int> dNbI; DevBuf<float2> dY; int rangeUsed[2] = {-1, -1};
  virtual void pack_frames() = 0;
  virtual bool moved() const { return false; }
  virtual void served(int) {}
  void compute() override {
    const int C = (int) this->ups.size();
    if (C == 0 || C != H::chan_n(est)) throw Error(DSR_E_DIMENSION, "Number of channels (%d) does not match the estimator (%d)", C, H::chan_n(est));
    range(rangeUsed[0], rangeUsed[1]);
    ok(H::build_table(est)); H::grid(est, gth, gph); nU = (int) gth.size();
    pack_frames();
    const int T = this->T, F = this->F; this->nFrames = T;
    if (T <= 0) return;
    const int nB = H::nbest(est);
    dY.reserve((size_t) T * F); dE.reserve(T); dRP.reserve((size_t) T * nU); dAcc.reserve(nU);
    dNbR.reserve((size_t) T * nB); dNbI.reserve((size_t) T * nB);
    DSR_HIP(hipMemsetAsync(dY.p, 0, sizeof(float2) * (size_t) T * F, S0)); DSR_HIP(hipMemsetAsync(dAcc.p, 0, sizeof(double) * nU, S0));
    ok(H::srp(est, (const float*) this->X.p, this->nf.p, 1, T, dE.p, dRP.p, dNbR.p, dNbI.p, dAcc.p, (float*) dY.p, nullptr, S0));
    E.resize(T); RP.resize((size_t) T * nU); Yh.resize((size_t) T * F);
    DSR_HIP(hipMemcpy(E.data(), dE.p, sizeof(float) * T, hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(RP.data(), dRP.p, sizeof(double) * RP.size(), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(Yh.data(), dY.p, sizeof(float2) * Yh.size(), hipMemcpyDeviceToHost));
  }
  void sync_table() {                 // a new steering table: _accRPs and _rpMat start from zero (beamformer.cc:3128-3130, :3148-3149; modalBeamformer.cc:818-820)
    const unsigned g = H::generation(est);
    if (g != seenGen) { acc.assign(nU, 0.0); rpMat.assign(nU, 0.0); haveAcc = true; seenGen = g; }
  }
  bool live() const { return haveAcc && H::has_table(est) && seenGen == H::generation(est); }   // setSearchParam freed _accRPs and _rpMat until the next table
  void set_doas() {                   // the ranks' (theta, phi): an empty rank is (-pi, -pi)
    nbDoa.resize(2 * nbIdx.size());
    for (size_t n = 0; n < nbIdx.size(); n++) { const int k = nbIdx[n]; nbDoa[2 * n] = k < 0 ? -M_PI : gth[k]; nbDoa[2 * n + 1] = k < 0 ? -M_PI : gph[k]; }
  }
  void reset_nbest() {
    const int nB = H::nbest(est); nbRp.resize(nB); nbIdx.resize(nB); nbest_reset(nbRp.data(), nbIdx.data(), nB); set_doas();
  }
  const void* next(int fx) override {
    const int M = this->M;
    if (vec.empty()) vec.assign((size_t) 2 * M, 0.0);
    if (fx == this->frameX && this->frameX >= 0) return vec.data();
    reset_nbest();                                          // before anything else, the end of the stream included (:3192-3196, :866-870)
    int fmin = 0, fmax = 0; range(fmin, fmax);
    if (this->ready && (gen != H::generation(est) || !H::has_table(est) || fmin != rangeUsed[0] || fmax != rangeUsed[1] || moved()))
      this->ready = false;                                  // setSearchParam (a new table), setFrequencyRange or what the binding watches since: the rest of the utterance anew
    if (!this->ready) {
      require_device();
      for (size_t i = 0; i < this->ups.size(); i++) this->ups[i]->materialize();
      compute(); gen = H::generation(est); this->ready = true;
    }
    sync_table();
    if (this->frameX + 1 >= this->nFrames) { this->endOfSamples = true; throw Error(DSR_E_ITERATOR, "end of samples!"); }
    const int t = ++this->frameX;
    energy = E[t];
    if (energy < H::threshold(est)) return vec.data();     // gated: no accumulation, no N-best, _vector as it was (:3215-3221)
    served(t);
    const int nB = H::nbest(est);
    const double* r = RP.data() + (size_t) t * nU;
    for (int k = 0; k < nU; k++) {                          // :3223-3245, :922-946
      acc[k] += r[k]; rpMat[k] = r[k];
      nbest_insert(nbRp.data(), nbIdx.data(), nB, r[k], k);
    }
    set_doas();
    const float2* y = Yh.data() + (size_t) t * this->F;
    for (int f = fmin; f <= fmax; f++) {                    // the last unit's bins and their conjugate mirror (:3166-3176, _calcResponsePower :874-889)
      vec[2 * f] = y[f].x; vec[2 * f + 1] = y[f].y;
      if (f > 0 && f < M / 2) { vec[2 * (M - f)] = y[f].x; vec[2 * (M - f) + 1] = -(double) y[f].y; }   // bin 0's mirror would be index M: not written
    }
    return vec.data();
  }
  void range(int& fmin, int& fmax) { ok(H::range(est, &fmin, &fmax)); }
  // getNBestRPs, getNBestDOAs, getResponsePowerMatrix, getAccumulators, getEnergy
  void get(int what, double* out, size_t outDoubles, size_t* n) {
    if (nbRp.empty()) reset_nbest();
    if (what < 0 || what > 4) throw Error(DSR_E_PARAMETER, "what %d", what);
    const std::vector<double> e(1, (double) energy), none;
    const std::vector<double>& v = what == 0 ? nbRp : what == 1 ? nbDoa : what == 2 ? (live() ? rpMat : none) : what == 3 ? (live() ? acc : none) : e;
    if (outDoubles < v.size()) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, v.size());
    std::copy(v.begin(), v.end(), out); *n = v.size();
  }
  void init_accs() {                  // _initAccs (beamformer.cc:3027-3041)
    std::fill(acc.begin(), acc.end(), 0.0); std::fill(rpMat.begin(), rpMat.end(), 0.0); reset_nbest();
  }
  void final_nbest() {                // _getNBestHypothesesFromACCRP (beamformer.cc:2986-3025): the DOA is the unit's (theta, phi)
    if (!live()) throw Error(DSR_E_ERROR, "no accumulators: run the estimator after construction / setSearchParam first");
    reset_nbest();
    ok(H::final_nbest(est, acc.data(), 1, nbRp.data(), nbIdx.data()));
    set_doas(); rpMat = acc;
  }
};

struct LinSrp {                      // the calls of a dsr_doa; a unit is (theta_k, _minPhi = 0)
  typedef dsr_doa Handle;
  static constexpr const char* notThis = "not a DOAEstimatorSRPDSBLA";
  static int chan_n(const Handle* h) { return dsr_doa_chan_n(h); }
  static int nbest(const Handle* h) { return dsr_doa_nbest(h); }
  static unsigned generation(const Handle* h) { return dsr_doa_table_generation(h); }
  static bool has_table(const Handle* h) { return dsr_doa_has_table(h) != 0; }
  static float threshold(const Handle* h) { return dsr_doa_energy_threshold(h); }
  static dsr_status range(const Handle* h, int* lo, int* hi) { return dsr_doa_frequency_range(h, lo, hi); }
  static dsr_status build_table(Handle* h) { return dsr_doa_build_table(h); }
  static void grid(Handle* h, std::vector<double>& th, std::vector<double>& ph) {
    int n = 0; ok(dsr_doa_theta_n(h, &n)); th.assign(n, 0.0); ph.assign(n, 0.0); ok(dsr_doa_thetas(h, th.data(), n));
  }
  static constexpr auto srp = dsr_doa_srp;
  static constexpr auto final_nbest = dsr_doa_final_nbest;
};
struct SphSrp {                      // the calls of a dsr_sph; the units are the (theta, phi) grid, theta-major
  typedef dsr_sph Handle;
  static constexpr const char* notThis = "not a spherical DOA estimator";
  static int chan_n(const Handle* h) { return dsr_sph_chan_n(h); }
  static int nbest(const Handle* h) { return dsr_sph_nbest(h); }
  static unsigned generation(const Handle* h) { return dsr_sph_table_generation(h); }
  static bool has_table(const Handle* h) { return dsr_sph_has_table(h) != 0; }
  static float threshold(const Handle* h) { return dsr_sph_energy_threshold(h); }
  static dsr_status range(const Handle* h, int* lo, int* hi) { return dsr_sph_frequency_range(h, lo, hi); }
  static dsr_status build_table(Handle* h) { return dsr_sph_build_table(h); }
  static void grid(Handle* h, std::vector<double>& th, std::vector<double>& ph) {
    int nT = 0, nP = 0; ok(dsr_sph_grid_n(h, &nT, &nP)); th.assign((size_t) nT * nP, 0.0); ph.assign((size_t) nT * nP, 0.0);
    ok(dsr_sph_grid(h, th.data(), ph.data(), nT * nP));
  }
  static constexpr auto srp = dsr_sph_srp;
  static constexpr auto final_nbest = dsr_sph_final_nbest;
};

struct DoaOp : SrpFace<BfOp, LinSrp> { void pack_frames() override { pack_half(); } };

struct SphBfOp : BfOp {              // EigenBeamformer / SphericalDSBeamformer and the further kinds (:1490-1542, :1858-1906, :2174-2222) as a stream (modalBeamformer.cc:347-399)
  // the utterance is materialised at the first pull; a geometry, look-direction, sigma2 or gain change since (the handle's settings generation)
  // recomputes it at the next pull, the frame counter kept.  The eigenbeams (getSnapShotArray) are computed on the device only when asked for.
  dsr_sph* sph = nullptr; int dim = 0; DevBuf<float2> dF, dYs; unsigned setGen = ~0u; bool eigenDone = false;
  int eigenFrame = -1; bool eigenRange = false; int eigenLo = 0, eigenHi = 0;
  void pack() {                       // X [C][T][F] of the channels' frames
    const int C = (int) ups.size();
    if (C == 0 || C != dsr_sph_chan_n(sph)) throw Error(DSR_E_DIMENSION, "Number of channels (%d) does not match the beamformer (%d)", C, dsr_sph_chan_n(sph));
    dim = dsr_sph_dim(sph); eigenDone = false; setGen = dsr_sph_settings_generation(sph);
    pack_half();
  }
  void compute() override {
    pack(); alloc(T); if (T <= 0) return;
    Y.reserve((size_t) T * F);
    if (dsr_sph_kind(sph) >= DSR_SPH_HWNC) ok(dsr_sph_beams(sph, (const float*) X.p, nf.p, 1, T, 1, (float*) Y.p, S0));   // the further kinds: one beam, the look direction
    else ok(dsr_sph_apply(sph, (const float*) X.p, nf.p, 1, T, (float*) Y.p, nullptr, S0));
    op_expand_bins(Y.p, T, F, M, d<double2>(), S0);
  }
  bool settings_moved() const { return ready && setGen != dsr_sph_settings_generation(sph); }
  const void* next(int fx) override {
    if (!(fx == frameX && frameX >= 0) && settings_moved()) ready = false;
    const void* r = BfOp::next(fx); eigenFrame = frameX; return r;
  }
  void eigenbeams(double* out) {                            // the current frame's F [F][dim] (zero before the first frame; the DOA op: its range only)
    std::vector<float2> fr((size_t) F * dim, make_float2(0.f, 0.f));
    if (eigenFrame >= 0 && eigenFrame < T) {
      if (!eigenDone) {
        dF.reserve((size_t) T * F * dim); dYs.reserve((size_t) T * F);
        ok(dsr_sph_apply(sph, (const float*) X.p, nf.p, 1, T, (float*) dYs.p, (float*) dF.p, S0));
        eigenDone = true;
      }
      DSR_HIP(hipMemcpy(fr.data(), dF.p + (size_t) eigenFrame * F * dim, sizeof(float2) * fr.size(), hipMemcpyDeviceToHost));
    }
    for (int f = 0; f < F; f++)
      for (int d = 0; d < dim; d++) {
        const bool have = !eigenRange || (f >= eigenLo && f <= eigenHi);
        const float2 v = have ? fr[(size_t) f * dim + d] : make_float2(0.f, 0.f);
        out[((size_t) f * dim + d) * 2] = v.x; out[((size_t) f * dim + d) * 2 + 1] = v.y;
      }
  }
};

// ModalSphericalArrayTracker / SpatialSphericalArrayTracker as a stream (tracker.cc:1280-1345 / :1356-1436) over a dsr_trk handle (not owned):
// ups = the 32 channels, a row = float (theta, phi).  The filter's state (position, K) belongs to the operator and outlives reset(), as in the
// reference; nextSpeaker() resets the stream and the state, setInitialPosition() moves the position alone.
struct TrkOp : dsr_stream {
  dsr_trk* trk = nullptr; int M = 0; DevBuf<float2> X; DevBuf<int> nf; DevBuf<double> state, p64; DevBuf<int> inf; bool stateReady = false, posPending = false; double pTheta = 0, pPhi = 0;
  void need_state() {
    if (!stateReady) { require_device(); state.reserve(dsr_trk_state_doubles(trk)); ok(dsr_trk_init_state(trk, state.p, 1, 0, S0)); stateReady = true; }
    if (posPending) { ok(dsr_trk_set_initial_position(trk, pTheta, pPhi)); ok(dsr_trk_init_state(trk, state.p, 1, 1, S0)); ok(dsr_trk_next_speaker(trk)); posPending = false; }
  }
  void compute() override {
    const int C = (int) ups.size();
    if (C != 32) throw Error(DSR_E_ARG, "the tracker needs the EigenMike's 32 channels, %d are set", C);
    const int T = shortest(this, 0, C), F = M / 2 + 1;
    alloc(T); if (T <= 0) return;
    need_state();
    X.reserve((size_t) C * T * F); pack_channels(this, 0, C, T, F, M, X.p); nf.upload(&T, 1);
    p64.reserve((size_t) T * 2); inf.reserve(T);
    ok(dsr_trk_run(trk, (const float*) X.p, nf.p, 1, T, state.p, d<float>(), p64.p, inf.p, S0));
  }
};
// PlaneWaveSimulator(source, modalDecomposition, channelX, theta, phi) (tracker.cc:1444-1488): ups[0] = the source spectrum; rows of fftLen bins
struct PwsOp : dsr_stream {
  int M = 0; std::vector<double2> hcoef; DevBuf<double2> coef; DevBuf<float2> src, Y; DevBuf<int> nf;
  void compute() override {
    const int T = ups[0]->nFrames, F = M / 2 + 1;
    alloc(T); if (T <= 0) return;
    if (!coef.p) coef.upload(hcoef);
    src.reserve((size_t) T * F); Y.reserve((size_t) T * M); op_pack_bins(ups[0]->d<double2>(), T, F, ups[0]->size_, src.p, S0); nf.upload(&T, 1);
    ok(dsr_pws_apply((const double*) coef.p, 1, (const float*) src.p, nf.p, 1, T, M, 1, (float*) Y.p, S0));
    op_expand_bins(Y.p, T, M, M, d<double2>(), S0);
  }
};

// the eigenbeams of the DOA operator: its range only, of the last ungated frame (a re-materialisation keeps it), anew after a settings change
struct SphDoaOp : SrpFace<SphBfOp, SphSrp> {
  void pack_frames() override { pack(); eigenRange = true; eigenLo = rangeUsed[0]; eigenHi = rangeUsed[1]; }   // the eigenbeams themselves only when getSnapShotArray asks
  bool moved() const override { return settings_moved(); }
  void served(int t) override { eigenFrame = t; }
};

struct OrthOp : dsr_stream {         // SubbandOrthogonalizer(beamformer, outChanX) (beamformer.cc:2817-2849): ups[0] = the SubbandMVDRGSC operator
  int outChanX = 0; DevBuf<float2> Z;
  void compute() override {
    BfOp* bf = dynamic_cast<BfOp*>(ups[0]); if (!bf) throw Error(DSR_E_PARAMETER, "SubbandOrthogonalizer needs a subband beamformer");
    const int T = bf->nFrames; alloc(T); if (T <= 0) return;
    if (outChanX <= 0) { DSR_HIP(hipMemcpyAsync(d<double2>(), bf->d<double2>(), sizeof(double2) * (size_t) T * size_, hipMemcpyDeviceToDevice, S0)); return; }
    const int F = bf->M / 2 + 1; Z.reserve((size_t) T * F);
    ok(dsr_bf_blocking_matrix_output(bf->w, (const float*) bf->X.p, 1, T, outChanX - 1, (float*) Z.p, S0));
    op_orth_assemble(Z.p, bf->d<double2>(), T, F, bf->M, d<double2>(), S0);
  }
};
struct WpeOp : dsr_stream {          // SingleChannelWPEDereverberationFeature (dereverberation.cc:28-300)
  int M = 0, lowerN = 0, upperN = 0, iterationsN = 2; double loadDb = -20.0, bandWidth = 0.0, sampleRate = 16000.0; DevBuf<float2> Y, O; DevBuf<int> nf;
  void compute() override {
    const int T = ups[0]->nFrames; alloc(T); if (T <= 0) return;
    const int F = M / 2 + 1; Y.reserve((size_t) T * F); O.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, Y.p, S0); nf.upload(&T, 1);
    ok(dsr_wpe_single((const float*) Y.p, nf.p, 1, T, M, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, (float*) O.p, nullptr, S0));
    op_expand_bins(O.p, T, F, M, d<double2>(), S0);
  }
};
struct WpeMultiOp : dsr_stream {     // MultiChannelWPEDereverberationFeature(source, channelX) (dereverberation.cc:281-602): ups = the source's channels
  int M = 0, lowerN = 0, upperN = 0, iterationsN = 2, channelX = 0, filterChan = -2; double loadDb = -20.0, bandWidth = 0.0, sampleRate = 16000.0;
  DevBuf<float2> Y, O; DevBuf<double2> G; DevBuf<int> nf;
  void compute() override {
    const int C = (int) ups.size();
    const int T = shortest(this, 0, C);                     // _fillBuffer stops with the shortest channel (:397-412)
    alloc(T); if (T <= 0) return;
    const int F = M / 2 + 1, P = upperN - lowerN + 1; Y.reserve((size_t) C * T * F); O.reserve((size_t) C * T * F); G.reserve((size_t) C * F * C * P);
    pack_channels(this, 0, C, T, F, M, Y.p);
    nf.upload(&T, 1);
    // all channels of a frame go through the filter of the channel that asked first (:381); on its own a feature asks first itself
    const int fc = filterChan == -2 ? channelX : filterChan;
    ok(dsr_wpe_multi((const float*) Y.p, nf.p, 1, C, T, M, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, fc, (float*) O.p, (double*) G.p, S0));
    op_expand_bins(O.p + (size_t) channelX * T * F, T, F, M, d<double2>(), S0);
  }
};
struct AecOp : dsr_stream {          // the echo cancellers of btk/cancelVP as a stream (cancelVP.cc:57-104, :141-209, :287-383, :513-650, :748-855, :1121-1198): ups = played, recorded
  dsr_aec* aec = nullptr; int M = 0, frameMode = 0; DevBuf<float2> P, Rc, O; DevBuf<int> nf; DevBuf<unsigned char> state; bool haveState = false;
  void ensure_state() {
    if (haveState) return;
    state.reserve(dsr_aec_state_bytes(aec, 1));
    ok(dsr_aec_state_init(aec, state.p, 1, S0));
    haveState = true;
  }
  void reset() override {                // cancelVP.h:60, :98, :134-142: filter coefficients only (NLMS, Kalman) or nothing (block variants)
    dsr_stream::reset();
    if (haveState) ok(dsr_aec_reset_filter(aec, state.p, 1, S0));
  }
  const void* next(int fx) override { if (!ready) frameMode = fx < 0 ? 1 : 0; return dsr_stream::next(fx); }
  void compute() override {
    const int T = ups[0]->nFrames < ups[1]->nFrames ? ups[0]->nFrames : ups[1]->nFrames; alloc(T); if (T <= 0) return;
    ensure_state();
    const int F = M / 2 + 1; P.reserve((size_t) T * F); Rc.reserve((size_t) T * F); O.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, P.p, S0); op_pack_bins(ups[1]->d<double2>(), T, F, M, Rc.p, S0); nf.upload(&T, 1);
    ok(dsr_aec_set_frame_mode(aec, dsr_aec_kind(aec) >= DSR_AEC_DTD ? frameMode : 0));      // DTD and the information kinds: _updateBand reads frameX
    ok(dsr_aec_apply(aec, (const float*) P.p, (const float*) Rc.p, nf.p, 1, T, 0, (float*) O.p, state.p, S0));
    op_expand_bins(O.p, T, F, M, d<double2>(), S0);
  }
};
struct CctdeOp : dsr_stream {        // CCTDE (CCTDE.h:60-101, CCTDE.cc:46-342): ups = the two SampleFeatures; a row = the nHeldMaxCC delays in seconds
  int N = 0, nHeld = 1, lower = -1, upper = -1;      // the band limits are kept and, as in the reference, never used (CCTDE.cc:186-205 cannot be reached)
  std::vector<int> allArgs, args; std::vector<double> allVals, vals, vec; DevBuf<double> dVals, dOne; DevBuf<int> dArgs, dArg1; DevBuf<float> pad; bool whole = false;
  int rate() const { return static_cast<const SampleSrc*>(ups[0])->sampleRate; }
  void reset() override { dsr_stream::reset(); whole = false; }
  // every block pair of the utterance in one call; next() then serves rows while the two sources move together
  void compute() override {
    const int T = shortest(this, 0, 2); alloc(T); allArgs.assign((size_t) T * nHeld, 0); allVals.assign((size_t) T * nHeld, 0.0); if (T <= 0) return;
    dVals.reserve((size_t) T * nHeld); dArgs.reserve((size_t) T * nHeld);
    ok(dsr_cctde_run(ups[0]->d<float>(), ups[1]->d<float>(), T, ups[0]->size_, N, nHeld, rate(), d<double>(), dArgs.p, dVals.p, S0));
    DSR_HIP(hipMemcpy(allArgs.data(), dArgs.p, allArgs.size() * sizeof(int), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(allVals.data(), dVals.p, allVals.size() * 8, hipMemcpyDeviceToHost));
  }
  // one pair of blocks that is not a row of the batch: the sources stand at different frames (nextX), or a whole recording (allsamples)
  const void* one(const float* a, const float* b, int blockLen, int fftLen) {
    dOne.reserve(2 * (size_t) nHeld); dArg1.reserve(nHeld); args.assign(nHeld, 0); vals.assign(nHeld, 0.0); vec.assign(nHeld, 0.0);
    ok(dsr_cctde_run(a, b, 1, blockLen, fftLen, nHeld, rate(), dOne.p, dArg1.p, dOne.p + nHeld, S0));
    DSR_HIP(hipMemcpy(vec.data(), dOne.p, (size_t) nHeld * 8, hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(vals.data(), dOne.p + nHeld, (size_t) nHeld * 8, hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(args.data(), dArg1.p, (size_t) nHeld * sizeof(int), hipMemcpyDeviceToHost));
    return vec.data();
  }
  const void* serve() {
    const int f0 = ups[0]->frameX, f1 = ups[1]->frameX, L = ups[0]->size_;
    if (f0 != f1) return one(ups[0]->d<float>() + (size_t) f0 * L, ups[1]->d<float>() + (size_t) f1 * L, L, N);
    materialize();
    args.assign(allArgs.begin() + (size_t) f0 * nHeld, allArgs.begin() + (size_t) (f0 + 1) * nHeld);
    vals.assign(allVals.begin() + (size_t) f0 * nHeld, allVals.begin() + (size_t) (f0 + 1) * nHeld);
    const double* r = (const double*) row(f0); vec.assign(r, r + nHeld);
    return vec.data();
  }
  const void* next(int fx) override {                      // CCTDE.cc:146-155: both sources move on
    if (fx == frameX && (frameX >= 0 || whole)) return vec.data();
    try { ups[0]->next(fx); ups[1]->next(fx); } catch (const Error&) { endOfSamples = true; throw; }
    whole = false; frameX++;
    return serve();
  }
  const void* nextX(int chanX, int fx) {                   // CCTDE.cc:262-302: source chanX moves on, the other one's current block is used again
    if (chanX < 0 || chanX > 1) throw Error(DSR_E_INDEX, "channel %d of 2", chanX);
    if (ups[1 - chanX]->frameX < 0) throw Error(DSR_E_CONSISTENCY, "Frame index (%d) < 0.", ups[1 - chanX]->frameX);
    try { ups[chanX]->next(fx); } catch (const Error&) { endOfSamples = true; throw; }
    whole = false; if (chanX == 0) frameX++;
    return serve();
  }
  void allsamples(int fftLen) {                            // CCTDE.cc:304-342: the two recordings as one block pair; the FFT length stays changed
    const SampleSrc* s0 = static_cast<const SampleSrc*>(ups[0]); const SampleSrc* s1 = static_cast<const SampleSrc*>(ups[1]);
    const size_t n0 = s0->samples.size(), n1 = s1->samples.size(), nmax = n0 > n1 ? n0 : n1;
    int L = fftLen;
    if (L < 0) { size_t p2 = 1; while (p2 < nmax) p2 *= 2; if (p2 > (size_t) 1 << 30) throw Error(DSR_E_DIMENSION, "%zu samples", nmax); L = (int) p2; }
    ok(dsr_cctde_check(L, nHeld)); require_device();
    N = L;
    const size_t bl = nmax < (size_t) L ? (nmax ? nmax : 1) : (size_t) L;
    std::vector<float> h(2 * bl, 0.0f);
    std::copy(s0->samples.begin(), s0->samples.begin() + (n0 < bl ? n0 : bl), h.begin()); std::copy(s1->samples.begin(), s1->samples.begin() + (n1 < bl ? n1 : bl), h.begin() + bl);
    pad.upload(h.data(), h.size());
    one(pad.p, pad.p + bl, (int) bl, L); whole = true;
  }
};
struct ZelinskiOp : dsr_stream {     // ZelinskiPostFilter (postfilter.cc:350-493): ups[0] = beamformer output, ups[1..] = the snapshot array's channels
  dsr_zelinski* plan = nullptr; int M = 0; double alpha = 0.6; int ptype = 2, minFrames = 0; std::vector<std::vector<double>> manifold; int chanSet = 0;
  int kind = 0; float threshold = 0.99f;                   // kind 1: McCowanPostFilter (the plan then also carries the noise coherence matrices)
  double minSV = 1e-8; int fbinX1 = 0;                     // kind 2: LefkimmiatisPostFilter
  void ensure_plan(int C) {
    if (plan) return;
    ok(kind == 2 ? dsr_lefkimmiatis_create(M, C, minSV, fbinX1, alpha, ptype, minFrames, threshold, &plan)
       : kind ? dsr_mccowan_create(M, C, alpha, ptype, minFrames, threshold, &plan) : dsr_zelinski_create(M, C, alpha, ptype, minFrames, &plan));
  }
  DevBuf<float2> X, Y, O; DevBuf<int> nf;
  ~ZelinskiOp() override { if (plan) dsr_zelinski_destroy(plan); }
  void compute() override {
    const int C = (int) ups.size() - 1;
    if (C < 1 || chanSet == 0) throw Error(DSR_E_ERROR, "set beamformer's weights");                     // postfilter.cc:447-450
    if (chanSet != C) throw Error(DSR_E_DIMENSION, "array manifold has %d channels, the snapshot array %d", chanSet, C);
    const int T = shortest(this, 0, C + 1);
    alloc(T); if (T <= 0) return;
    ensure_plan(C);
    for (int f = 0; f <= M / 2; f++) if (!manifold[f].empty()) dsr_zelinski_set_manifold(plan, f, manifold[f].data());
    const int F = M / 2 + 1; X.reserve((size_t) C * T * F); Y.reserve((size_t) T * F); O.reserve((size_t) T * F);
    pack_channels(this, 1, C, T, F, M, X.p);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, Y.p, S0);
    nf.upload(&T, 1);
    ok(dsr_zelinski_apply(plan, (const float*) X.p, (const float*) Y.p, nf.p, 1, T, (float*) O.p, nullptr, S0));
    op_expand_bins(O.p, T, F, M, d<double2>(), S0);
  }
};

// SpectralSubtractor (spectralsubtraction.cc:141-267): ups = the channels of setChannel.  The noise estimates live as long as the operator
// (reset() never touches them); the state is sized by the first call that needs it, channels are set before that.
struct SpecSubOp : dsr_stream {
  dsr_specsub* h = nullptr; int M = 0; DevBuf<float2> X; DevBuf<int> nf; DevBuf<unsigned char> state; int stateC = 0;
  ~SpecSubOp() override { if (h) dsr_specsub_destroy(h); }
  void* st() {
    const int C = (int) ups.size();
    if (stateC == 0 && C > 0) { require_device(); state.reserve(dsr_specsub_state_bytes(h, 1)); ok(dsr_specsub_state_init(h, state.p, 1, S0)); stateC = C; }
    if (stateC != C) throw Error(DSR_E_CONSISTENCY, "setChannel() after the noise estimates are in use (%d channels, %d now)", stateC, C);
    return state.p;
  }
  void compute() override {
    const int C = (int) ups.size(); if (C < 1) throw Error(DSR_E_ERROR, "setChannel() has not been called");
    const int T = shortest(this, 0, C); alloc(T); if (T <= 0) return;
    const int F = M / 2 + 1; X.reserve((size_t) C * T * F); pack_channels(this, 0, C, T, F, M, X.p); nf.upload(&T, 1);
    ok(dsr_specsub_apply(h, (const float*) X.p, nf.p, 1, T, dev.p, M, 1, st(), S0));
  }
};
struct WienerOp : dsr_stream {       // WienerFilter (spectralsubtraction.cc:269-347): ups = target, noise; frame counter and PSD memories outlive reset()
  dsr_wiener* h = nullptr; int M = 0; DevBuf<float2> S, N; DevBuf<int> nf; DevBuf<unsigned char> state; bool have = false;
  ~WienerOp() override { if (h) dsr_wiener_destroy(h); }
  void compute() override {
    const int T = shortest(this, 0, 2); alloc(T); if (T <= 0) return;
    if (!have) { state.reserve(dsr_wiener_state_bytes(h, 1)); ok(dsr_wiener_state_init(h, state.p, 1, S0)); have = true; }
    const int F = M / 2 + 1; S.reserve((size_t) T * F); N.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, S.p, S0); op_pack_bins(ups[1]->d<double2>(), T, F, M, N.p, S0); nf.upload(&T, 1);
    ok(dsr_wiener_apply(h, (const float*) S.p, (const float*) N.p, nf.p, 1, T, dev.p, M, 1, state.p, S0));
  }
};
struct MaskOp : dsr_stream {         // BinaryMaskFilter / KimBinaryMaskFilter / IIDBinaryMaskFilter (binauralprocessing.cc:47-211, 431-520): ups = srcL, srcR
  dsr_binmask* h = nullptr; int M = 0; DevBuf<float2> L, R; DevBuf<int> nf; DevBuf<unsigned char> state; bool have = false;
  ~MaskOp() override { if (h) dsr_binmask_destroy(h); }
  void compute() override {
    const int T = shortest(this, 0, 2); alloc(T); if (T <= 0) return;
    if (!have) { state.reserve(dsr_binmask_state_bytes(h, 1)); ok(dsr_binmask_state_init(h, state.p, 1, S0)); have = true; }   // _prevMu = 1, untouched by reset()
    const int F = M / 2 + 1; L.reserve((size_t) T * F); R.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, L.p, S0); op_pack_bins(ups[1]->d<double2>(), T, F, M, R.p, S0); nf.upload(&T, 1);
    ok(dsr_binmask_apply(h, (const float*) L.p, (const float*) R.p, nf.p, 1, T, dev.p, M, 1, nullptr, nullptr, state.p, S0));
  }
};
// KimITD / IID / FDIID ThresholdEstimator (binauralprocessing.cc:232-426, 525-683, 702-928): ups = srcL, srcR; the output vector is never written
// there, so the rows are zeros; reset() clears the accumulators; calcThreshold divides them in place, so a second call differs, as there
struct ThestOp : dsr_stream {
  dsr_thest* h = nullptr; int M = 0; DevBuf<float2> L, R; DevBuf<int> nf; DevBuf<unsigned char> state; bool have = false, fresh = false;
  std::vector<double> acc, cost, thresholds; double threshold = 0.0;
  ~ThestOp() override { if (h) dsr_thest_destroy(h); }
  void ensure() { if (!have) { require_device(); state.reserve(dsr_thest_state_bytes(h, 1)); ok(dsr_thest_state_init(h, state.p, 1, S0)); have = true; } }
  void reset() override { dsr_stream::reset(); if (have) ok(dsr_thest_reset_state(h, state.p, 1, S0)); fresh = false; }
  void compute() override {
    const int T = shortest(this, 0, 2); alloc(T); DSR_HIP(hipMemsetAsync(dev.p, 0, (size_t) (T > 0 ? T : 1) * rowBytes(), S0)); fresh = false; if (T <= 0) return;
    ensure();
    const int F = M / 2 + 1; L.reserve((size_t) T * F); R.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, L.p, S0); op_pack_bins(ups[1]->d<double2>(), T, F, M, R.p, S0); nf.upload(&T, 1);
    ok(dsr_thest_run(h, (const float*) L.p, (const float*) R.p, nf.p, 1, T, state.p, S0));
  }
  double calc() {
    ensure();
    const size_t n = dsr_thest_acc_doubles(h), F = (size_t) M / 2 + 1, nC = (size_t) dsr_thest_n_cand(h);
    if (!fresh) { acc.assign(n, 0.0); ok(dsr_thest_state_read(h, state.p, 1, 0, acc.data(), n)); fresh = true; }
    cost.assign(dsr_thest_kind(h) == DSR_THEST_FDIID ? F * nC : nC, 0.0); thresholds.assign(F, 0.0);
    ok(dsr_thest_calc_threshold(h, acc.data(), n, 1, &threshold, nullptr, cost.data(), cost.size(), thresholds.data(), (int) F));
    return threshold;
  }
};

struct MccOp : dsr_stream {          // MCCLocalizer / MCCCalculator (MCCLocalizer.h:214-301): ups = the channels, a row = the best position / [cost, 0, 0]
  dsr_mcc* mcc = nullptr; bool calc = false; int normalize = 1; bool haveDelays = false; std::vector<double> delays;
  int C = 0, S = 1; std::vector<float> hx; DevBuf<float> dx; DevBuf<double> dD; DevBuf<int> dI;
  std::vector<double> vec, cost, pos, eig, R; std::vector<int> tau;
  void compute() override {}
  void init() {
    C = dsr_mcc_chan_n(mcc); S = calc ? 1 : dsr_mcc_max_source(mcc);
    vec.assign(3, 0.0); cost.assign(S, 0.0); pos.assign((size_t) S * 3, 0.0); eig.assign((size_t) S * C, 0.0); tau.assign((size_t) S * C, 0); R.assign((size_t) C * C, 0.0);
  }
  const void* next(int fx) override {
    if (fx == frameX && frameX >= 0) return vec.data();
    if (calc && !haveDelays) { fprintf(stderr, "set time delays with setTimeDelays()\n"); throw Error(DSR_E_ERROR, "set time delays with setTimeDelays()"); }   // MCCLocalizer.cc:540-543
    if ((int) ups.size() != C) throw Error(DSR_E_DIMENSION, "%zu channels are set, the search grid has %d", ups.size(), C);
    const int L = ups[0]->size_;
    hx.resize((size_t) C * L);
    try { for (int c = 0; c < C; c++) std::memcpy(hx.data() + (size_t) c * L, ups[c]->next(fx), (size_t) L * sizeof(float)); }
    catch (const Error&) { endOfSamples = true; throw; }
    ok(dsr_mcc_check_block(mcc, L));                                                                     // "Data samples are insufficient", before anything is allocated
    const size_t nd = (size_t) S * (1 + 3 + C) + (size_t) C * C;
    dx.reserve(hx.size()); dD.reserve(nd); dI.reserve((size_t) S * C);
    double* dCost = dD.p; double* dPos = dCost + S; double* dEig = dPos + (size_t) S * 3; double* dR = dEig + (size_t) S * C;
    DSR_HIP(hipMemcpy(dx.p, hx.data(), hx.size() * sizeof(float), hipMemcpyHostToDevice));
    if (calc) ok(dsr_mcc_calc(mcc, dx.p, nullptr, 1, L, L, delays.data(), normalize, nullptr, dCost, tau.data(), dEig, dR, S0));
    else ok(dsr_mcc_run(mcc, dx.p, nullptr, 1, L, L, nullptr, nullptr, dCost, dI.p, dPos, dEig, nullptr, dR, S0));
    DSR_HIP(hipStreamSynchronize(S0));
    DSR_HIP(hipMemcpy(cost.data(), dCost, cost.size() * 8, hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(eig.data(), dEig, eig.size() * 8, hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(R.data(), dR, R.size() * 8, hipMemcpyDeviceToHost));
    if (calc) { vec[0] = cost[0]; vec[1] = vec[2] = 0.0; }
    else {
      DSR_HIP(hipMemcpy(pos.data(), dPos, pos.size() * 8, hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(tau.data(), dI.p, tau.size() * sizeof(int), hipMemcpyDeviceToHost));
      for (int k = 0; k < 3; k++) vec[k] = pos[k];
    }
    frameX++;
    return vec.data();
  }
};

template <class T> T* mk(const char* name, const char* dflt, int size, int type) { T* s = new T(); s->name = (name && *name) ? name : dflt; s->size_ = size; s->type = type; return s; }
// what the filter-bank operators' create functions share: the operator (order unchecked, `bins` bins a frame on the bank's side) owns the plan
// that `plan` creates into it, and is handed out on top of `up` only when that succeeded
template <class Op, class Plan> void bank_create(dsr_stream* up, const char* name, const char* dflt, int size, int type, int bins, dsr_stream** out, Plan plan)
{
  std::unique_ptr<Op> s(mk<Op>(name, dflt, size, type)); s->bins = bins; s->checkOrder = false;
  ok(plan(*s));
  s->add_up(up); *out = s.release();
}
// a stream handle as the operator Op, or Op's own refusal
template <class Op> Op& srp_op(dsr_stream* s, bool argsOk = true)
{
  Op* q = dynamic_cast<Op*>(s); if (!q || !argsOk) throw Error(DSR_E_PARAMETER, "%s", Op::Calls::notThis);
  return *q;
}
template <class Op> Op* as_op(dsr_stream* s, const char* what) { Op* q = dynamic_cast<Op*>(s); if (!q) throw Error(DSR_E_PARAMETER, "not a %s stream", what); return q; }
dsr_stream* need(dsr_stream* s, int type, const char* what) {
  if (!s) throw Error(DSR_E_PARAMETER, "null upstream for %s", what);
  if (s->type != type) throw Error(DSR_E_TYPE, "%s needs an upstream of element type %d, got %d", what, type, s->type);
  return s;
}

}  // namespace

extern "C" {

void dsr_stream_retain(dsr_stream* s) { if (s) s->refs++; }
void dsr_stream_release(dsr_stream* s) { if (s && --s->refs == 0) delete s; }
int dsr_stream_size(const dsr_stream* s) { return s->size_; }
int dsr_stream_type(const dsr_stream* s) { return s->type; }
int dsr_stream_frameX(const dsr_stream* s) { return s->frameX; }
int dsr_stream_is_end(const dsr_stream* s) { return s->endOfSamples ? 1 : 0; }
const char* dsr_stream_name(const dsr_stream* s) { return s->name.c_str(); }

dsr_status dsr_stream_next(dsr_stream* s, int frameX, const void** data, size_t* n)
{ return guard([&] { if (!s || !data) throw Error(DSR_E_PARAMETER, "null argument"); *data = s->next(frameX); if (n) *n = (size_t) s->size_; }); }
dsr_status dsr_stream_current(dsr_stream* s, const void** data, size_t* n)
{
  return guard([&] {
    if (!s || !data) throw Error(DSR_E_PARAMETER, "null argument");
    if (s->frameX < 0) throw Error(DSR_E_CONSISTENCY, "Frame index (%d) < 0.", s->frameX);      // stream.h:44-46
    *data = s->next(s->frameX); if (n) *n = (size_t) s->size_;
  });
}
dsr_status dsr_stream_reset(dsr_stream* s) { return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->reset(); }); }

dsr_status dsr_sample_feature_create(int blockLen, int shiftLen, int padZeros, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!out || blockLen < 1 || shiftLen < 1) throw Error(DSR_E_PARAMETER, "bad argument");
    SampleSrc* s = mk<SampleSrc>(name, "Sample", blockLen, DSR_T_FLOAT); s->blockLen = blockLen; s->shiftLen = shiftLen; s->padZeros = padZeros;
    s->checkOrder = true; *out = s;
  });
}
dsr_status dsr_sample_feature_set_samples(dsr_stream* s, const float* samples, size_t n, unsigned sampleRate)
{
  return guard([&] {
    SampleSrc* q = dynamic_cast<SampleSrc*>(s); if (!q || (!samples && n)) throw Error(DSR_E_PARAMETER, "not a SampleFeature");
    q->samples.assign(samples, samples + n); if (sampleRate) q->sampleRate = (int) sampleRate; q->reset();    // setSamples() resets (feature.cc:688)
  });
}
// SampleFeature::read(fn, format, samplerate, chX, chN, cfrom, to, outsamplerate, norm) (feature.cc:243-393).  The reference reads through libsndfile's
// sf_readf_float; here: RIFF/WAVE PCM of 8, 16, 24 or 32 bits (format tag 1, or the extensible tag carrying PCM), parsed by hand.  norm == 0 keeps the
// file's integer scale (SFC_SET_NORM_FLOAT off), otherwise samples are normalised to [-1, 1) and, for norm != 1, multiplied by norm.  The error branches
// are the reference's: a file that cannot be opened or parsed and an empty sample range are jio errors, chX == 0 and chX out of range jconsistency
// errors (in the reference's order: the range is checked before the channel).  Sample-rate conversion (outsamplerate != the file's rate; SRCONV builds
// only) is refused.  format / samplerate / chN only steer libsndfile's RAW reader and are accepted for the signature.  *nread = frames read.
dsr_status dsr_sample_feature_read(dsr_stream* s, const char* fn, int format, int samplerate, int chX, int chN, int cfrom, int to, int outsamplerate,
                                   float norm, int* nread)
{
  (void) format; (void) samplerate; (void) chN;
  return guard([&] {
    SampleSrc* q = dynamic_cast<SampleSrc*>(s); if (!q || !fn) throw Error(DSR_E_PARAMETER, "not a SampleFeature");
    FILE* fp = fopen(fn, "rb");
    if (!fp) throw Error(DSR_E_IO, "Could not open file %s.", fn);
    std::vector<unsigned char> raw; int nch = 0, bits = 0, rate = 0; long frames = 0; int sw = 0;
    try {
      auto rd = [&](void* p, size_t n) { if (fread(p, 1, n, fp) != n) throw Error(DSR_E_IO, "Could not open file %s.", fn); };
      auto u32 = [&]() { unsigned char b[4]; rd(b, 4); return (unsigned) b[0] | (unsigned) b[1] << 8 | (unsigned) b[2] << 16 | (unsigned) b[3] << 24; };
      auto u16 = [&]() { unsigned char b[2]; rd(b, 2); return (unsigned) (b[0] | b[1] << 8); };
      char id[4]; rd(id, 4); if (memcmp(id, "RIFF", 4)) throw Error(DSR_E_IO, "Could not open file %s.", fn);
      (void) u32(); rd(id, 4); if (memcmp(id, "WAVE", 4)) throw Error(DSR_E_IO, "Could not open file %s.", fn);
      bool haveFmt = false, haveData = false; long dataBytes = 0;
      while (!haveData) {
        if (fread(id, 1, 4, fp) != 4) break;
        const unsigned len = u32();
        if (!memcmp(id, "fmt ", 4)) {
          if (len < 16) throw Error(DSR_E_IO, "Could not open file %s.", fn);
          const unsigned tag = u16(); nch = (int) u16(); rate = (int) u32(); (void) u32(); (void) u16(); bits = (int) u16();
          if (tag != 1 && tag != 0xFFFE) throw Error(DSR_E_IO, "Could not open file %s.", fn);
          if (len > 16) fseek(fp, (long) (len - 16 + (len & 1)), SEEK_CUR);
          haveFmt = true;
        } else if (!memcmp(id, "data", 4)) {
          if (!haveFmt) throw Error(DSR_E_IO, "Could not open file %s.", fn);
          dataBytes = (long) len; haveData = true;
        } else fseek(fp, (long) (len + (len & 1)), SEEK_CUR);
      }
      if (!haveData || nch < 1) throw Error(DSR_E_IO, "Could not open file %s.", fn);
      sw = (bits + 7) / 8;
      if (sw < 1 || sw > 4) throw Error(DSR_E_IO, "sndfile error: unsupported sample width %d.", sw);
      frames = dataBytes / ((long) sw * nch);
      if (outsamplerate == -1) outsamplerate = rate;
      if (to < 0 || to >= frames) to = (int) frames - 1;
      if (cfrom < 0) cfrom = 0;
      if (cfrom > to || cfrom > frames) throw Error(DSR_E_IO, "Cannot load samples from %d to %d.", cfrom, to);
      const long n = (long) to - cfrom + 1;
      fseek(fp, (long) cfrom * sw * nch, SEEK_CUR);
      raw.resize((size_t) n * sw * nch);
      const size_t got = fread(raw.data(), 1, raw.size(), fp); raw.resize(got - got % ((size_t) sw * nch));
    } catch (...) { fclose(fp); throw; }
    fclose(fp);
    if (chX > nch || chX < 1) {
      if (chX == 0) throw Error(DSR_E_CONSISTENCY, "Multi-channel read is not yet supported.");
      throw Error(DSR_E_CONSISTENCY, "Selected channel out of range of available channels.");
    }
    const size_t nfr = raw.size() / ((size_t) sw * nch);
    std::vector<float> x(nfr);
    for (size_t i = 0; i < nfr; i++) {
      const unsigned char* b = raw.data() + (i * nch + (size_t) (chX - 1)) * sw; long long v;
      if (sw == 1) v = (long long) b[0] - 128;
      else if (sw == 2) v = (short) (b[0] | b[1] << 8);
      else if (sw == 3) { int t = b[0] | b[1] << 8 | b[2] << 16; if (t >= 1 << 23) t -= 1 << 24; v = t; }
      else v = (int) ((unsigned) b[0] | (unsigned) b[1] << 8 | (unsigned) b[2] << 16 | (unsigned) b[3] << 24);
      double d = (double) v;
      if (norm != 0.0f) d = d / (double) (1LL << (8 * sw - 1));                            // libsndfile's float normalisation
      x[i] = (float) d;
    }
    if (rate != outsamplerate) throw Error(DSR_E_ERROR, "sample rate conversion (%d -> %d) is not supported", rate, outsamplerate);
    if (norm != 1.0f && norm != 0.0f) for (size_t i = 0; i < nfr; i++) x[i] *= norm;
    q->samples.swap(x); q->sampleRate = rate; q->nChan = nch; q->reset();                  // _cur = 0; reset() (:386-388)
    if (nread) *nread = (int) nfr;
  });
}
int dsr_sample_feature_sample_rate(const dsr_stream* s) { const SampleSrc* q = dynamic_cast<const SampleSrc*>(s); return q ? q->sampleRate : 0; }
dsr_status dsr_sample_feature_data(const dsr_stream* s, const float** data, size_t* n)
{
  return guard([&] {
    const SampleSrc* q = dynamic_cast<const SampleSrc*>(s); if (!q || !data || !n) throw Error(DSR_E_PARAMETER, "not a SampleFeature");
    *data = q->samples.data(); *n = q->samples.size();
  });
}

dsr_status dsr_frame_source_create(int type, int size, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!out || size < 1 || type < 0 || type > DSR_T_COMPLEX) throw Error(DSR_E_PARAMETER, "bad argument");
    FrameSrc* s = mk<FrameSrc>(name, "PyFeatureStream", size, type); s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_frame_source_set_frames(dsr_stream* s, const void* data, size_t nframes)
{
  return guard([&] {
    FrameSrc* q = dynamic_cast<FrameSrc*>(s); if (!q || (!data && nframes)) throw Error(DSR_E_PARAMETER, "not a frame source");
    q->frames.assign((const unsigned char*) data, (const unsigned char*) data + nframes * q->rowBytes()); q->T = (int) nframes;
    const bool f = q->filling; q->filling = true; q->reset(); q->filling = f; q->stale = false;          // fresh frames: nothing to refill
  });
}
dsr_status dsr_frame_source_set_refill(dsr_stream* s, int (*refill)(void*), void* user)
{
  return guard([&] {
    FrameSrc* q = dynamic_cast<FrameSrc*>(s); if (!q) throw Error(DSR_E_PARAMETER, "not a frame source");
    q->refill = refill; q->refillUser = user;
  });
}

dsr_status dsr_analysis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, int dct, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "OverSampledDFTAnalysisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    const int D = M >> r;
    if (samp->size_ != D) throw Error(DSR_E_DIMENSION, "Input block length (%d) != _D (%d)", samp->size_, D);      // modulated.cc:373-374
    bank_create<AnalysisOp>(samp, name, "OverSampledDFTAnalysisBank", M, DSR_T_COMPLEX, M / 2 + 1, out,
                            [&](AnalysisOp& s) { s.skipEmpty = true; return dsr_fb_create(prototype, M, m, r, 0, dct, 1, &s.fb); });
  });
}
dsr_status dsr_pr_analysis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "PerfectReconstructionFFTAnalysisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    const int D = M >> r;
    if (samp->size_ != D) throw Error(DSR_E_DIMENSION, "Input block length (%d) != _D (%d)", samp->size_, D);
    bank_create<PrAnalysisOp>(samp, name, "PerfectReconstructionFFTAnalysisBank", 2 * M, DSR_T_COMPLEX, 2 * M, out,
                              [&](PrAnalysisOp& s) { return dsr_prfb_create(prototype, M, m, r, &s.fb); });
  });
}
dsr_status dsr_pr_synthesis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_COMPLEX, "PerfectReconstructionFFTSynthesisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    if (samp->size_ != 2 * M) throw Error(DSR_E_DIMENSION, "Input size (%d) != 2M (%d)", samp->size_, 2 * M);
    bank_create<PrSynthesisOp>(samp, name, "PerfectReconstructionFFTSynthesisBank", M >> r, DSR_T_FLOAT, 2 * M, out,
                               [&](PrSynthesisOp& s) { return dsr_prfb_create(prototype, M, m, r, &s.fb); });
  });
}
dsr_status dsr_normal_fft_bank_create(dsr_stream* samp, int M, int r, int windowType, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "NormalFFTAnalysisBank"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    const int D = M >> r;
    if (samp->size_ != D) throw Error(DSR_E_DIMENSION, "Input block length (%d) != _D (%d)", samp->size_, D);      // modulated.cc:138-139
    bank_create<StftOp>(samp, name, "NormalFFTAnalysisBank", M, DSR_T_COMPLEX, M, out, [&](StftOp& s) { return dsr_stft_create(M, r, windowType, &s.plan); });
  });
}
dsr_status dsr_synthesis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, int dct, int gain, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_COMPLEX, "OverSampledDFTSynthesisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    if (samp->size_ != M) throw Error(DSR_E_DIMENSION, "Input size (%d) != M (%d)", samp->size_, M);
    bank_create<SynthesisOp>(samp, name, "OverSampledDFTSynthesisBank", M >> r, DSR_T_FLOAT, M / 2 + 1, out,
                             [&](SynthesisOp& s) { s.hermitian = true; return dsr_fb_create(prototype, M, m, r, 1, dct, gain, &s.fb); });
  });
}
dsr_status dsr_wpe_single_stream_create(dsr_stream* samples, int lowerN, int upperN, int iterationsN, double loadDb, double bandWidth, double sampleRate,
                                        const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samples, DSR_T_COMPLEX, "SingleChannelWPEDereverberationFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (upperN < lowerN) throw Error(DSR_E_PARAMETER, "bad prediction range [%d, %d]", lowerN, upperN);
    if (bandWidth > sampleRate / 2.0) throw Error(DSR_E_DIMENSION, "Bandwidth is greater than the Nyquist rate.");
    WpeOp* s = mk<WpeOp>(name, "SingleChannelWPEDereverberationFeature", samples->size_, DSR_T_COMPLEX);
    s->M = samples->size_; s->lowerN = lowerN; s->upperN = upperN; s->iterationsN = iterationsN; s->loadDb = loadDb; s->bandWidth = bandWidth; s->sampleRate = sampleRate;
    s->add_up(samples); *out = s;
  });
}
dsr_status dsr_wpe_multi_feature_create(dsr_stream* const* channels, int channelsN, int channelX, int lowerN, int upperN, int iterationsN, double loadDb,
                                        double bandWidth, double sampleRate, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!channels || !out || channelsN < 1) throw Error(DSR_E_PARAMETER, "null argument");
    if (channelX < 0 || channelX >= channelsN) throw Error(DSR_E_INDEX, "channel %d of %d", channelX, channelsN);
    for (int c = 0; c < channelsN; c++) { need(channels[c], DSR_T_COMPLEX, "MultiChannelWPEDereverberation"); if (channels[c]->size_ != channels[0]->size_) throw Error(DSR_E_DIMENSION, "channel %d has %d subbands, channel 0 %d", c, channels[c]->size_, channels[0]->size_); }
    if (upperN < lowerN) throw Error(DSR_E_PARAMETER, "bad prediction range [%d, %d]", lowerN, upperN);
    if (bandWidth > sampleRate / 2.0) throw Error(DSR_E_DIMENSION, "Bandwidth is greater than the Nyquist rate.");
    WpeMultiOp* s = mk<WpeMultiOp>(name, "MultiChannelWPEDereverberationFeature", channels[0]->size_, DSR_T_COMPLEX);
    s->M = channels[0]->size_; s->channelX = channelX; s->lowerN = lowerN; s->upperN = upperN; s->iterationsN = iterationsN; s->loadDb = loadDb; s->bandWidth = bandWidth; s->sampleRate = sampleRate;
    for (int c = 0; c < channelsN; c++) s->add_up(channels[c]);
    s->checkOrder = true; *out = s;                      // getOutput: jindex_error on out-of-order requests (:371-372)
  });
}
dsr_status dsr_aec_stream_create(dsr_aec* aec, dsr_stream* played, dsr_stream* recorded, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!aec || !out) throw Error(DSR_E_PARAMETER, "null argument");
    need(played, DSR_T_COMPLEX, "EchoCancellationFeature"); need(recorded, DSR_T_COMPLEX, "EchoCancellationFeature");
    if (played->size_ != dsr_aec_fft_len(aec) || recorded->size_ != played->size_)
      throw Error(DSR_E_DIMENSION, "played has %d subbands, recorded %d, the echo canceller %d", played->size_, recorded->size_, dsr_aec_fft_len(aec));
    AecOp* s = mk<AecOp>(name, "AEC", played->size_, DSR_T_COMPLEX);
    s->aec = aec; s->M = played->size_; s->add_up(played); s->add_up(recorded); *out = s;
  });
}
dsr_status dsr_cctde_stream_create(dsr_stream* samp1, dsr_stream* samp2, int fftLen, int nHeldMaxCC, int freqLowerLimit, int freqUpperLimit, const char* name,
                                   dsr_stream** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    const SampleSrc* a = dynamic_cast<const SampleSrc*>(samp1); const SampleSrc* b = dynamic_cast<const SampleSrc*>(samp2);
    if (!a || !b) throw Error(DSR_E_TYPE, "CCTDE needs two SampleFeatures");
    if (a->sampleRate != b->sampleRate) throw Error(DSR_E_DIMENSION, "The sampling rates must be the same but %d != %d", a->sampleRate, b->sampleRate);   // CCTDE.cc:76-80
    if (a->size_ != b->size_) throw Error(DSR_E_DIMENSION, "Block sizes must be the same but %d != %d", a->size_, b->size_);
    (void) fftLen;                                                       // ignored there too: the length is the power of two that holds a block (CCTDE.cc:62-63)
    int N = 1; while (N < a->size_) N *= 2;
    ok(dsr_cctde_check(N, nHeldMaxCC));
    CctdeOp* s = mk<CctdeOp>(name, "CCTDE", nHeldMaxCC, DSR_T_DOUBLE);
    s->N = N; s->nHeld = nHeldMaxCC; s->lower = freqLowerLimit; s->upper = freqUpperLimit; s->vec.assign(nHeldMaxCC, 0.0); s->args.assign(nHeldMaxCC, 0); s->vals.assign(nHeldMaxCC, 0.0);
    s->checkOrder = false; s->add_up(samp1); s->add_up(samp2); *out = s;
  });
}
namespace { CctdeOp* cctde_op(dsr_stream* s) { CctdeOp* q = dynamic_cast<CctdeOp*>(s); if (!q) throw Error(DSR_E_PARAMETER, "not a CCTDE stream"); return q; } }
dsr_status dsr_cctde_stream_next_x(dsr_stream* s, int chanX, int frameX, const void** data, size_t* n)
{ return guard([&] { CctdeOp& q = *cctde_op(s); if (!data) throw Error(DSR_E_PARAMETER, "null argument"); *data = q.nextX(chanX, frameX); if (n) *n = (size_t) q.nHeld; }); }
dsr_status dsr_cctde_stream_allsamples(dsr_stream* s, int fftLen) { return guard([&] { cctde_op(s)->allsamples(fftLen); }); }
dsr_status dsr_cctde_stream_get_sample_delays(dsr_stream* s, const int32_t** lags, size_t* n)
{ return guard([&] { CctdeOp& q = *cctde_op(s); if (!lags) throw Error(DSR_E_PARAMETER, "null argument"); *lags = q.args.data(); if (n) *n = q.args.size(); }); }
dsr_status dsr_cctde_stream_get_cc_values(dsr_stream* s, const double** values, size_t* n)
{ return guard([&] { CctdeOp& q = *cctde_op(s); if (!values) throw Error(DSR_E_PARAMETER, "null argument"); *values = q.vals.data(); if (n) *n = q.vals.size(); }); }
dsr_status dsr_cctde_stream_set_target_frequency_range(dsr_stream* s, int freqLowerLimit, int freqUpperLimit)
{ return guard([&] { CctdeOp& q = *cctde_op(s); q.lower = freqLowerLimit; q.upper = freqUpperLimit; }); }
dsr_status dsr_mcc_stream_create(dsr_mcc* mcc, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!mcc || !out) throw Error(DSR_E_PARAMETER, "null argument");
    MccOp* s = mk<MccOp>(name, "MCCSourceLocalizer", 3, DSR_T_DOUBLE); s->mcc = mcc; s->init(); s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_mcccalc_stream_create(dsr_mcc* mcc, int normalizeVariance, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!mcc || !out) throw Error(DSR_E_PARAMETER, "null argument");
    MccOp* s = mk<MccOp>(name, "MCCCalculator", 3, DSR_T_DOUBLE); s->mcc = mcc; s->calc = true; s->normalize = normalizeVariance != 0; s->init(); s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_mcc_stream_set_channel(dsr_stream* s, dsr_stream* chan)
{
  return guard([&] {
    MccOp* q = as_op<MccOp>(s, "MCC"); need(chan, DSR_T_FLOAT, "MCCLocalizer");
    if (!q->ups.empty() && q->ups[0]->size_ != chan->size_) throw Error(DSR_E_DIMENSION, "Block sizes must be the same but %d != %d", q->ups[0]->size_, chan->size_);
    q->add_up(chan);
  });
}
dsr_status dsr_mcccalc_stream_set_time_delays(dsr_stream* s, const double* delays, int n)
{
  return guard([&] {
    MccOp* q = as_op<MccOp>(s, "MCC"); if (!q->calc || !delays) throw Error(DSR_E_PARAMETER, "not an MCCCalculator stream");
    if (n != q->C) throw Error(DSR_E_DIMENSION, "%d delays for %d channels", n, q->C);
    q->delays.assign(delays, delays + n); q->haveDelays = true;
  });
}
dsr_status dsr_mcc_stream_get(dsr_stream* s, int what, int nth, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    MccOp* q = as_op<MccOp>(s, "MCC"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (what != DSR_MCC_GET_R && (nth < 0 || nth >= q->S)) throw Error(DSR_E_INDEX, "entry %d of %d", nth, q->S);
    const size_t C = (size_t) q->C; size_t m = 0;
    switch (what) {
      case DSR_MCC_GET_COST: m = 1; break; case DSR_MCC_GET_TAU: case DSR_MCC_GET_EIGEN: m = C; break; case DSR_MCC_GET_POSITION: m = 3; break;
      case DSR_MCC_GET_R: m = C * C; break; default: throw Error(DSR_E_PARAMETER, "unknown part %d", what);
    }
    if (outDoubles < m) throw Error(DSR_E_DIMENSION, "part %d needs %zu doubles, the buffer holds %zu", what, m, outDoubles);
    for (size_t i = 0; i < m; i++)
      out[i] = what == DSR_MCC_GET_COST ? q->cost[nth] : what == DSR_MCC_GET_TAU ? (double) q->tau[nth * C + i] : what == DSR_MCC_GET_POSITION ? q->pos[nth * 3 + i]
             : what == DSR_MCC_GET_EIGEN ? q->eig[nth * C + i] : q->R[i];
    if (n) *n = m;
  });
}
int dsr_cctde_stream_fft_len(const dsr_stream* s) { const CctdeOp* q = dynamic_cast<const CctdeOp*>(s); return q ? q->N : 0; }
dsr_status dsr_aec_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    AecOp* q = dynamic_cast<AecOp*>(s); if (!q || !out) throw Error(DSR_E_PARAMETER, "not an echo cancellation stream");
    require_device(); q->ensure_state();
    const size_t F = (size_t) q->M / 2 + 1, L = (size_t) dsr_aec_sample_n(q->aec);
    const size_t cnt = what == DSR_AEC_STATE_K ? F * L * L * 2 : what == DSR_AEC_STATE_SIGMA2V ? F : what == DSR_AEC_STATE_DTD ? 3 : what == DSR_AEC_STATE_BAND ? F * 3 :
                       (what == DSR_AEC_STATE_SKIPPED || what == DSR_AEC_STATE_RESETS) ? 1 : F * L * 2;
    ok(dsr_aec_state_read(q->aec, q->state.p, 1, what, out, outDoubles));
    if (n) *n = cnt;
  });
}
dsr_status dsr_wpe_multi_feature_set_filter_channel(dsr_stream* feature, int filterChan)
{
  return guard([&] {
    WpeMultiOp* q = dynamic_cast<WpeMultiOp*>(feature); if (!q) throw Error(DSR_E_PARAMETER, "not a MultiChannelWPEDereverberationFeature");
    if (filterChan >= (int) q->ups.size()) throw Error(DSR_E_INDEX, "filter channel %d of %d", filterChan, (int) q->ups.size());
    q->filterChan = filterChan < 0 ? -1 : filterChan; q->ready = false;
  });
}
dsr_status dsr_zelinski_stream_create(dsr_stream* output, int fftLen, double alpha, int type, int minFrames, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(output, DSR_T_COMPLEX, "ZelinskiPostFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (output->size_ != fftLen) throw Error(DSR_E_DIMENSION, "Input block length (%d) != fftLen (%d)", output->size_, fftLen);      // postfilter.cc:359-362
    ZelinskiOp* s = mk<ZelinskiOp>(name, "ZelinskPostFilter", fftLen, DSR_T_COMPLEX); s->M = fftLen; s->alpha = alpha; s->ptype = type; s->minFrames = minFrames;
    s->manifold.assign((size_t) fftLen / 2 + 1, std::vector<double>()); s->checkOrder = false;
    s->add_up(output); *out = s;
  });
}
dsr_status dsr_mccowan_stream_create(dsr_stream* output, int fftLen, double alpha, int type, int minFrames, float threshold, const char* name, dsr_stream** out)
{
  const dsr_status s0 = dsr_zelinski_stream_create(output, fftLen, alpha, type, minFrames, (name && *name) ? name : "McCowanPostFilterPtr", out);
  if (s0 != DSR_OK) return s0;
  ZelinskiOp* q = static_cast<ZelinskiOp*>(*out); q->kind = 1; q->threshold = threshold;
  return DSR_OK;
}
dsr_status dsr_lefkimmiatis_stream_create(dsr_stream* output, int fftLen, double minSV, int fbinX1, double alpha, int type, int minFrames, float threshold,
                                          const char* name, dsr_stream** out)
{
  const dsr_status s0 = dsr_zelinski_stream_create(output, fftLen, alpha, type, minFrames, (name && *name) ? name : "LefkimmiatisPostFilte", out);
  if (s0 != DSR_OK) return s0;
  ZelinskiOp* q = static_cast<ZelinskiOp*>(*out); q->kind = 2; q->threshold = threshold; q->minSV = minSV; q->fbinX1 = fbinX1;
  return DSR_OK;
}
// noise coherence setters of McCowanPostFilter (postfilter.cc:546-682); chanN fixes the array size at the first call
dsr_status dsr_mccowan_stream_set_noise(dsr_stream* pf, int what, int fbinX, const double* data, int chanN, double a, double b)
{
  return guard([&] {
    ZelinskiOp* q = dynamic_cast<ZelinskiOp*>(pf); if (!q || q->kind < 1) throw Error(DSR_E_PARAMETER, "not a McCowan post-filter");
    q->ensure_plan(chanN); dsr_status s = DSR_OK;
    switch (what) {
    case 0: s = dsr_mccowan_set_noise_matrix(q->plan, fbinX, data); break;
    case 1: s = dsr_mccowan_set_diffuse_noise_model(q->plan, data, a, b); break;
    case 2: s = dsr_mccowan_diagonal_loading(q->plan, fbinX, (float) a); break;
    case 3: s = dsr_mccowan_divide_nondiagonal(q->plan, (float) a); break;
    default: throw Error(DSR_E_PARAMETER, "bad selector %d", what);
    }
    ok(s);
    q->ready = false;
  });
}
dsr_status dsr_zelinski_stream_set_channel(dsr_stream* pf, dsr_stream* chan)
{
  return guard([&] {
    ZelinskiOp* q = dynamic_cast<ZelinskiOp*>(pf); if (!q) throw Error(DSR_E_PARAMETER, "not a Zelinski post-filter");
    need(chan, DSR_T_COMPLEX, "ZelinskiPostFilter channel"); if (chan->size_ != q->M) throw Error(DSR_E_DIMENSION, "channel size %d != fftLen %d", chan->size_, q->M);
    q->add_up(chan); q->ready = false;
  });
}
dsr_status dsr_zelinski_stream_set_manifold(dsr_stream* pf, int fbinX, const double* vec, int chanN)
{
  return guard([&] {
    ZelinskiOp* q = dynamic_cast<ZelinskiOp*>(pf); if (!q || !vec) throw Error(DSR_E_PARAMETER, "not a Zelinski post-filter");
    if (fbinX < 0 || fbinX >= q->M) throw Error(DSR_E_DIMENSION, "fbinX %d must be less than %d", fbinX, q->M);
    if (fbinX <= q->M / 2) q->manifold[fbinX].assign(vec, vec + 2 * (size_t) chanN);
    q->chanSet = chanN; q->ready = false;
  });
}
// SpectralSubtractorPtr(fftLen, halfBandShift, ft, flooringV, nm) (postfilter.i:182-184)
dsr_status dsr_specsub_stream_create(int fftLen, int halfBandShift, float ft, float flooringV, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    std::unique_ptr<SpecSubOp> s(mk<SpecSubOp>(name, "SpectralSubtractor", fftLen, DSR_T_COMPLEX)); s->M = fftLen; s->checkOrder = false;
    ok(dsr_specsub_create(fftLen, halfBandShift, ft, flooringV, &s->h)); *out = s.release();
  });
}
dsr_status dsr_specsub_stream_set_channel(dsr_stream* ss, dsr_stream* chan, double alpha)
{
  return guard([&] {
    SpecSubOp* q = as_op<SpecSubOp>(ss, "SpectralSubtractor"); need(chan, DSR_T_COMPLEX, "SpectralSubtractor channel");
    if (chan->size_ != q->M) throw Error(DSR_E_DIMENSION, "channel size %d != fftLen %d", chan->size_, q->M);
    if (q->stateC) throw Error(DSR_E_CONSISTENCY, "setChannel() after the noise estimates are in use");
    ok(dsr_specsub_set_channel(q->h, alpha)); q->add_up(chan); q->ready = false;
  });
}
// what: 0 setNoiseOverEstimationFactor(value), 1 startTraining, 2 stopTraining, 3 startNoiseSubtraction, 4 stopNoiseSubtraction, 5 clear,
// 6 clearNoiseSamples, 7 readNoiseFile(fn, idx), 8 writeNoiseFile(fn, idx) (spectralsubtraction.h:75-118).  The frames of an utterance are
// computed at its first next(): a call takes effect from the next reset() on.
dsr_status dsr_specsub_stream_control(dsr_stream* ss, int what, double value, const char* fn, int idx)
{
  return guard([&] {
    SpecSubOp* q = as_op<SpecSubOp>(ss, "SpectralSubtractor");
    switch (what) {
    case 0: ok(dsr_specsub_set_noise_over_estimation_factor(q->h, (float) value)); break;
    case 1: ok(dsr_specsub_start_training(q->h)); break;
    case 2: ok(dsr_specsub_stop_training(q->h, q->ups.empty() ? nullptr : q->st(), 1, S0)); break;
    case 3: case 4: ok(dsr_specsub_set_noise_subtraction(q->h, what == 3)); break;
    case 5: if (!q->ups.empty()) ok(dsr_specsub_clear(q->h, q->st(), 1, S0)); break;
    case 6: if (!q->ups.empty()) ok(dsr_specsub_clear_noise_samples(q->h, q->st(), 1, S0)); break;
    case 7: ok(dsr_specsub_read_noise_file(q->h, fn, idx, q->ups.empty() ? nullptr : q->st(), 1)); break;
    case 8: ok(dsr_specsub_write_noise_file(q->h, fn, idx, q->ups.empty() ? nullptr : q->st(), 1, 0)); break;
    default: throw Error(DSR_E_PARAMETER, "bad selector %d", what);
    }
    q->ready = false;
  });
}
dsr_status dsr_wiener_stream_create(dsr_stream* targetSignal, dsr_stream* noiseSignal, int halfBandShift, float alpha, float flooringV, double beta, const char* name,
                                    dsr_stream** out)
{
  return guard([&] {
    need(targetSignal, DSR_T_COMPLEX, "WienerFilter"); need(noiseSignal, DSR_T_COMPLEX, "WienerFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    std::unique_ptr<WienerOp> s(mk<WienerOp>(name, "WienerFilter", targetSignal->size_, DSR_T_COMPLEX)); s->M = targetSignal->size_; s->checkOrder = false;
    ok(dsr_wiener_create(targetSignal->size_, noiseSignal->size_, halfBandShift, alpha, flooringV, beta, &s->h)); ok(dsr_wiener_carry(s->h, 1));
    s->add_up(targetSignal); s->add_up(noiseSignal); *out = s.release();
  });
}
// what: 0 setNoiseAmplificationFactor(value), 1 startUpdatingNoisePSD, 2 stopUpdatingNoisePSD
dsr_status dsr_wiener_stream_control(dsr_stream* wf, int what, double value)
{
  return guard([&] {
    WienerOp* q = as_op<WienerOp>(wf, "WienerFilter");
    if (what == 0) ok(dsr_wiener_set_noise_amplification_factor(q->h, value)); else if (what == 1 || what == 2) ok(dsr_wiener_set_updating_noise_psd(q->h, what == 1));
    else throw Error(DSR_E_PARAMETER, "bad selector %d", what);
    q->ready = false;
  });
}
// BinaryMaskFilterPtr / KimBinaryMaskFilterPtr / IIDBinaryMaskFilterPtr(chanX, srcL, srcR, M, threshold, alpha, dEta[, dPowerCoeff], nm) (postfilter.i:274-368)
dsr_status dsr_binmask_stream_create(int kind, unsigned chanX, dsr_stream* srcL, dsr_stream* srcR, unsigned M, float threshold, float alpha, float dEta,
                                     float dPowerCoeff, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(srcL, DSR_T_COMPLEX, "BinaryMaskFilter"); need(srcR, DSR_T_COMPLEX, "BinaryMaskFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (srcL->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Left input block length (%d) != M (%d)", srcL->size_, (int) M);       // binauralprocessing.cc:58-66
    if (srcR->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Right input block length (%d) != M (%d)", srcR->size_, (int) M);
    std::unique_ptr<MaskOp> s(mk<MaskOp>(name, kind == 1 ? "KimBinaryMaskFilter" : kind == 2 ? "IIDBinaryMaskFilter" : "BinaryMaskFilter", (int) M, DSR_T_COMPLEX));
    s->M = (int) M; s->checkOrder = false;
    ok(dsr_binmask_create(kind, chanX, (int) M, threshold, alpha, dEta, dPowerCoeff, &s->h)); ok(dsr_binmask_carry(s->h, 1));
    s->add_up(srcL); s->add_up(srcR); *out = s.release();
  });
}
dsr_status dsr_binmask_stream_set_threshold(dsr_stream* m, float threshold)
{ return guard([&] { MaskOp* q = as_op<MaskOp>(m, "BinaryMaskFilter"); ok(dsr_binmask_set_threshold(q->h, threshold)); q->ready = false; }); }
dsr_status dsr_binmask_stream_threshold(dsr_stream* m, double* threshold)
{ return guard([&] { if (!threshold) throw Error(DSR_E_PARAMETER, "null argument"); *threshold = dsr_binmask_threshold(as_op<MaskOp>(m, "BinaryMaskFilter")->h); }); }
dsr_status dsr_binmask_stream_set_thresholds(dsr_stream* m, const double* thresholds, int n)
{ return guard([&] { MaskOp* q = as_op<MaskOp>(m, "BinaryMaskFilter"); ok(dsr_binmask_set_thresholds(q->h, thresholds, n)); q->ready = false; }); }
dsr_status dsr_binmask_stream_thresholds(dsr_stream* m, double* out, int n, int32_t* exists)
{ return guard([&] { ok(dsr_binmask_thresholds(as_op<MaskOp>(m, "BinaryMaskFilter")->h, out, n, exists)); }); }
// KimITDThresholdEstimatorPtr / IIDThresholdEstimatorPtr / FDIIDThresholdEstimatorPtr (postfilter.i:332-428)
dsr_status dsr_thest_stream_create(int kind, dsr_stream* srcL, dsr_stream* srcR, unsigned M, float minThreshold, float maxThreshold, float width, float minFreq,
                                   float maxFreq, int sampleRate, float dEta, float dPowerCoeff, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(srcL, DSR_T_COMPLEX, "ThresholdEstimator"); need(srcR, DSR_T_COMPLEX, "ThresholdEstimator"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (srcL->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Left input block length (%d) != M (%d)", srcL->size_, (int) M);
    if (srcR->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Right input block length (%d) != M (%d)", srcR->size_, (int) M);
    std::unique_ptr<ThestOp> s(mk<ThestOp>(name, kind == 0 ? "KimITDThresholdEstimator" : kind == 1 ? "IIDThresholdEstimator" : "FDIIDThresholdEstimator", (int) M, DSR_T_COMPLEX));
    s->M = (int) M; s->checkOrder = false;
    ok(dsr_thest_create(kind, (int) M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, &s->h));
    s->add_up(srcL); s->add_up(srcR); *out = s.release();
  });
}
dsr_status dsr_thest_stream_calc_threshold(dsr_stream* e, double* threshold)
{ return guard([&] { if (!threshold) throw Error(DSR_E_PARAMETER, "null argument"); *threshold = as_op<ThestOp>(e, "ThresholdEstimator")->calc(); }); }
dsr_status dsr_thest_stream_threshold(dsr_stream* e, double* threshold)
{ return guard([&] { if (!threshold) throw Error(DSR_E_PARAMETER, "null argument"); *threshold = as_op<ThestOp>(e, "ThresholdEstimator")->threshold; }); }
// getCostFunction() / getCostFunction(freqX) of the last calcThreshold (zeros before one, where the reference prints a warning); FDIID: getThresholds
dsr_status dsr_thest_stream_get_cost_function(dsr_stream* e, unsigned freqX, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    ThestOp* q = as_op<ThestOp>(e, "ThresholdEstimator"); if (!out || !n) throw Error(DSR_E_PARAMETER, "null argument");
    const size_t nC = (size_t) dsr_thest_n_cand(q->h); if (outDoubles < nC) throw Error(DSR_E_DIMENSION, "%zu doubles for %zu", outDoubles, nC);
    const bool fd = dsr_thest_kind(q->h) == DSR_THEST_FDIID;
    if (fd && freqX > (unsigned) q->M / 2) throw Error(DSR_E_INDEX, "bin %u of %d", freqX, q->M / 2 + 1);
    std::fill(out, out + nC, 0.0); *n = nC;
    if (!q->cost.empty()) std::copy(q->cost.begin() + (fd ? freqX * nC : 0), q->cost.begin() + (fd ? freqX * nC : 0) + nC, out);
  });
}
int dsr_thest_stream_n_cand(dsr_stream* e) { ThestOp* q = dynamic_cast<ThestOp*>(e); return q ? dsr_thest_n_cand(q->h) : 0; }
dsr_status dsr_thest_stream_thresholds(dsr_stream* e, double* out, int n)
{
  return guard([&] {
    ThestOp* q = as_op<ThestOp>(e, "ThresholdEstimator"); if (!out || n < q->M / 2 + 1) throw Error(DSR_E_DIMENSION, "%d doubles for %d bins", n, q->M / 2 + 1);
    std::fill(out, out + q->M / 2 + 1, 0.0); if (!q->thresholds.empty()) std::copy(q->thresholds.begin(), q->thresholds.end(), out);
  });
}
dsr_status dsr_subband_bf_create(dsr_bf* weights, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!weights || !out) throw Error(DSR_E_PARAMETER, "null argument");
    BfOp* s = mk<BfOp>(name, "SubbandBeamformer", dsr_bf_fft_len(weights), DSR_T_COMPLEX); s->w = weights; s->M = dsr_bf_fft_len(weights); s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_subband_mmi_stream_create(dsr_mmi* weights, int fftLen, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!weights || !out) throw Error(DSR_E_PARAMETER, "null argument");
    MmiOp* s = mk<MmiOp>(name, "SubbandMMI", fftLen, DSR_T_COMPLEX); s->w = nullptr; s->mm = weights; s->M = fftLen; s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_doa_stream_create(dsr_doa* doa, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!doa || !out) throw Error(DSR_E_PARAMETER, "null argument");
    DoaOp* s = mk<DoaOp>(name, "DOAEstimatorSRPDSBLAPtr", dsr_doa_fft_len(doa), DSR_T_COMPLEX); s->w = nullptr; s->est = doa; s->M = dsr_doa_fft_len(doa);
    s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_doa_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n)
{ return guard([&] { srp_op<DoaOp>(s, out && n).get(what, out, outDoubles, n); }); }
dsr_status dsr_doa_stream_init_accs(dsr_stream* s) { return guard([&] { srp_op<DoaOp>(s).init_accs(); }); }
dsr_status dsr_doa_stream_final_nbest(dsr_stream* s) { return guard([&] { srp_op<DoaOp>(s).final_nbest(); }); }
dsr_status dsr_sph_bf_stream_create(dsr_sph* sph, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!sph || !out) throw Error(DSR_E_PARAMETER, "null argument");
    static const char* const NAMES[] = {"EigenBeamformer", "SphericalDSBeamformer", "SphericalHWNCBeamformer", "SphericalGSCBeamformer",
                                        "SphericalHWNCGSCBeamformer", "SphericalSpatialDSBeamformer", "SphericalMOENBeamformer"};
    const char* dflt = NAMES[dsr_sph_kind(sph)];
    SphBfOp* s = mk<SphBfOp>(name, dflt, dsr_sph_fft_len(sph), DSR_T_COMPLEX); s->w = nullptr; s->sph = sph; s->M = dsr_sph_fft_len(sph);
    s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_sph_stream_get_eigenbeams(dsr_stream* s, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    SphBfOp* q = dynamic_cast<SphBfOp*>(s); if (!q || !out || !n) throw Error(DSR_E_PARAMETER, "not a spherical beamformer stream");
    if (q->F == 0) { q->F = q->M / 2 + 1; q->dim = dsr_sph_dim(q->sph); }
    const size_t need = (size_t) q->F * q->dim * 2;
    if (outDoubles < need) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, need);
    q->eigenbeams(out); *n = need;
  });
}
dsr_status dsr_trk_stream_create(dsr_trk* trk, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!trk || !out) throw Error(DSR_E_ARG, "null argument");
    TrkOp* s = mk<TrkOp>(name, "SphericalArrayTracker", 2, DSR_T_FLOAT); s->trk = trk; s->M = dsr_trk_fft_len(trk); s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_trk_stream_set_channel(dsr_stream* s, dsr_stream* chan)
{
  return guard([&] {
    TrkOp* q = as_op<TrkOp>(s, "tracker"); need(chan, DSR_T_COMPLEX, "setChannel");
    if (chan->size_ != q->M) throw Error(DSR_E_DIMENSION, "channel size %d != fftLen %d", chan->size_, q->M);
    q->add_up(chan); q->ready = false;
  });
}
dsr_status dsr_trk_stream_next_speaker(dsr_stream* s)
{ return guard([&] { TrkOp* q = as_op<TrkOp>(s, "tracker"); q->reset(); ok(dsr_trk_next_speaker(q->trk)); q->stateReady = false; q->posPending = false; }); }
dsr_status dsr_trk_stream_set_initial_position(dsr_stream* s, double theta, double phi)
{
  return guard([&] {
    TrkOp* q = as_op<TrkOp>(s, "tracker"); q->posPending = true; q->pTheta = theta; q->pPhi = phi; q->ready = false;      // applied when the next frame is computed
  });
}
dsr_status dsr_pws_stream_create(dsr_stream* source, const dsr_trk* decomposition, unsigned channelX, double theta, double phi, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!decomposition || !out) throw Error(DSR_E_ARG, "null argument");
    need(source, DSR_T_COMPLEX, "PlaneWaveSimulator");
    const int M = dsr_trk_fft_len(decomposition), F = M / 2 + 1;
    if (channelX >= 32 || source->size_ < F) throw Error(DSR_E_ARG, "channel %u of 32, a source of at least %d bins", channelX, F);
    std::vector<double> all((size_t) 2 * 32 * F); ok(dsr_pws_coefficients(decomposition, theta, phi, all.data(), all.size()));
    std::unique_ptr<PwsOp> s(mk<PwsOp>(name, "Plane Wave Simulator", M, DSR_T_COMPLEX)); s->M = M; s->checkOrder = false;
    const double2* row = reinterpret_cast<const double2*>(all.data()) + (size_t) channelX * F; s->hcoef.assign(row, row + F);
    s->add_up(source); *out = s.release();
  });
}
dsr_status dsr_sph_doa_stream_create(dsr_sph* sph, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!sph || !out) throw Error(DSR_E_PARAMETER, "null argument");
    const char* dflt = "DirectionEstimatorSRPMB";               // both classes' default name (beamformer.i:539, :624)
    SphDoaOp* s = mk<SphDoaOp>(name, dflt, dsr_sph_fft_len(sph), DSR_T_COMPLEX); s->w = nullptr; s->sph = s->est = sph; s->M = dsr_sph_fft_len(sph);
    s->checkOrder = false; *out = s;
  });
}
dsr_status dsr_sph_doa_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n)
{ return guard([&] { srp_op<SphDoaOp>(s, out && n).get(what, out, outDoubles, n); }); }
dsr_status dsr_sph_doa_stream_init_accs(dsr_stream* s) { return guard([&] { srp_op<SphDoaOp>(s).init_accs(); }); }
dsr_status dsr_sph_doa_stream_final_nbest(dsr_stream* s) { return guard([&] { srp_op<SphDoaOp>(s).final_nbest(); }); }
dsr_status dsr_subband_orthogonalizer_create(dsr_stream* beamformer, int outChanX, const char* name, dsr_stream** out)
{
  return guard([&] {
    BfOp* q = dynamic_cast<BfOp*>(beamformer); if (!q || !q->w || !out) throw Error(DSR_E_PARAMETER, "not a subband beamformer");
    OrthOp* s = mk<OrthOp>(name, "SubbandOrthogonalizer", q->M, DSR_T_COMPLEX); s->outChanX = outChanX; s->checkOrder = false;
    s->add_up(beamformer); *out = s;
  });
}
dsr_status dsr_subband_bf_set_channel(dsr_stream* bf, dsr_stream* chan)
{
  return guard([&] {
    BfOp* q = dynamic_cast<BfOp*>(bf); if (!q) throw Error(DSR_E_PARAMETER, "not a subband beamformer");
    need(chan, DSR_T_COMPLEX, "setChannel"); if (chan->size_ != q->M) throw Error(DSR_E_DIMENSION, "channel size %d != fftLen %d", chan->size_, q->M);
    q->add_up(chan); q->ready = false;
  });
}
dsr_status dsr_preemphasis_create(dsr_stream* samp, double mu, const char* name, dsr_stream** out)
{ return guard([&] { need(samp, DSR_T_FLOAT, "PreemphasisFeature"); Preemph* s = mk<Preemph>(name, "Preemphasis", samp->size_, DSR_T_FLOAT); s->mu = mu; s->add_up(samp); *out = s; }); }
dsr_status dsr_hamming_create(dsr_stream* samp, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!samp || (samp->type != DSR_T_FLOAT && samp->type != DSR_T_SHORT)) throw Error(DSR_E_TYPE, "HammingFeature needs a float or short stream");
    Hamming* s = mk<Hamming>(name, "Hamming", samp->size_, DSR_T_FLOAT);
    std::vector<double> w(samp->size_); const double temp = 2. * M_PI / (double) (samp->size_ - 1);
    for (int i = 0; i < samp->size_; i++) w[i] = 0.54 - 0.46 * cos(temp * i);
    require_device(); s->w.upload(w); s->add_up(samp); *out = s;
  });
}
dsr_status dsr_highpass_filter_create(dsr_stream* output, float cutOffFreq, int sampleRate, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(output, DSR_T_COMPLEX, "highPassFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (sampleRate <= 0) throw Error(DSR_E_PARAMETER, "sample rate %d", sampleRate);
    const unsigned cut = (unsigned) ((float) output->size_ * cutOffFreq / (float) sampleRate);                 // postfilter.cc:1228
    if (cut < 1 || cut > (unsigned) output->size_ / 2) throw Error(DSR_E_INDEX, "highPassFilter: the cut-off bin %u must lie in 1..%d (the reference writes outside its vector otherwise)", cut, output->size_ / 2);
    HighPassOp* s = mk<HighPassOp>(name, "highPassFilter", output->size_, DSR_T_COMPLEX); s->cut = (int) cut; s->checkOrder = false;
    s->add_up(output); *out = s;
  });
}
dsr_status dsr_fft_create(dsr_stream* samp, int fftLen, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "FFTFeature");
    if (!is_pow2((unsigned) fftLen) || fftLen < 2 || fftLen > 8192 || samp->size_ > fftLen) throw Error(DSR_E_DIMENSION, "fftLen=%d must be a power of two >= the window length %d", fftLen, samp->size_);
    FFTOp* s = mk<FFTOp>(name, "FFT", fftLen, DSR_T_COMPLEX); s->L = samp->size_;
    std::vector<double2> tw(fftLen); for (int k = 0; k < fftLen; k++) { const double a = 2.0 * M_PI * k / fftLen; tw[k] = make_double2(cos(a), sin(a)); }
    require_device(); s->tw.upload(tw); s->add_up(samp); *out = s;
  });
}
dsr_status dsr_spectral_power_create(dsr_stream* fft, int powN, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(fft, DSR_T_COMPLEX, "SpectralPowerFeature"); const int sz = powN == 0 ? fft->size_ : powN;
    if (sz != fft->size_ && sz != fft->size_ / 2 + 1) throw Error(DSR_E_CONSISTENCY, "Number of power coefficients %d does not match FFT length %d.", sz, fft->size_);
    PowerOp* s = mk<PowerOp>(name, "Power", sz, DSR_T_DOUBLE); s->fftLen = fft->size_; s->add_up(fft); *out = s;
  });
}
dsr_status dsr_vtln_create(dsr_stream* pow, int coeffN, double ratio, double edge, int version, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(pow, DSR_T_DOUBLE, "VTLNFeature"); const int N = coeffN == 0 ? pow->size_ : coeffN;
    if (N != pow->size_) throw Error(DSR_E_DIMENSION, "VTLN size %d != input size %d", N, pow->size_);
    if (version != 1 && version != 2) throw Error(DSR_E_PARAMETER, "unknown version number (%d)", version);
    VtlnOp* s = mk<VtlnOp>(name, "VTLN", N, DSR_T_DOUBLE); SparseRowsD r; build_vtln_rows(N, ratio, edge, version, r);
    require_device(); s->s.upload(r.start); s->c.upload(r.count); s->o.upload(r.off); s->coef.upload(r.coef); s->div.upload(r.div); s->rf = r.roundFloat;
    s->add_up(pow); *out = s;
  });
}
dsr_status dsr_mel_create(dsr_stream* mag, int powN, float rate, float low, float up, int filterN, int version, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(mag, DSR_T_DOUBLE, "MelFeature"); const int P = powN == 0 ? mag->size_ : powN;
    std::unique_ptr<MelOp> s(mk<MelOp>(name, "MelFFT", filterN, DSR_T_DOUBLE)); SparseRowsF r; build_mel_rows(P, rate, low, up, filterN, version, r);
    if (mag->size_ < r.nReq) throw Error(DSR_E_CONSISTENCY, "Matrix columns differ: %d and %d.", mag->size_, r.nReq);
    for (size_t i = 0; i < r.start.size(); i++) if (r.start[i] + r.count[i] > mag->size_) throw Error(DSR_E_CONSISTENCY, "mel filter %zu reads past the input", i);
    require_device(); s->s.upload(r.start); s->c.upload(r.count); s->o.upload(r.off); s->coef.upload(r.coef); s->inN = mag->size_;
    s->add_up(mag); *out = s.release();
  });
}
dsr_status dsr_log_create(dsr_stream* mel, double m, double a, int sphinx, const char* name, dsr_stream** out)
{ return guard([&] { need(mel, DSR_T_DOUBLE, "LogFeature"); LogOp* s = mk<LogOp>(name, "LogMel", mel->size_, DSR_T_FLOAT); s->m = m; s->a = a; s->sphinx = sphinx; s->add_up(mel); *out = s; }); }
dsr_status dsr_cepstral_create(dsr_stream* mel, int ncep, int type, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(mel, DSR_T_FLOAT, "CepstralFeature");
    GemvOp* s = mk<GemvOp>(name, "Cepstral", ncep, DSR_T_FLOAT); build_dct(ncep, mel->size_, type, s->hA);
    require_device(); s->A.upload(s->hA); s->add_up(mel); *out = s;
  });
}
dsr_status dsr_lpc_feature_create(dsr_stream* src, int order, int correlate, float warp, int method, int kind, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, kind ? "LPCFeature" : "MVDRFeature");
    dsr_lpc* plan = nullptr;
    ok(dsr_lpc_create(src->size_, order, correlate, warp, method, kind, &plan));
    LpcOp* s = mk<LpcOp>(name, kind ? "LPC" : "MVDR", src->size_ / 2 + 1, DSR_T_DOUBLE); s->plan = plan; s->add_up(src); *out = s;
  });
}
dsr_status dsr_wtmvdr_feature_create(dsr_stream* src, int order, int correlate, float warp, int warpFactorFixed, float sensibility, const char* name,
                                     dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "WarpedTwiceMVDRFeature");
    dsr_wtmvdr* plan = nullptr;
    ok(dsr_wtmvdr_create(src->size_, order, correlate, warp, warpFactorFixed, sensibility, &plan));
    WtMvdrOp* s = mk<WtMvdrOp>(name, "WTMVDR", src->size_ / 2 + 1, DSR_T_DOUBLE); s->plan = plan; s->add_up(src); *out = s;
  });
}
dsr_status dsr_spectral_smoothing_create(dsr_stream* adjustTo, dsr_stream* adjustFrom, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(adjustTo, DSR_T_DOUBLE, "SpectralSmoothing"); need(adjustFrom, DSR_T_DOUBLE, "SpectralSmoothing");
    if (adjustTo->size_ != adjustFrom->size_) throw Error(DSR_E_DIMENSION, "Feature sizes (%d vs. %d) do not match.", adjustTo->size_, adjustFrom->size_);   // lpc.cc:476-477
    if (adjustTo->size_ < 2) throw Error(DSR_E_PARAMETER, "SpectralSmoothing needs at least 2 coefficients, got %d", adjustTo->size_);
    SpecSmoothOp* s = mk<SpecSmoothOp>(name, "Spectral Smoothing", adjustTo->size_, DSR_T_DOUBLE); s->add_up(adjustTo); s->add_up(adjustFrom); *out = s;
  });
}
dsr_status dsr_filter_feature_create(dsr_stream* src, const double* a, int lenA, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "FilterFeature");
    if (!a || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (lenA < 1 || lenA % 2 != 1) throw Error(DSR_E_DIMENSION, "Length of filter (%d) is not odd.", lenA);                  // feature.cc:3219-3220
    FirOp* s = mk<FirOp>(name, "Filter", src->size_, DSR_T_FLOAT); s->a.assign(a, a + lenA); s->add_up(src); *out = s;
  });
}
dsr_status dsr_merge_feature_create(dsr_stream* stat, dsr_stream* delta, dsr_stream* deltaDelta, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(stat, DSR_T_FLOAT, "MergeFeature"); need(delta, DSR_T_FLOAT, "MergeFeature"); need(deltaDelta, DSR_T_FLOAT, "MergeFeature");
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    MergeOp* s = mk<MergeOp>(name, "Merge", stat->size_ + delta->size_ + deltaDelta->size_, DSR_T_FLOAT);
    s->add_up(stat); s->add_up(delta); s->add_up(deltaDelta); *out = s;
  });
}
namespace {
void conv_create(int kind, dsr_stream* src, const double* h, int P, int fftLen, const char* name, const char* dflt, dsr_stream** out)
{
  need(src, DSR_T_FLOAT, dflt);
  if (!out) throw Error(DSR_E_PARAMETER, "null argument");
  if (!h) throw Error(DSR_E_PARAMETER, "null impulse response");
  dsr_conv* plan = nullptr;
  ok(dsr_conv_create(kind, src->size_, P, fftLen, 1, &plan));
  std::unique_ptr<ConvOp> s(mk<ConvOp>(name, dflt, dsr_conv_size(plan), DSR_T_FLOAT)); s->plan = plan;
  ok(dsr_conv_set_response(plan, h));
  s->add_up(src); *out = s.release();
}
}  // namespace
dsr_status dsr_overlap_add_create(dsr_stream* src, const double* h, int P, int fftLen, const char* name, dsr_stream** out)
{ return guard([&] { conv_create(0, src, h, P, fftLen, name, "Overlap Add", out); }); }
dsr_status dsr_overlap_save_create(dsr_stream* src, const double* h, int P, const char* name, dsr_stream** out)
{ return guard([&] { conv_create(1, src, h, P, 0, name, "Overlap Save", out); }); }
dsr_status dsr_overlap_save_update(dsr_stream* s, const double* delta, int n)
{
  return guard([&] {
    ConvOp* q = as_op<ConvOp>(s, "OverlapSave");
    if (!delta) throw Error(DSR_E_PARAMETER, "null argument");
    if (n != q->ups[0]->size_)                                                                                                 // convolution.cc:284-286
      throw Error(DSR_E_DIMENSION, "Dimension of udpate vector (%d) does not match frequency response (%d).", n, q->ups[0]->size_);
    ok(dsr_conv_update(q->plan, 0, delta));
  });
}
dsr_status dsr_signal_power_create(dsr_stream* samp, const char* name, dsr_stream** out)
{ return guard([&] { need(samp, DSR_T_FLOAT, "SignalPowerFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument"); SignalPowerOp* s = mk<SignalPowerOp>(name, "Signal Power", 1, DSR_T_FLOAT); s->add_up(samp); *out = s; }); }
dsr_status dsr_zcr_hamming_create(dsr_stream* samp, const char* name, dsr_stream** out)
{ return guard([&] { need(samp, DSR_T_FLOAT, "ZeroCrossingRateHammingFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument"); ZcrOp* s = mk<ZcrOp>(name, "Zero Crossing Rate Hamming", 1, DSR_T_FLOAT); s->add_up(samp); *out = s; }); }
dsr_status dsr_yin_pitch_create(dsr_stream* samp, unsigned samplerate, float threshold, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "YINPitchFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (samp->size_ < 2) throw Error(DSR_E_DIMENSION, "YIN needs frames of at least 2 samples, got %d.", samp->size_);
    YinOp* s = mk<YinOp>(name, "YIN Pitch", 1, DSR_T_FLOAT); s->sr = samplerate; s->tr = threshold; s->add_up(samp); *out = s;
  });
}
dsr_status dsr_spike_filter_create(dsr_stream* src, unsigned tapN, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "SpikeFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    ok(dsr_spike_filter_check(src->size_, tapN > 0x7fffffffu ? 0x7fffffff : (int) tapN));
    SpikeOp* s = mk<SpikeOp>(name, "Spike Filter", src->size_, DSR_T_FLOAT); s->tapN = (int) tapN; s->add_up(src); *out = s;
  });
}
dsr_status dsr_spike_filter2_create(dsr_stream* src, unsigned width, float maxslope, float startslope, float thresh, float alpha, unsigned verbose, const char* name,
                                    dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "SpikeFilter2"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    (void) verbose;                                                                                                            // its printf passes floats to %d
    if (src->size_ > 16000) throw Error(DSR_E_DIMENSION, "SpikeFilter2 stages a block in LDS: %d samples exceed 16000.", src->size_);
    Spike2Op* s = mk<Spike2Op>(name, "Spike Filter 2", src->size_, DSR_T_FLOAT);
    s->width = width; s->maxslope = maxslope; s->startslope = startslope; s->thresh = thresh; s->alpha = alpha; s->add_up(src); *out = s;
  });
}
dsr_status dsr_spike_filter2_spikes(dsr_stream* s, unsigned* n)
{ return guard([&] { Spike2Op* q = as_op<Spike2Op>(s, "SpikeFilter2"); if (!n) throw Error(DSR_E_PARAMETER, "null argument"); *n = q->spikes; }); }
dsr_status dsr_alog_create(dsr_stream* samp, double m, double a, int runon, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "ALogFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    MinMaxOp* s = mk<MinMaxOp>(name, "ALog Power", 1, DSR_T_FLOAT); s->alog = 1; s->runon = runon != 0; s->p0 = m; s->p1 = a; s->add_up(samp); *out = s;
  });
}
dsr_status dsr_normalize_create(dsr_stream* samp, double min, double max, int runon, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "NormalizeFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    MinMaxOp* s = mk<MinMaxOp>(name, "Normalize", samp->size_, DSR_T_FLOAT); s->runon = runon != 0; s->p0 = min; s->p1 = max; s->add_up(samp); *out = s;
  });
}
dsr_status dsr_minmax_next_speaker(dsr_stream* s)
{ return guard([&] { as_op<MinMaxOp>(s, "ALogFeature or NormalizeFeature")->fresh = true; }); }
dsr_status dsr_threshold_create(dsr_stream* samp, double value, double thresh, const char* mode, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "ThresholdFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    int compare = 0; ok(dsr_threshold_mode(mode, &compare));
    ThreshAmpOp* s = mk<ThreshAmpOp>(name, "Threshold", samp->size_, DSR_T_FLOAT); s->value = value; s->thresh = thresh; s->compare = compare; s->add_up(samp); *out = s;
  });
}
dsr_status dsr_amplification_create(dsr_stream* src, double amplify, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "AmplificationFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    ThreshAmpOp* s = mk<ThreshAmpOp>(name, "Amplification", src->size_, DSR_T_FLOAT); s->value = amplify; s->compare = 2; s->add_up(src); *out = s;
  });
}
dsr_status dsr_spectral_resampling_create(dsr_stream* src, double ratio, unsigned len, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_DOUBLE, "SpectralResamplingFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    int outN = 0; ok(dsr_spectral_resample_size(src->size_, ratio, (int) len, &outN));
    ResampleOp* s = mk<ResampleOp>(name, "Resampling", outN, DSR_T_DOUBLE); s->ratio = ratio; s->len = (int) len; s->add_up(src); *out = s;
  });
}
dsr_status dsr_sphinx_mel_feature_create(dsr_stream* mag, unsigned fftN, unsigned powerN, float sampleRate, float lowerF, float upperF, unsigned filterN,
                                         const char* name, dsr_stream** out)
{
  return guard([&] {
    need(mag, DSR_T_DOUBLE, "SphinxMelFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    const unsigned pN = powerN == 0 ? (unsigned) mag->size_ : powerN;
    if ((int) pN != mag->size_) throw Error(DSR_E_DIMENSION, "SphinxMelFeature: powerN = %u does not match the source's size %d.", pN, mag->size_);   // gsl_blas_dgemv's own check
    dsr_sphinx_mel* plan = nullptr; ok(dsr_sphinx_mel_create(fftN, pN, sampleRate, lowerF, upperF, filterN, &plan));
    SphinxMelOp* s = mk<SphinxMelOp>(name, "Sphinx Mel Filter Bank", (int) filterN, DSR_T_DOUBLE); s->plan = plan; s->add_up(mag); *out = s;
  });
}
dsr_status dsr_storage_create(dsr_stream* src, const char* name, dsr_stream** out)
{ return guard([&] { need(src, DSR_T_FLOAT, "StorageFeature"); StorageOp* s = mk<StorageOp>(name, "Storage", src->size_, DSR_T_FLOAT); s->randomAccess = true; s->checkOrder = false; s->add_up(src); *out = s; }); }
dsr_status dsr_mean_subtraction_create(dsr_stream* src, double dnf, int runon, const char* name, dsr_stream** out)
{ return guard([&] { need(src, DSR_T_FLOAT, "MeanSubtractionFeature"); CmnOp* s = mk<CmnOp>(name, "Mean Subtraction", src->size_, DSR_T_FLOAT); s->mode = runon ? 2 : 1; s->dnf = dnf; s->add_up(src); *out = s; }); }
dsr_status dsr_mean_subtraction_set_weight(dsr_stream* cmn, dsr_stream* weight)
{
  return guard([&] {
    CmnOp* q = dynamic_cast<CmnOp*>(cmn); if (!q) throw Error(DSR_E_PARAMETER, "not a MeanSubtractionFeature");
    need(weight, DSR_T_FLOAT, "MeanSubtractionFeature weight"); if (q->ups.size() > 1) throw Error(DSR_E_CONSISTENCY, "the weight stream is already set");
    q->add_up(weight); q->ready = false;
  });
}
dsr_status dsr_adjacent_create(dsr_stream* single, int delta, const char* name, dsr_stream** out)
{ return guard([&] { need(single, DSR_T_FLOAT, "AdjacentFeature"); AdjOp* s = mk<AdjOp>(name, "Adjacent", (2 * delta + 1) * single->size_, DSR_T_FLOAT); s->delta = delta; s->add_up(single); *out = s; }); }
dsr_status dsr_linear_transform_create(dsr_stream* src, int sz, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "LinearTransformFeature"); if (sz < 1) throw Error(DSR_E_DIMENSION, "bad output size %d", sz);
    GemvOp* s = mk<GemvOp>(name, "Transform", sz, DSR_T_FLOAT); s->hA.assign((size_t) sz * src->size_, 0.0f);     // calloc'd matrix (feature.cc:2936)
    require_device(); s->A.upload(s->hA); s->add_up(src); *out = s;
  });
}
dsr_status dsr_linear_transform_set(dsr_stream* s, const float* matrix)
{
  return guard([&] {
    GemvOp* q = dynamic_cast<GemvOp*>(s); if (!q || !matrix) throw Error(DSR_E_PARAMETER, "not a linear transform");
    q->hA.assign(matrix, matrix + q->hA.size()); q->A.upload(q->hA); q->ready = false;
  });
}

// LinearTransformFeature::load(fileName, old) (feature.cc:2972-2976): gsl_matrix_float_load into the operator's (size x srcSize) matrix, then the
// crop to (size x srcSize) -- which only ever shrinks (gslmatrix.cc:6-15), so a Janus file must carry exactly that shape.
dsr_status dsr_linear_transform_load(dsr_stream* s, const char* fileName, int old)
{
  return guard([&] {
    GemvOp* q = dynamic_cast<GemvOp*>(s); if (!q || !fileName) throw Error(DSR_E_PARAMETER, "not a linear transform");
    const int rows = q->size_, cols = q->ups[0]->size_;
    std::vector<float> m((size_t) rows * cols, 0.0f); int r2 = 0, c2 = 0;
    ok(dsr_fmat_load(fileName, old, rows, cols, m.data(), &r2, &c2));
    if (r2 < rows) throw Error(DSR_E_DIMENSION, "Cannot resize from %d to %d", r2, rows);           // the crop back to (size x srcSize)
    if (c2 < cols) throw Error(DSR_E_DIMENSION, "Cannot resize from %d to %d", c2, cols);
    q->hA = m; q->A.upload(q->hA); q->ready = false;
  });
}
// StorageFeature::write(fileName, plainText) / read(fileName) (feature.cc:3025-3067), quirks kept: the count that is written is _frameX -- the
// index of the last frame, one less than the number of frames that follow it; read() takes that number for _frameX and reads that many frames,
// i.e. one fewer than the file holds.  Binary: big-endian ints (write_int) and native-endian float blocks (gsl_vector_float_fwrite).
dsr_status dsr_storage_write(dsr_stream* s, const char* fileName, int plainText)
{
  return guard([&] {
    StorageOp* q = dynamic_cast<StorageOp*>(s); if (!q || !fileName) throw Error(DSR_E_PARAMETER, "not a StorageFeature");
    if (q->frameX <= 0) throw Error(DSR_E_IO, "Frame count must be > 0.\n");
    FILE* fp = fopen(fileName, "w"); if (!fp) throw Error(DSR_E_IO, "Could not open file %s", fileName);
    const int sz = q->size_;
    auto wbe = [&](int v) { const unsigned u = (unsigned) v; const unsigned char b[4] = { (unsigned char) (u >> 24), (unsigned char) (u >> 16), (unsigned char) (u >> 8), (unsigned char) u }; fwrite(b, 1, 4, fp); };
    if (plainText) {
      fprintf(fp, "%d %d\n", q->frameX, sz);
      for (int i = 0; i <= q->frameX; i++) { const float* r = (const float*) q->row(i); for (int j = 0; j < sz; j++) { fprintf(fp, "%g", (double) r[j]); if (j < sz - 1) fprintf(fp, " "); } fprintf(fp, "\n"); }
    } else {
      wbe(q->frameX); wbe(sz);
      for (int i = 0; i <= q->frameX; i++) fwrite(q->row(i), sizeof(float), (size_t) sz, fp);
    }
    fclose(fp);
  });
}
dsr_status dsr_storage_read(dsr_stream* s, const char* fileName)
{
  return guard([&] {
    StorageOp* q = dynamic_cast<StorageOp*>(s); if (!q || !fileName) throw Error(DSR_E_PARAMETER, "not a StorageFeature");
    FILE* fp = fopen(fileName, "r"); if (!fp) throw Error(DSR_E_IO, "Could not open file %s", fileName);
    auto rbe = [&](int& v) { unsigned char b[4]; if (fread(b, 1, 4, fp) != 4) { fclose(fp); throw Error(DSR_E_IO, "premature end of %s", fileName); } v = (int) ((unsigned) b[0] << 24 | (unsigned) b[1] << 16 | (unsigned) b[2] << 8 | (unsigned) b[3]); };
    int fx = 0, sz = 0; rbe(fx); rbe(sz);
    if (sz != q->size_) { fclose(fp); throw Error(DSR_E_DIMENSION, "Feature dimensions (%d vs. %d) do not match.\n", sz, q->size_); }
    if (fx < 0 || fx >= 100000) { fclose(fp); throw Error(DSR_E_DIMENSION, "Frame %d is greater than maximum number %d.", fx, 100000); }
    // the operator now serves frames 0.._frameX from its own store: frames 0.._frameX-1 from the file, frame _frameX as the store had it (zero)
    q->nFrames = fx + 1; q->host.assign((size_t) q->nFrames * q->rowBytes() + 16, 0);
    for (int i = 0; i < fx; i++) if (fread(q->host.data() + (size_t) i * q->rowBytes(), sizeof(float), (size_t) sz, fp) != (size_t) sz) { fclose(fp); throw Error(DSR_E_IO, "premature end of %s", fileName); }
    fclose(fp);
    require_device(); q->dev.reserve(q->host.size()); DSR_HIP(hipMemcpy(q->dev.p, q->host.data(), (size_t) q->nFrames * q->rowBytes(), hipMemcpyHostToDevice));
    q->ready = true; q->frameX = fx; q->endOfSamples = false;
  });
}

// ---------------------------------------------------------------------------------------------------------------------------------
// Speech activity detection over streams (include/dsr.h section 7b).  A metric is no stream (next() returns a number), but it follows the
// streams' convention: the sources' whole utterance is evaluated by one batch call at the first next() after a reset(), from a working copy
// of the carried state; commit(n) then advances the carried state itself by the n frames that were really served.
struct dsr_vad_metric {
  enum { ENERGY = 0, SIMPLE = 1, POWER = 2, CCC = 5, GG = 6 };         // POWER + kind of dsr_sad_power_run, GG + kind of dsr_sad_gg_run; ups of GG: (X1, env1[, X2, env2])
  int refs = 1, kind = ENERGY; std::string name; std::vector<dsr_stream*> ups;
  double initialEnergy = 5.0e+07, threshold = 0.5, gamma = 0.98, E0 = 1.0, twiddle = -1.0, beta = 0.95; dsr_sad_gg* gg = nullptr; DevBuf<double> rho, wRho; unsigned headN = 4, tailN = 10, energiesN = 200, fftLen = 0, lowX = 0, highX = 0, nCand = 1;
  DevBuf<double> hist, wHist, E, wE, dDec, dScore, dPow; DevBuf<int> cnt, wCnt; DevBuf<unsigned char> pack; bool stateReady = false;
  bool ready = false; int T = 0, cur = -1; std::vector<double> dec, score, powers; double curScore = 0.0;
  ~dsr_vad_metric() { for (size_t i = 0; i < ups.size(); i++) dsr_stream_release(ups[i]); if (gg) dsr_sad_gg_destroy(gg); }
  bool stateful() const { return kind == ENERGY || kind == SIMPLE || kind == GG + 1; }
  size_t rhoN() const { return (size_t) 2 * (fftLen / 2 + 1); }
  void need_state() {
    if (stateReady) return;
    require_device();
    if (kind == ENERGY) { hist.reserve(energiesN); wHist.reserve(energiesN); cnt.reserve(4); wCnt.reserve(4); ok(dsr_sad_energy_state_init(hist.p, cnt.p, 1, (int) energiesN, initialEnergy, 0, S0)); }
    if (kind == SIMPLE) { const double z = 0.0; E.upload(&z, 1, S0); wE.reserve(1); }
    if (kind == GG + 1) { const std::vector<double> z(rhoN(), 0.0); rho.upload(z, S0); wRho.reserve(rhoN()); }
    stateReady = true;
  }
  void run(int n, bool work) {                                         // the first n frames, on the working copy of the state or on the state itself
    dDec.reserve(n > 0 ? n : 1); dScore.reserve(n > 0 ? n : 1);
    if (kind == ENERGY) {
      if (work) { DSR_HIP(hipMemcpyAsync(wHist.p, hist.p, energiesN * sizeof(double), hipMemcpyDeviceToDevice, S0)); DSR_HIP(hipMemcpyAsync(wCnt.p, cnt.p, 4 * sizeof(int), hipMemcpyDeviceToDevice, S0)); }
      ok(dsr_sad_energy_run(ups[0]->d<float>(), nullptr, 1, n, ups[0]->size_, threshold, headN, tailN, (int) energiesN, work ? wHist.p : hist.p, work ? wCnt.p : cnt.p, dDec.p,
                            dScore.p, nullptr, S0));
    } else if (kind == SIMPLE) {
      if (work) DSR_HIP(hipMemcpyAsync(wE.p, E.p, sizeof(double), hipMemcpyDeviceToDevice, S0));
      ok(dsr_sad_simple_energy_run(ups[0]->d<double2>(), nullptr, 1, n, (int) fftLen, threshold, gamma, work ? wE.p : E.p, dDec.p, dScore.p, S0));
    } else if (kind >= GG) {
      const bool two = kind > GG;
      if (work && kind == GG + 1) DSR_HIP(hipMemcpyAsync(wRho.p, rho.p, rhoN() * sizeof(double), hipMemcpyDeviceToDevice, S0));
      ok(dsr_sad_gg_run(gg, kind - GG, ups[0]->dev.p, two ? ups[2]->dev.p : nullptr, ups[1]->d<float>(), two ? ups[3]->d<float>() : nullptr, ups[1]->size_, nullptr, 1, n,
                        twiddle, threshold, beta, kind == GG + 1 ? (work ? wRho.p : rho.p) : nullptr, dDec.p, dScore.p, nullptr, S0));
    } else {
      const int C = (int) ups.size(); const size_t rb = ups[0]->rowBytes();
      pack.reserve((size_t) C * (n > 0 ? n : 1) * rb);
      for (int c = 0; c < C && n > 0; c++) DSR_HIP(hipMemcpyAsync(pack.p + (size_t) c * n * rb, ups[c]->dev.p, (size_t) n * rb, hipMemcpyDeviceToDevice, S0));
      if (kind == CCC) ok(dsr_sad_ccc_run(pack.p, 1, nullptr, 1, C, n, fftLen, lowX, highX, nCand, threshold, dDec.p, dScore.p, nullptr, S0));
      else { dPow.reserve((size_t) C * (n > 0 ? n : 1)); ok(dsr_sad_power_run((const float*) pack.p, nullptr, 1, C, n, fftLen, lowX, highX, kind - POWER, E0, dDec.p, dPow.p, dScore.p, S0)); }
    }
  }
  void materialize() {
    if (ready) return;
    if (ups.empty()) throw Error(DSR_E_CONSISTENCY, "%s has no channel.", name.c_str());
    if (kind == CCC && ups.size() < 2) throw Error(DSR_E_DIMENSION, "%s needs at least 2 channels, got %zu.", name.c_str(), ups.size());
    need_state();
    for (size_t i = 0; i < ups.size(); i++) ups[i]->materialize();
    T = ups[0]->nFrames; for (size_t i = 1; i < ups.size(); i++) T = std::min(T, ups[i]->nFrames);
    run(T, true);
    dec.assign(T, 0.0); score.assign(T, 0.0);
    if (T > 0) { DSR_HIP(hipMemcpy(dec.data(), dDec.p, T * sizeof(double), hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(score.data(), dScore.p, T * sizeof(double), hipMemcpyDeviceToHost)); }
    if (kind >= POWER && kind < CCC) { powers.assign((size_t) T * ups.size(), 0.0); if (T > 0) DSR_HIP(hipMemcpy(powers.data(), dPow.p, powers.size() * sizeof(double), hipMemcpyDeviceToHost)); }
    ready = true; cur = -1;
  }
  void commit(int n) {                                                 // the carried state after the first n frames of the materialised utterance
    if (ready && stateful() && n > 0) { run(std::min(n, T), false); DSR_HIP(hipStreamSynchronize(S0)); }
    ready = false; cur = -1;
  }
  double next(int fx) {
    materialize();
    const int idx = fx < 0 ? cur + 1 : fx;
    if (idx >= T) throw Error(DSR_E_ITERATOR, "end of samples!");
    cur = idx; curScore = score[idx];
    return dec[idx];
  }
  void reset() {
    commit(cur + 1);
    if (kind == ENERGY && stateReady) ok(dsr_sad_energy_state_init(hist.p, cnt.p, 1, (int) energiesN, initialEnergy, 1, S0));   // sad.cc:459-463
    for (size_t i = 0; i < ups.size(); i++) ups[i]->reset();
  }
  void next_speaker() {
    ready = false; cur = -1; stateReady = false; need_state();         // sad.cc:465-472, 168-171
    for (size_t i = 0; i < ups.size(); i++) ups[i]->reset();
  }
};

namespace {
struct HangoverOp : dsr_stream {     // HangoverVADFeature, HangoverMIVADFeature, HangoverMultiStageVADFeature (sad.cc:1705-1945); ups[0] = the source
  int kind = 0; unsigned headN = 4, tailN = 10; std::vector<dsr_vad_metric*> metrics; std::vector<double> thr;
  int start = 0, length = 0, consumed = 0; std::vector<int> codes; DevBuf<double> dDec; DevBuf<int> dOut, dCodes;
  ~HangoverOp() override { for (size_t i = 0; i < metrics.size(); i++) dsr_sad_metric_release(metrics[i]); }
  void reset() override { for (size_t i = 0; i < metrics.size(); i++) metrics[i]->reset(); dsr_stream::reset(); }
  void compute() override {
    int T = ups[0]->nFrames; const int K = (int) metrics.size();
    for (int k = 0; k < K; k++) { metrics[k]->materialize(); T = std::min(T, metrics[k]->T); }
    start = -(int) headN; length = consumed = 0; codes.assign(T, 0);
    if (T <= 0) { alloc(0); return; }
    dDec.reserve((size_t) K * T); dOut.reserve(3); dCodes.reserve(T);
    for (int k = 0; k < K; k++) DSR_HIP(hipMemcpyAsync(dDec.p + (size_t) k * T, metrics[k]->dDec.p, T * sizeof(double), hipMemcpyDeviceToDevice, S0));
    ok(dsr_sad_hangover_run(dDec.p, nullptr, K, 1, T, thr.data(), headN, tailN, kind, dOut.p, dOut.p + 1, dOut.p + 2, dCodes.p, S0));
    dev.reserve((size_t) T * rowBytes());
    ok(dsr_sad_gather_run(ups[0]->d<float>(), dOut.p, dOut.p + 1, 1, T, size_, d<float>(), S0));
    int o[3]; DSR_HIP(hipMemcpy(o, dOut.p, sizeof o, hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(codes.data(), dCodes.p, T * sizeof(int), hipMemcpyDeviceToHost));
    start = o[0]; length = o[1]; consumed = o[2]; nFrames = length;
    for (int k = 0; k < K; k++) metrics[k]->commit(consumed);          // the reference never evaluates a metric past the segment's end
  }
  int decision_metric() const {
    if (!ready || consumed < 1 || (frameX < 0 && !endOfSamples)) return 0;
    if (endOfSamples || length == 0) return codes[consumed - 1];
    return frameX < (int) headN ? codes[start + (int) headN - 1] : codes[start + frameX];
  }
};
struct ShapeOp : dsr_stream {        // the spectral-shape operators of sadFeature.cc
  int op = 0; float sampleRate = 16000.0f, thresh = 0.0f;
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_sad_shape_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, op, sampleRate, thresh, d<float>(), S0)); }
};
dsr_vad_metric* mk_metric(int kind, const char* name, const char* dflt) { dsr_vad_metric* m = new dsr_vad_metric(); m->kind = kind; m->name = (name && *name) ? name : dflt; return m; }
dsr_vad_metric* metric(dsr_vad_metric* m) { if (!m) throw Error(DSR_E_PARAMETER, "null metric"); return m; }
}  // namespace

dsr_status dsr_sad_energy_metric_create(dsr_stream* source, double initialEnergy, double threshold, unsigned headN, unsigned tailN, unsigned energiesN, const char* name,
                                        dsr_vad_metric** out)
{
  return guard([&] {
    need(source, DSR_T_FLOAT, "EnergyVADMetric"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (energiesN < 1 || energiesN > 8192) throw Error(DSR_E_DIMENSION, "energiesN = %u is outside [1, 8192].", energiesN);
    if (!(threshold >= 0.0 && threshold < 1.0)) throw Error(DSR_E_DIMENSION, "Threshold %g is outside [0, 1).", threshold);
    dsr_vad_metric* m = mk_metric(dsr_vad_metric::ENERGY, name, "Energy VAD Metric");
    m->initialEnergy = initialEnergy; m->threshold = threshold; m->headN = headN; m->tailN = tailN; m->energiesN = energiesN;
    dsr_stream_retain(source); m->ups.push_back(source); *out = m;
  });
}
dsr_status dsr_sad_power_metric_create(int kind, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const char* name, dsr_vad_metric** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    unsigned lo, hi, bn; ok(dsr_sad_band(fftLen, sampleRate, lowCutoff, highCutoff, &lo, &hi, &bn));
    dsr_vad_metric* m = mk_metric(dsr_vad_metric::POWER + kind, name, kind == 0 ? "Power Spectrum VAD Metric" : kind == 1 ? "NormalizedEnergyMetric" : "TSPS VAD Metric");
    m->fftLen = fftLen; m->lowX = lo; m->highX = hi; m->E0 = kind == 2 ? 5000 : 1.0; *out = m;                     // sad.cc:639, 733, 966
  });
}
dsr_status dsr_sad_ccc_metric_create(unsigned fftLen, unsigned nCand, double sampleRate, double lowCutoff, double highCutoff, const char* name, dsr_vad_metric** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftLen < 4 || fftLen > 2048 || (fftLen & (fftLen - 1))) throw Error(DSR_E_DIMENSION, "fftLen = %u is no power of two in [4, 2048].", fftLen);
    if (nCand < 1 || nCand > 64) throw Error(DSR_E_DIMENSION, "nCand = %u is outside [1, 64].", nCand);
    unsigned lo, hi, bn; ok(dsr_sad_band(fftLen, sampleRate, lowCutoff, highCutoff, &lo, &hi, &bn));
    dsr_vad_metric* m = mk_metric(dsr_vad_metric::CCC, name, "CCC VAD Metric");
    m->fftLen = fftLen; m->lowX = lo; m->highX = hi; m->nCand = nCand; m->threshold = 0.1; *out = m;               // sad.cc:822
  });
}
dsr_status dsr_sad_simple_energy_create(dsr_stream* samp, double threshold, double gamma, dsr_vad_metric** out)
{
  return guard([&] {
    need(samp, DSR_T_COMPLEX, "SimpleEnergyVAD"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    dsr_vad_metric* m = mk_metric(dsr_vad_metric::SIMPLE, nullptr, "Simple Energy VAD");
    m->threshold = threshold; m->gamma = gamma; m->fftLen = (unsigned) samp->size_; dsr_stream_retain(samp); m->ups.push_back(samp); *out = m;
  });
}
dsr_status dsr_sad_gg_metric_create(int kind, dsr_stream* source1, dsr_stream* source2, dsr_stream* est1, dsr_stream* est2, const char* shapeFactorDir, double twiddle,
                                    double threshold, double beta, double sampleRate, double lowCutoff, double highCutoff, const char* name, dsr_vad_metric** out)
{
  return guard([&] {
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    static const char* names[3] = { "Negentropy VAD Metric", "Mutual Information VAD Metric", "Likelihood Ratio VAD Metric" };
    need(source1, DSR_T_COMPLEX, names[kind]); need(est1, DSR_T_FLOAT, names[kind]); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind > 0) { need(source2, DSR_T_COMPLEX, names[kind]); need(est2, DSR_T_FLOAT, names[kind]); }
    const unsigned fftLen = (unsigned) source1->size_; const int F = (int) (fftLen / 2 + 1);
    if (kind > 0 && source2->size_ != source1->size_) throw Error(DSR_E_DIMENSION, "The two sources have %d and %d elements.", source1->size_, source2->size_);
    if (est1->size_ < F || (kind > 0 && est2->size_ != est1->size_))
      throw Error(DSR_E_DIMENSION, "Numbers of spectral bins and envelope elements do not match (%d vs. %d)", F, est1->size_);
    std::vector<double> sf; const bool fromDir = shapeFactorDir && *shapeFactorDir;
    if (fromDir) { sf.resize(F); ok(dsr_sad_gg_read_shape_factors(shapeFactorDir, fftLen, sf.data())); }
    std::unique_ptr<dsr_vad_metric> m(mk_metric(dsr_vad_metric::GG + kind, name, names[kind]));
    ok(dsr_sad_gg_create(fromDir ? sf.data() : nullptr, fftLen, sampleRate, lowCutoff, highCutoff, kind == 1, &m->gg));
    m->fftLen = fftLen; m->twiddle = twiddle; m->threshold = threshold; m->beta = beta;
    dsr_stream* u[4] = { source1, est1, source2, est2 };
    for (int i = 0; i < (kind > 0 ? 4 : 2); i++) { dsr_stream_retain(u[i]); m->ups.push_back(u[i]); }
    *out = m.release();
  });
}
void dsr_sad_metric_release(dsr_vad_metric* m) { if (m && --m->refs == 0) delete m; }
dsr_status dsr_sad_metric_set_channel(dsr_vad_metric* m, dsr_stream* chan)
{
  return guard([&] {
    metric(m);
    if (m->kind < dsr_vad_metric::POWER || m->kind >= dsr_vad_metric::GG) throw Error(DSR_E_PARAMETER, "%s takes no channels.", m->name.c_str());
    const bool ccc = m->kind == dsr_vad_metric::CCC;
    need(chan, ccc ? DSR_T_COMPLEX : DSR_T_FLOAT, m->name.c_str());
    const int want = ccc ? (int) m->fftLen : (int) (m->fftLen / 2 + 1);
    if (chan->size_ != want) throw Error(DSR_E_DIMENSION, "%s: a channel of %d elements where fftLen = %u needs %d.", m->name.c_str(), chan->size_, m->fftLen, want);
    dsr_stream_retain(chan); m->ups.push_back(chan); m->ready = false;
  });
}
dsr_status dsr_sad_metric_clear_channel(dsr_vad_metric* m)
{ return guard([&] { metric(m); if (m->kind < dsr_vad_metric::POWER || m->kind >= dsr_vad_metric::GG) return; for (size_t i = 0; i < m->ups.size(); i++) dsr_stream_release(m->ups[i]); m->ups.clear(); m->ready = false; }); }
dsr_status dsr_sad_metric_set_e0(dsr_vad_metric* m, double E0) { return guard([&] { metric(m)->E0 = E0; m->ready = false; }); }
dsr_status dsr_sad_metric_set_ncand(dsr_vad_metric* m, unsigned nCand)
{ return guard([&] { metric(m); if (nCand < 1 || nCand > 64) throw Error(DSR_E_DIMENSION, "nCand = %u is outside [1, 64].", nCand); m->nCand = nCand; m->ready = false; }); }
dsr_status dsr_sad_metric_set_threshold(dsr_vad_metric* m, double threshold) { return guard([&] { metric(m)->threshold = threshold; m->ready = false; }); }
dsr_status dsr_sad_metric_next(dsr_vad_metric* m, int frameX, double* value)
{ return guard([&] { metric(m); if (!value) throw Error(DSR_E_PARAMETER, "null argument"); *value = m->next(frameX); }); }
dsr_status dsr_sad_metric_reset(dsr_vad_metric* m) { return guard([&] { metric(m)->reset(); }); }
dsr_status dsr_sad_metric_next_speaker(dsr_vad_metric* m) { return guard([&] { metric(m)->next_speaker(); }); }
dsr_status dsr_sad_metric_score(dsr_vad_metric* m, double* score) { return guard([&] { metric(m); if (!score) throw Error(DSR_E_PARAMETER, "null argument"); *score = m->curScore; }); }
dsr_status dsr_sad_metric_powers(dsr_vad_metric* m, double* powers, int n)
{
  return guard([&] {
    metric(m); if (!powers) throw Error(DSR_E_PARAMETER, "null argument");
    if (m->kind < dsr_vad_metric::POWER || m->kind >= dsr_vad_metric::CCC) throw Error(DSR_E_PARAMETER, "%s keeps no channel powers.", m->name.c_str());
    if (!m->ready || m->cur < 0 || n != (int) m->ups.size()) throw Error(DSR_E_CONSISTENCY, "no frame of %d channels has been served.", n);
    memcpy(powers, m->powers.data() + (size_t) m->cur * n, n * sizeof(double));
  });
}
dsr_status dsr_sad_metric_energy_percentile(dsr_vad_metric* m, double percentile, double* value)
{
  return guard([&] {
    metric(m); if (m->kind != dsr_vad_metric::ENERGY) throw Error(DSR_E_PARAMETER, "%s keeps no energies.", m->name.c_str());
    m->need_state();
    const bool live = m->ready && m->cur >= 0;                          // frames served since the last commit: the history as it is after them
    if (live) { m->run(m->cur + 1, true); }
    std::vector<double> h(m->energiesN);
    DSR_HIP(hipStreamSynchronize(S0)); DSR_HIP(hipMemcpy(h.data(), live ? m->wHist.p : m->hist.p, h.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (live) { m->run(m->T, true); }                                   // dDec / dScore again hold the whole utterance
    ok(dsr_sad_energy_percentile(h.data(), (int) m->energiesN, percentile, value));
  });
}
dsr_status dsr_sad_shape_create(dsr_stream* src, int op, float sampleRate, float thresh, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "a spectral-shape feature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (op < 0 || op > 3) throw Error(DSR_E_PARAMETER, "operator %d", op);
    int tx = 0; if (op == 1) ok(dsr_sad_band_ratio_index(src->size_, sampleRate, thresh, &tx));
    static const char* names[4] = { "Energy Diffusion", "Band Energy Ratio", "Negative Entropy", "Significant Subbands" };
    ShapeOp* s = mk<ShapeOp>(name, names[op], 1, DSR_T_FLOAT); s->op = op; s->sampleRate = sampleRate; s->thresh = thresh; s->add_up(src); *out = s;
  });
}
dsr_status dsr_sad_hangover_create(dsr_stream* source, dsr_vad_metric* met, double threshold, unsigned headN, unsigned tailN, int kind, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(source, DSR_T_FLOAT, "HangoverVADFeature"); metric(met); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    if (headN < 1) throw Error(DSR_E_DIMENSION, "headN = 0: the ring of buffered frames would be empty.");
    HangoverOp* s = mk<HangoverOp>(name, kind == 0 ? "Hangover VAD Feature" : kind == 1 ? "Hangover MIVAD Feature" : "HangoverMultiStageVADFeature", source->size_, DSR_T_FLOAT);
    s->kind = kind; s->headN = headN; s->tailN = tailN; s->add_up(source); met->refs++; s->metrics.push_back(met); s->thr.push_back(threshold); *out = s;
  });
}
dsr_status dsr_sad_hangover_add_metric(dsr_stream* h, dsr_vad_metric* met, double threshold)
{
  return guard([&] {
    HangoverOp* s = as_op<HangoverOp>(h, "hangover"); metric(met);
    if (s->kind == 0) throw Error(DSR_E_PARAMETER, "HangoverVADFeature takes one metric.");
    if (s->metrics.size() >= (s->kind == 1 ? 3u : 8u)) throw Error(DSR_E_DIMENSION, "%s has all its metrics.", s->name.c_str());
    if (s->kind == 2 && s->metrics.size() >= 2 && met->stateful())      // sad.cc:1932-1935 calls it twice in a frame where its stage fires
      throw Error(DSR_E_CONSISTENCY, "%s: the stateful %s at stage %zu would be advanced twice a frame.", s->name.c_str(), met->name.c_str(), s->metrics.size());
    met->refs++; s->metrics.push_back(met); s->thr.push_back(threshold); s->ready = false;
  });
}
dsr_status dsr_sad_hangover_next_speaker(dsr_stream* h)
{ return guard([&] { HangoverOp* s = as_op<HangoverOp>(h, "hangover"); s->dsr_stream::reset(); for (size_t i = 0; i < s->metrics.size(); i++) s->metrics[i]->next_speaker(); }); }
dsr_status dsr_sad_hangover_prefix_n(dsr_stream* h, int* prefixN)
{ return guard([&] { HangoverOp* s = as_op<HangoverOp>(h, "hangover"); if (!prefixN) throw Error(DSR_E_PARAMETER, "null argument"); *prefixN = s->ready ? s->start : -(int) s->headN; }); }
dsr_status dsr_sad_hangover_decision_metric(dsr_stream* h, int* dm)
{ return guard([&] { HangoverOp* s = as_op<HangoverOp>(h, "hangover"); if (!dm) throw Error(DSR_E_PARAMETER, "null argument"); *dm = s->decision_metric(); }); }

// ---------------------------------------------------------------------------------------------------------------------------------
// FeatureSpaceAdaptationFeature as a stream operator (asr/train/fsa.cc:247-280): every frame of the source under transform 0 of the adaptation
// handle, which exists from distribSet() on.  The frames stay on the device, so a distribution set built on this stream decodes adapted
// features without a host round trip.  A changed transform or shift shows after the next reset(), as every operator here recomputes then.
namespace {
struct FsaOp : dsr_stream {
  int maxAccu = 1, maxTran = 1; dsr_fsa* h = nullptr;
  ~FsaOp() override { dsr_fsa_destroy(h); }
  void compute() override {
    if (!h) throw Error(DSR_E_CONSISTENCY, "Must initialize the distribution set before using.");       // fsa.cc:251-252
    alloc(ups[0]->nFrames);
    ok(dsr_fsa_apply(h, ups[0]->d<float>(), nFrames, nullptr, dsr_fsa_shift(h), d<float>(), S0));
  }
  const void* next(int fx) override {
    if (fx == frameX && frameX >= 0) return row(frameX);                                                // fsa.cc:249
    if (!h) throw Error(DSR_E_CONSISTENCY, "Must initialize the distribution set before using.");
    return dsr_stream::next(fx);
  }
};
}  // namespace

dsr_status dsr_fsa_feature_create(dsr_stream* src, int maxAccu, int maxTran, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "FeatureSpaceAdaptationFeature");
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (maxAccu < 1 || maxTran < 1) throw Error(DSR_E_PARAMETER, "%d accumulators, %d transformations", maxAccu, maxTran);
    FsaOp* s = mk<FsaOp>(name, "FeatureSpaceAdaptationFeature", src->size_, DSR_T_FLOAT); s->maxAccu = maxAccu; s->maxTran = maxTran; s->add_up(src); *out = s;
  });
}
dsr_status dsr_fsa_feature_distrib_set(dsr_stream* s, dsr_gmm* gmm)
{
  return guard([&] {
    FsaOp* q = as_op<FsaOp>(s, "FeatureSpaceAdaptationFeature"); if (!gmm) throw Error(DSR_E_PARAMETER, "null argument");
    if (q->size_ != dsr_gmm_dim(gmm)) throw Error(DSR_E_DIMENSION, "Feature and codebook dimensions (%d vs. %d) do not match.", q->size_, dsr_gmm_dim(gmm));
    dsr_fsa* h = nullptr; ok(dsr_fsa_create(gmm, q->maxAccu, q->maxTran, &h));
    dsr_fsa_destroy(q->h); q->h = h; q->ready = false;
  });
}
dsr_fsa* dsr_fsa_feature_handle(dsr_stream* s) { FsaOp* q = dynamic_cast<FsaOp*>(s); return q ? q->h : nullptr; }

// ---------------------------------------------------------------------------------------------------------------------------------
// ASR side of the boundary: the distribution set as the decoder sees it.  The reference decoder asks _dist->find(distX-1)->score(_frameX)
// (asr/decoder/decoder.h:985); Distrib::score -> CodebookBasic::score pulls frame frameX of the feature stream and caches the codebook's
// score for that frame (asr/gaussian/distribBasic.h:48-50,110-114, codebookBasic.cc:431-465).  Here a distribution set is a GMM model bound to
// a feature stream handle: score(distX, frameX) scores ALL distributions of that frame on the device at the first request and serves the rest
// of the frame's requests from the host copy; decode_stream() keeps everything on the device (features -> scores -> token passing), no host
// round trip.
struct dsr_distribset { dsr_gmm* gmm = nullptr; dsr_stream* feat = nullptr; int mode = 0; int cachedFrame = -1; std::vector<float> row; DevBuf<float> d_row, d_scores; DevBuf<int> d_T; };

dsr_status dsr_distribset_create(dsr_gmm* gmm, dsr_stream* feature, int gmmMode, dsr_distribset** out)
{
  return guard([&] {
    if (!gmm || !feature || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (feature->type != DSR_T_FLOAT) throw Error(DSR_E_TYPE, "the feature stream of a codebook set delivers float vectors");
    if (feature->size_ != dsr_gmm_dim(gmm)) throw Error(DSR_E_DIMENSION, "Feature and codebook dimensions (%d vs. %d) do not match.", feature->size_, dsr_gmm_dim(gmm));
    if (gmmMode < 0 || gmmMode > 2) throw Error(DSR_E_PARAMETER, "bad scoring mode %d", gmmMode);
    dsr_distribset* d = new dsr_distribset(); d->gmm = gmm; d->feat = feature; d->mode = gmmMode; dsr_stream_retain(feature); *out = d;
  });
}
void dsr_distribset_destroy(dsr_distribset* d) { if (d) { dsr_stream_release(d->feat); delete d; } }
int dsr_distribset_ndists(const dsr_distribset* d) { return d ? dsr_gmm_num_dists(d->gmm) : 0; }
dsr_status dsr_distribset_find(const dsr_distribset* d, const char* name, int* distX)
{ if (!d) return guard([&] { throw Error(DSR_E_PARAMETER, "null argument"); }); return dsr_gmm_find_dist(d->gmm, name, distX); }
const char* dsr_distribset_name(const dsr_distribset* d, int distX) { return d ? dsr_gmm_dist_name(d->gmm, distX) : ""; }
dsr_status dsr_distribset_reset_cache(dsr_distribset* d) { return guard([&] { if (!d) throw Error(DSR_E_PARAMETER, "null argument"); d->cachedFrame = -1; }); }      // codebookBasic.cc:414-420
dsr_status dsr_distribset_reset_feature(dsr_distribset* d) { return guard([&] { if (!d) throw Error(DSR_E_PARAMETER, "null argument"); d->feat->reset(); d->cachedFrame = -1; }); }
dsr_status dsr_distribset_score(dsr_distribset* d, int distX, int frameX, float* score)
{
  return guard([&] {
    if (!d || !score) throw Error(DSR_E_PARAMETER, "null argument");
    const int K = dsr_gmm_num_dists(d->gmm);
    if (distX < 0 || distX >= K) throw Error(DSR_E_INDEX, "distribution %d of %d", distX, K);
    if (frameX != d->cachedFrame || frameX < 0) {
      (void) d->feat->next(frameX);                                       // jiterator_error at the end of the stream, jindex_error out of order
      const int t = d->feat->frameX;
      d->d_row.reserve((size_t) K); d->row.resize((size_t) K);
      const float* x = reinterpret_cast<const float*>(d->feat->dev.p) + (size_t) t * d->feat->size_;
      ok(dsr_gmm_score(d->gmm, x, 1, d->mode, d->d_row.p, nullptr, S0));
      DSR_HIP(hipMemcpy(d->row.data(), d->d_row.p, sizeof(float) * (size_t) K, hipMemcpyDeviceToHost));
      d->cachedFrame = t;
    }
    *score = d->row[(size_t) distX];
  });
}
// _Decoder::decode() (decoder.h:688-737) for the utterance the feature stream currently holds: _newUtterance resets the cache and the feature
// (decoder.h:488-492), every frame is scored and decoded on the device.  An empty stream is DSR_E_ITERATOR (the exception escapes decode(), :691).
dsr_status dsr_decoder_decode_stream(dsr_decoder* dec, dsr_distribset* d, dsr_decode_result* res, int32_t* arcs_out, uint32_t* words_out, int maxPath)
{
  return guard([&] {
    if (!dec || !d || !res) throw Error(DSR_E_PARAMETER, "null argument");
    d->cachedFrame = -1; d->feat->reset();
    d->feat->materialize();
    const int T = d->feat->nFrames, K = dsr_gmm_num_dists(d->gmm);
    if (T <= 0) { d->feat->endOfSamples = true; throw Error(DSR_E_ITERATOR, "end of samples!"); }
    d->d_scores.reserve((size_t) T * K); d->d_T.upload(&T, 1);
    ok(dsr_gmm_score(d->gmm, reinterpret_cast<const float*>(d->feat->dev.p), (int64_t) T, d->mode, d->d_scores.p, nullptr, S0));
    ok(dsr_decoder_decode_batch(dec, d->d_scores.p, d->d_T.p, 1, T, K, res, arcs_out, words_out, maxPath, S0));
    d->feat->frameX = T - 1; d->feat->endOfSamples = true;                   // the reference has pulled the stream to its end
    if (res->status != DSR_OK) throw Error(res->status, "decode failed (status %d)", res->status);
  });
}

// Lattice::gammaProbsDist(dss, acScale, lmScale, lmPenalty, silPenalty, silSymbol) (asr/lattice/lattice.cc:331-341): the links' acoustic scores are
// recomputed from the distribution set (_updateAc, :381-409: links of the initial node and of the nodes in _nodes -- not of the final nodes -- with
// an input symbol; score = sum over the link's frames), then gammaProbs.  The frames are scored once on the device, the per-link sums are a gather
// kernel over the score matrix.  A sum above LogZero is the reference's consistency error.
dsr_status dsr_lattice_gamma_probs_dist(dsr_lattice* L, dsr_distribset* d, double acScale, double lmScale, double lmPenalty, double silPenalty, unsigned silenceX,
                                        double* logProb)
{
  return guard([&] {
    if (!L || !d) throw Error(DSR_E_PARAMETER, "null argument");
    d->cachedFrame = -1;                                                     // dss->resetCache()
    L->ensure_ops(); L->sorted.clear();                                      // _clearSorted()
    d->feat->materialize();
    const int T = d->feat->nFrames, K = dsr_gmm_num_dists(d->gmm);
    std::vector<int> link, dist, start, end;
    auto take = [&](int node) {
      for (size_t k = 0; k < L->adj[(size_t) node].size(); k++) {
        const int e = L->adj[(size_t) node][k];
        if (L->in[(size_t) e] == 0) continue;
        const long dx = (long) L->in[(size_t) e] - 1;
        if (dx >= K) throw Error(DSR_E_INDEX, "link %d names distribution %ld of %d", e, dx, K);
        if (L->start[(size_t) e] <= L->end[(size_t) e] && (L->start[(size_t) e] < 0 || L->end[(size_t) e] >= T))
          throw Error(DSR_E_INDEX, "link %d spans frames %d..%d of %d", e, L->start[(size_t) e], L->end[(size_t) e], T);
        link.push_back(e); dist.push_back((int) dx); start.push_back(L->start[(size_t) e]); end.push_back(L->end[(size_t) e]);
      }
    };
    take(0);
    for (size_t p = 0; p < L->slots.size(); p++) if (L->slots[p] >= 0) take(L->slots[p]);
    if (!link.empty()) {
      if (T <= 0) throw Error(DSR_E_ITERATOR, "end of samples!");
      d->d_scores.reserve((size_t) T * K);
      ok(dsr_gmm_score(d->gmm, reinterpret_cast<const float*>(d->feat->dev.p), (int64_t) T, d->mode, d->d_scores.p, nullptr, S0));
      DevBuf<int> dd, ds, de; DevBuf<double> dout; dd.upload(dist); ds.upload(start); de.upload(end); dout.reserve(link.size());
      op_link_ac(d->d_scores.p, K, dd.p, ds.p, de.p, (int) link.size(), dout.p, S0);
      DSR_HIP(hipGetLastError());
      std::vector<double> sums(link.size());
      DSR_HIP(hipMemcpy(sums.data(), dout.p, sizeof(double) * link.size(), hipMemcpyDeviceToHost));
      for (size_t i = 0; i < link.size(); i++) {
        if (sums[i] > 1.0E10) throw Error(DSR_E_CONSISTENCY, "Log-prob (%g) > LogZero (%g)", sums[i], 1.0E10);
        L->ac[(size_t) link[i]] = sums[i];
      }
    }
    const double p = L->gamma_probs(acScale, lmScale, lmPenalty, silPenalty, silenceX);
    if (logProb) *logProb = p;
  });
}

}  // extern "C"
