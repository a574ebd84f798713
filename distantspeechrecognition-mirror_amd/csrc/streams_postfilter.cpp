// csrc/streams_postfilter.cpp -- the operators of btk/postfilter as streams: Zelinski / McCowan / Lefkimmiatis, the high-pass filter, spectral
// subtraction, the Wiener filter, the binary masks and their threshold estimators (see stream_op.h).
#include "stream_op.h"

extern "C" {

namespace { struct ZelinskiOp : dsr_stream {     // ZelinskiPostFilter (postfilter.cc:350-493): ups[0] = beamformer output, ups[1..] = the snapshot array's channels
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
}; }
dsr_status dsr_zelinski_stream_create(dsr_stream* output, int fftLen, double alpha, int type, int minFrames, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(output, DSR_T_COMPLEX, "ZelinskiPostFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (output->size_ != fftLen) throw Error(DSR_E_DIMENSION, "Input block length (%d) != fftLen (%d)", output->size_, fftLen);      // postfilter.cc:359-362
    auto s = new_op<ZelinskiOp>(out, name, "ZelinskPostFilter", fftLen, DSR_T_COMPLEX); s->M = fftLen; s->alpha = alpha; s->ptype = type; s->minFrames = minFrames;
    s->manifold.assign((size_t) fftLen / 2 + 1, std::vector<double>()); s->checkOrder = false;
    hand_out(out, std::move(s), {output});
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
    ZelinskiOp* q = as_op<ZelinskiOp>(pf, "not a McCowan post-filter"); if (q->kind < 1) throw Error(DSR_E_PARAMETER, "not a McCowan post-filter");
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
    ZelinskiOp* q = as_op<ZelinskiOp>(pf, "not a Zelinski post-filter");
    need(chan, DSR_T_COMPLEX, "ZelinskiPostFilter channel"); if (chan->size_ != q->M) throw Error(DSR_E_DIMENSION, "channel size %d != fftLen %d", chan->size_, q->M);
    q->add_up(chan); q->ready = false;
  });
}
dsr_status dsr_zelinski_stream_set_manifold(dsr_stream* pf, int fbinX, const double* vec, int chanN)
{
  return guard([&] {
    ZelinskiOp* q = as_op<ZelinskiOp>(pf, "not a Zelinski post-filter", vec != nullptr);
    if (fbinX < 0 || fbinX >= q->M) throw Error(DSR_E_DIMENSION, "fbinX %d must be less than %d", fbinX, q->M);
    if (fbinX <= q->M / 2) q->manifold[fbinX].assign(vec, vec + 2 * (size_t) chanN);
    q->chanSet = chanN; q->ready = false;
  });
}
// highPassFilter (postfilter.cc:1222-1261)
namespace { struct HighPassOp : dsr_stream { int cut = 1; void compute() override { alloc(ups[0]->nFrames); op_highpass(ups[0]->d<double2>(), nFrames, size_, cut, d<double2>(), S0); } }; }
dsr_status dsr_highpass_filter_create(dsr_stream* output, float cutOffFreq, int sampleRate, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(output, DSR_T_COMPLEX, "highPassFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (sampleRate <= 0) throw Error(DSR_E_PARAMETER, "sample rate %d", sampleRate);
    const unsigned cut = (unsigned) ((float) output->size_ * cutOffFreq / (float) sampleRate);                 // postfilter.cc:1228
    if (cut < 1 || cut > (unsigned) output->size_ / 2) throw Error(DSR_E_INDEX, "highPassFilter: the cut-off bin %u must lie in 1..%d (the reference writes outside its vector otherwise)", cut, output->size_ / 2);
    auto s = new_op<HighPassOp>(out, name, "highPassFilter", output->size_, DSR_T_COMPLEX); s->cut = (int) cut; s->checkOrder = false;
    hand_out(out, std::move(s), {output});
  });
}
// SpectralSubtractor (spectralsubtraction.cc:141-267): ups = the channels of setChannel.  The noise estimates live as long as the operator
// (reset() never touches them); the state is sized by the first call that needs it, channels are set before that.
namespace { struct SpecSubOp : dsr_stream {
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
}; }
// SpectralSubtractorPtr(fftLen, halfBandShift, ft, flooringV, nm) (postfilter.i:182-184)
dsr_status dsr_specsub_stream_create(int fftLen, int halfBandShift, float ft, float flooringV, const char* name, dsr_stream** out)
{
  return guard([&] {
    auto s = new_op<SpecSubOp>(out, name, "SpectralSubtractor", fftLen, DSR_T_COMPLEX); s->M = fftLen; s->checkOrder = false;
    ok(dsr_specsub_create(fftLen, halfBandShift, ft, flooringV, &s->h)); hand_out(out, std::move(s));
  });
}
dsr_status dsr_specsub_stream_set_channel(dsr_stream* ss, dsr_stream* chan, double alpha)
{
  return guard([&] {
    SpecSubOp* q = as_op<SpecSubOp>(ss, "not a SpectralSubtractor stream"); need(chan, DSR_T_COMPLEX, "SpectralSubtractor channel");
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
    SpecSubOp* q = as_op<SpecSubOp>(ss, "not a SpectralSubtractor stream");
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
namespace { struct WienerOp : dsr_stream {       // WienerFilter (spectralsubtraction.cc:269-347): ups = target, noise; frame counter and PSD memories outlive reset()
  dsr_wiener* h = nullptr; int M = 0; DevBuf<float2> S, N; DevBuf<int> nf; DevBuf<unsigned char> state; bool have = false;
  ~WienerOp() override { if (h) dsr_wiener_destroy(h); }
  void compute() override {
    const int T = shortest(this, 0, 2); alloc(T); if (T <= 0) return;
    if (!have) { state.reserve(dsr_wiener_state_bytes(h, 1)); ok(dsr_wiener_state_init(h, state.p, 1, S0)); have = true; }
    const int F = M / 2 + 1; S.reserve((size_t) T * F); N.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, S.p, S0); op_pack_bins(ups[1]->d<double2>(), T, F, M, N.p, S0); nf.upload(&T, 1);
    ok(dsr_wiener_apply(h, (const float*) S.p, (const float*) N.p, nf.p, 1, T, dev.p, M, 1, state.p, S0));
  }
}; }
dsr_status dsr_wiener_stream_create(dsr_stream* targetSignal, dsr_stream* noiseSignal, int halfBandShift, float alpha, float flooringV, double beta, const char* name,
                                    dsr_stream** out)
{
  return guard([&] {
    need(targetSignal, DSR_T_COMPLEX, "WienerFilter"); need(noiseSignal, DSR_T_COMPLEX, "WienerFilter");
    auto s = new_op<WienerOp>(out, name, "WienerFilter", targetSignal->size_, DSR_T_COMPLEX); s->M = targetSignal->size_; s->checkOrder = false;
    ok(dsr_wiener_create(targetSignal->size_, noiseSignal->size_, halfBandShift, alpha, flooringV, beta, &s->h)); ok(dsr_wiener_carry(s->h, 1));
    hand_out(out, std::move(s), {targetSignal, noiseSignal});
  });
}
// what: 0 setNoiseAmplificationFactor(value), 1 startUpdatingNoisePSD, 2 stopUpdatingNoisePSD
dsr_status dsr_wiener_stream_control(dsr_stream* wf, int what, double value)
{
  return guard([&] {
    WienerOp* q = as_op<WienerOp>(wf, "not a WienerFilter stream");
    if (what == 0) ok(dsr_wiener_set_noise_amplification_factor(q->h, value)); else if (what == 1 || what == 2) ok(dsr_wiener_set_updating_noise_psd(q->h, what == 1));
    else throw Error(DSR_E_PARAMETER, "bad selector %d", what);
    q->ready = false;
  });
}
namespace { struct MaskOp : dsr_stream {         // BinaryMaskFilter / KimBinaryMaskFilter / IIDBinaryMaskFilter (binauralprocessing.cc:47-211, 431-520): ups = srcL, srcR
  dsr_binmask* h = nullptr; int M = 0; DevBuf<float2> L, R; DevBuf<int> nf; DevBuf<unsigned char> state; bool have = false;
  ~MaskOp() override { if (h) dsr_binmask_destroy(h); }
  void compute() override {
    const int T = shortest(this, 0, 2); alloc(T); if (T <= 0) return;
    if (!have) { state.reserve(dsr_binmask_state_bytes(h, 1)); ok(dsr_binmask_state_init(h, state.p, 1, S0)); have = true; }   // _prevMu = 1, untouched by reset()
    const int F = M / 2 + 1; L.reserve((size_t) T * F); R.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, L.p, S0); op_pack_bins(ups[1]->d<double2>(), T, F, M, R.p, S0); nf.upload(&T, 1);
    ok(dsr_binmask_apply(h, (const float*) L.p, (const float*) R.p, nf.p, 1, T, dev.p, M, 1, nullptr, nullptr, state.p, S0));
  }
}; }
// BinaryMaskFilterPtr / KimBinaryMaskFilterPtr / IIDBinaryMaskFilterPtr(chanX, srcL, srcR, M, threshold, alpha, dEta[, dPowerCoeff], nm) (postfilter.i:274-368)
dsr_status dsr_binmask_stream_create(int kind, unsigned chanX, dsr_stream* srcL, dsr_stream* srcR, unsigned M, float threshold, float alpha, float dEta,
                                     float dPowerCoeff, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(srcL, DSR_T_COMPLEX, "BinaryMaskFilter"); need(srcR, DSR_T_COMPLEX, "BinaryMaskFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (srcL->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Left input block length (%d) != M (%d)", srcL->size_, (int) M);       // binauralprocessing.cc:58-66
    if (srcR->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Right input block length (%d) != M (%d)", srcR->size_, (int) M);
    auto s = new_op<MaskOp>(out, name, kind == 1 ? "KimBinaryMaskFilter" : kind == 2 ? "IIDBinaryMaskFilter" : "BinaryMaskFilter", (int) M, DSR_T_COMPLEX);
    s->M = (int) M; s->checkOrder = false;
    ok(dsr_binmask_create(kind, chanX, (int) M, threshold, alpha, dEta, dPowerCoeff, &s->h)); ok(dsr_binmask_carry(s->h, 1));
    hand_out(out, std::move(s), {srcL, srcR});
  });
}
dsr_status dsr_binmask_stream_set_threshold(dsr_stream* m, float threshold)
{ return guard([&] { MaskOp* q = as_op<MaskOp>(m, "not a BinaryMaskFilter stream"); ok(dsr_binmask_set_threshold(q->h, threshold)); q->ready = false; }); }
dsr_status dsr_binmask_stream_threshold(dsr_stream* m, double* threshold)
{ return guard([&] { if (!threshold) throw Error(DSR_E_PARAMETER, "null argument"); *threshold = dsr_binmask_threshold(as_op<MaskOp>(m, "not a BinaryMaskFilter stream")->h); }); }
dsr_status dsr_binmask_stream_set_thresholds(dsr_stream* m, const double* thresholds, int n)
{ return guard([&] { MaskOp* q = as_op<MaskOp>(m, "not a BinaryMaskFilter stream"); ok(dsr_binmask_set_thresholds(q->h, thresholds, n)); q->ready = false; }); }
dsr_status dsr_binmask_stream_thresholds(dsr_stream* m, double* out, int n, int32_t* exists)
{ return guard([&] { ok(dsr_binmask_thresholds(as_op<MaskOp>(m, "not a BinaryMaskFilter stream")->h, out, n, exists)); }); }

// KimITD / IID / FDIID ThresholdEstimator (binauralprocessing.cc:232-426, 525-683, 702-928): ups = srcL, srcR; the output vector is never written
// there, so the rows are zeros; reset() clears the accumulators; calcThreshold divides them in place, so a second call differs, as there
namespace { struct ThestOp : dsr_stream {
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
}; }
// KimITDThresholdEstimatorPtr / IIDThresholdEstimatorPtr / FDIIDThresholdEstimatorPtr (postfilter.i:332-428)
dsr_status dsr_thest_stream_create(int kind, dsr_stream* srcL, dsr_stream* srcR, unsigned M, float minThreshold, float maxThreshold, float width, float minFreq,
                                   float maxFreq, int sampleRate, float dEta, float dPowerCoeff, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(srcL, DSR_T_COMPLEX, "ThresholdEstimator"); need(srcR, DSR_T_COMPLEX, "ThresholdEstimator"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (srcL->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Left input block length (%d) != M (%d)", srcL->size_, (int) M);
    if (srcR->size_ != (int) M) throw Error(DSR_E_DIMENSION, "Right input block length (%d) != M (%d)", srcR->size_, (int) M);
    auto s = new_op<ThestOp>(out, name, kind == 0 ? "KimITDThresholdEstimator" : kind == 1 ? "IIDThresholdEstimator" : "FDIIDThresholdEstimator", (int) M, DSR_T_COMPLEX);
    s->M = (int) M; s->checkOrder = false;
    ok(dsr_thest_create(kind, (int) M, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, &s->h));
    hand_out(out, std::move(s), {srcL, srcR});
  });
}
dsr_status dsr_thest_stream_calc_threshold(dsr_stream* e, double* threshold)
{ return guard([&] { if (!threshold) throw Error(DSR_E_PARAMETER, "null argument"); *threshold = as_op<ThestOp>(e, "not a ThresholdEstimator stream")->calc(); }); }
dsr_status dsr_thest_stream_threshold(dsr_stream* e, double* threshold)
{ return guard([&] { if (!threshold) throw Error(DSR_E_PARAMETER, "null argument"); *threshold = as_op<ThestOp>(e, "not a ThresholdEstimator stream")->threshold; }); }
// getCostFunction() / getCostFunction(freqX) of the last calcThreshold (zeros before one, where the reference prints a warning); FDIID: getThresholds
dsr_status dsr_thest_stream_get_cost_function(dsr_stream* e, unsigned freqX, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    ThestOp* q = as_op<ThestOp>(e, "not a ThresholdEstimator stream"); if (!out || !n) throw Error(DSR_E_PARAMETER, "null argument");
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
    ThestOp* q = as_op<ThestOp>(e, "not a ThresholdEstimator stream"); if (!out || n < q->M / 2 + 1) throw Error(DSR_E_DIMENSION, "%d doubles for %d bins", n, q->M / 2 + 1);
    std::fill(out, out + q->M / 2 + 1, 0.0); if (!q->thresholds.empty()) std::copy(q->thresholds.begin(), q->thresholds.end(), out);
  });
}

}  // extern "C"
