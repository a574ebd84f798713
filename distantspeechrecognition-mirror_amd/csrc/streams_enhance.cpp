// csrc/streams_enhance.cpp -- btk/cancelVP (the echo cancellers) and btk/dereverberation (WPE) as streams (see stream_op.h).
#include "stream_op.h"

extern "C" {

namespace { struct AecOp : dsr_stream {          // the echo cancellers of btk/cancelVP as a stream (cancelVP.cc:57-104, :141-209, :287-383, :513-650, :748-855, :1121-1198): ups = played, recorded
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
}; }
dsr_status dsr_aec_stream_create(dsr_aec* aec, dsr_stream* played, dsr_stream* recorded, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!aec || !out) throw Error(DSR_E_PARAMETER, "null argument");
    need(played, DSR_T_COMPLEX, "EchoCancellationFeature"); need(recorded, DSR_T_COMPLEX, "EchoCancellationFeature");
    if (played->size_ != dsr_aec_fft_len(aec) || recorded->size_ != played->size_)
      throw Error(DSR_E_DIMENSION, "played has %d subbands, recorded %d, the echo canceller %d", played->size_, recorded->size_, dsr_aec_fft_len(aec));
    auto s = new_op<AecOp>(out, name, "AEC", played->size_, DSR_T_COMPLEX); s->aec = aec; s->M = played->size_; hand_out(out, std::move(s), {played, recorded});
  });
}
dsr_status dsr_aec_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    AecOp* q = as_op<AecOp>(s, "not an echo cancellation stream", out != nullptr);
    require_device(); q->ensure_state();
    const size_t F = (size_t) q->M / 2 + 1, L = (size_t) dsr_aec_sample_n(q->aec);
    const size_t cnt = what == DSR_AEC_STATE_K ? F * L * L * 2 : what == DSR_AEC_STATE_SIGMA2V ? F : what == DSR_AEC_STATE_DTD ? 3 : what == DSR_AEC_STATE_BAND ? F * 3 :
                       (what == DSR_AEC_STATE_SKIPPED || what == DSR_AEC_STATE_RESETS) ? 1 : F * L * 2;
    ok(dsr_aec_state_read(q->aec, q->state.p, 1, what, out, outDoubles));
    if (n) *n = cnt;
  });
}
namespace { struct WpeOp : dsr_stream {          // SingleChannelWPEDereverberationFeature (dereverberation.cc:28-300)
  int M = 0, lowerN = 0, upperN = 0, iterationsN = 2; double loadDb = -20.0, bandWidth = 0.0, sampleRate = 16000.0; DevBuf<float2> Y, O; DevBuf<int> nf;
  void compute() override {
    const int T = ups[0]->nFrames; alloc(T); if (T <= 0) return;
    const int F = M / 2 + 1; Y.reserve((size_t) T * F); O.reserve((size_t) T * F);
    op_pack_bins(ups[0]->d<double2>(), T, F, M, Y.p, S0); nf.upload(&T, 1);
    ok(dsr_wpe_single((const float*) Y.p, nf.p, 1, T, M, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, (float*) O.p, nullptr, S0));
    op_expand_bins(O.p, T, F, M, d<double2>(), S0);
  }
}; }
dsr_status dsr_wpe_single_stream_create(dsr_stream* samples, int lowerN, int upperN, int iterationsN, double loadDb, double bandWidth, double sampleRate,
                                        const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samples, DSR_T_COMPLEX, "SingleChannelWPEDereverberationFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (upperN < lowerN) throw Error(DSR_E_PARAMETER, "bad prediction range [%d, %d]", lowerN, upperN);
    if (bandWidth > sampleRate / 2.0) throw Error(DSR_E_DIMENSION, "Bandwidth is greater than the Nyquist rate.");
    auto s = new_op<WpeOp>(out, name, "SingleChannelWPEDereverberationFeature", samples->size_, DSR_T_COMPLEX);
    s->M = samples->size_; s->lowerN = lowerN; s->upperN = upperN; s->iterationsN = iterationsN; s->loadDb = loadDb; s->bandWidth = bandWidth; s->sampleRate = sampleRate;
    hand_out(out, std::move(s), {samples});
  });
}
namespace { struct WpeMultiOp : dsr_stream {     // MultiChannelWPEDereverberationFeature(source, channelX) (dereverberation.cc:281-602): ups = the source's channels
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
}; }
dsr_status dsr_wpe_multi_feature_create(dsr_stream* const* channels, int channelsN, int channelX, int lowerN, int upperN, int iterationsN, double loadDb,
                                        double bandWidth, double sampleRate, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!channels || !out || channelsN < 1) throw Error(DSR_E_PARAMETER, "null argument");
    if (channelX < 0 || channelX >= channelsN) throw Error(DSR_E_INDEX, "channel %d of %d", channelX, channelsN);
    for (int c = 0; c < channelsN; c++) { need(channels[c], DSR_T_COMPLEX, "MultiChannelWPEDereverberation"); if (channels[c]->size_ != channels[0]->size_) throw Error(DSR_E_DIMENSION, "channel %d has %d subbands, channel 0 %d", c, channels[c]->size_, channels[0]->size_); }
    if (upperN < lowerN) throw Error(DSR_E_PARAMETER, "bad prediction range [%d, %d]", lowerN, upperN);
    if (bandWidth > sampleRate / 2.0) throw Error(DSR_E_DIMENSION, "Bandwidth is greater than the Nyquist rate.");
    auto s = new_op<WpeMultiOp>(out, name, "MultiChannelWPEDereverberationFeature", channels[0]->size_, DSR_T_COMPLEX);
    s->M = channels[0]->size_; s->channelX = channelX; s->lowerN = lowerN; s->upperN = upperN; s->iterationsN = iterationsN; s->loadDb = loadDb; s->bandWidth = bandWidth; s->sampleRate = sampleRate;
    for (int c = 0; c < channelsN; c++) s->add_up(channels[c]);
    s->checkOrder = true; hand_out(out, std::move(s));     // getOutput: jindex_error on out-of-order requests (:371-372)
  });
}
dsr_status dsr_wpe_multi_feature_set_filter_channel(dsr_stream* feature, int filterChan)
{
  return guard([&] {
    WpeMultiOp* q = as_op<WpeMultiOp>(feature, "not a MultiChannelWPEDereverberationFeature");
    if (filterChan >= (int) q->ups.size()) throw Error(DSR_E_INDEX, "filter channel %d of %d", filterChan, (int) q->ups.size());
    q->filterChan = filterChan < 0 ? -1 : filterChan; q->ready = false;
  });
}

}  // extern "C"
