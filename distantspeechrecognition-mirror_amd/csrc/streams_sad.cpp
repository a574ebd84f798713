// csrc/streams_sad.cpp -- btk/sad over streams: the VAD metrics, the spectral-shape features, the hangover segmenters (see stream_op.h).
#include "stream_op.h"

extern "C" {

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
    std::unique_ptr<dsr_vad_metric> m(mk_metric(dsr_vad_metric::ENERGY, name, "Energy VAD Metric"));
    m->initialEnergy = initialEnergy; m->threshold = threshold; m->headN = headN; m->tailN = tailN; m->energiesN = energiesN;
    dsr_stream_retain(source); m->ups.push_back(source); *out = m.release();
  });
}
dsr_status dsr_sad_power_metric_create(int kind, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const char* name, dsr_vad_metric** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    unsigned lo, hi, bn; ok(dsr_sad_band(fftLen, sampleRate, lowCutoff, highCutoff, &lo, &hi, &bn));
    std::unique_ptr<dsr_vad_metric> m(mk_metric(dsr_vad_metric::POWER + kind, name, kind == 0 ? "Power Spectrum VAD Metric" : kind == 1 ? "NormalizedEnergyMetric" : "TSPS VAD Metric"));
    m->fftLen = fftLen; m->lowX = lo; m->highX = hi; m->E0 = kind == 2 ? 5000 : 1.0; *out = m.release();             // sad.cc:639, 733, 966
  });
}
dsr_status dsr_sad_ccc_metric_create(unsigned fftLen, unsigned nCand, double sampleRate, double lowCutoff, double highCutoff, const char* name, dsr_vad_metric** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftLen < 4 || fftLen > 2048 || (fftLen & (fftLen - 1))) throw Error(DSR_E_DIMENSION, "fftLen = %u is no power of two in [4, 2048].", fftLen);
    if (nCand < 1 || nCand > 64) throw Error(DSR_E_DIMENSION, "nCand = %u is outside [1, 64].", nCand);
    unsigned lo, hi, bn; ok(dsr_sad_band(fftLen, sampleRate, lowCutoff, highCutoff, &lo, &hi, &bn));
    std::unique_ptr<dsr_vad_metric> m(mk_metric(dsr_vad_metric::CCC, name, "CCC VAD Metric"));
    m->fftLen = fftLen; m->lowX = lo; m->highX = hi; m->nCand = nCand; m->threshold = 0.1; *out = m.release();       // sad.cc:822
  });
}
dsr_status dsr_sad_simple_energy_create(dsr_stream* samp, double threshold, double gamma, dsr_vad_metric** out)
{
  return guard([&] {
    need(samp, DSR_T_COMPLEX, "SimpleEnergyVAD"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    std::unique_ptr<dsr_vad_metric> m(mk_metric(dsr_vad_metric::SIMPLE, nullptr, "Simple Energy VAD"));
    m->threshold = threshold; m->gamma = gamma; m->fftLen = (unsigned) samp->size_; dsr_stream_retain(samp); m->ups.push_back(samp); *out = m.release();
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
namespace { struct ShapeOp : dsr_stream {        // the spectral-shape operators of sadFeature.cc
  int op = 0; float sampleRate = 16000.0f, thresh = 0.0f;
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_sad_shape_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, op, sampleRate, thresh, d<float>(), S0)); }
}; }
dsr_status dsr_sad_shape_create(dsr_stream* src, int op, float sampleRate, float thresh, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "a spectral-shape feature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (op < 0 || op > 3) throw Error(DSR_E_PARAMETER, "operator %d", op);
    int tx = 0; if (op == 1) ok(dsr_sad_band_ratio_index(src->size_, sampleRate, thresh, &tx));
    static const char* names[4] = { "Energy Diffusion", "Band Energy Ratio", "Negative Entropy", "Significant Subbands" };
    auto s = new_op<ShapeOp>(out, name, names[op], 1, DSR_T_FLOAT); s->op = op; s->sampleRate = sampleRate; s->thresh = thresh; hand_out(out, std::move(s), {src});
  });
}
namespace { struct HangoverOp : dsr_stream {     // HangoverVADFeature, HangoverMIVADFeature, HangoverMultiStageVADFeature (sad.cc:1705-1945); ups[0] = the source
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
}; }
dsr_status dsr_sad_hangover_create(dsr_stream* source, dsr_vad_metric* met, double threshold, unsigned headN, unsigned tailN, int kind, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(source, DSR_T_FLOAT, "HangoverVADFeature"); metric(met); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < 0 || kind > 2) throw Error(DSR_E_PARAMETER, "kind %d", kind);
    if (headN < 1) throw Error(DSR_E_DIMENSION, "headN = 0: the ring of buffered frames would be empty.");
    auto s = new_op<HangoverOp>(out, name, kind == 0 ? "Hangover VAD Feature" : kind == 1 ? "Hangover MIVAD Feature" : "HangoverMultiStageVADFeature", source->size_, DSR_T_FLOAT);
    s->kind = kind; s->headN = headN; s->tailN = tailN; met->refs++; s->metrics.push_back(met); s->thr.push_back(threshold); hand_out(out, std::move(s), {source});
  });
}
dsr_status dsr_sad_hangover_add_metric(dsr_stream* h, dsr_vad_metric* met, double threshold)
{
  return guard([&] {
    HangoverOp* s = as_op<HangoverOp>(h, "not a hangover stream"); metric(met);
    if (s->kind == 0) throw Error(DSR_E_PARAMETER, "HangoverVADFeature takes one metric.");
    if (s->metrics.size() >= (s->kind == 1 ? 3u : 8u)) throw Error(DSR_E_DIMENSION, "%s has all its metrics.", s->name.c_str());
    if (s->kind == 2 && s->metrics.size() >= 2 && met->stateful())      // sad.cc:1932-1935 calls it twice in a frame where its stage fires
      throw Error(DSR_E_CONSISTENCY, "%s: the stateful %s at stage %zu would be advanced twice a frame.", s->name.c_str(), met->name.c_str(), s->metrics.size());
    met->refs++; s->metrics.push_back(met); s->thr.push_back(threshold); s->ready = false;
  });
}
dsr_status dsr_sad_hangover_next_speaker(dsr_stream* h)
{ return guard([&] { HangoverOp* s = as_op<HangoverOp>(h, "not a hangover stream"); s->dsr_stream::reset(); for (size_t i = 0; i < s->metrics.size(); i++) s->metrics[i]->next_speaker(); }); }
dsr_status dsr_sad_hangover_prefix_n(dsr_stream* h, int* prefixN)
{ return guard([&] { HangoverOp* s = as_op<HangoverOp>(h, "not a hangover stream"); if (!prefixN) throw Error(DSR_E_PARAMETER, "null argument"); *prefixN = s->ready ? s->start : -(int) s->headN; }); }
dsr_status dsr_sad_hangover_decision_metric(dsr_stream* h, int* dm)
{ return guard([&] { HangoverOp* s = as_op<HangoverOp>(h, "not a hangover stream"); if (!dm) throw Error(DSR_E_PARAMETER, "null argument"); *dm = s->decision_metric(); }); }

}  // extern "C"
