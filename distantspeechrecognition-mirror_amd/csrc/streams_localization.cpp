// csrc/streams_localization.cpp -- btk/TDEstimator and btk/localization as streams: CCTDE, MCCLocalizer / MCCCalculator (see stream_op.h).
#include "stream_op.h"

extern "C" {

namespace {
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
CctdeOp* cctde_op(dsr_stream* s) { return as_op<CctdeOp>(s, "not a CCTDE stream"); }
}  // namespace
dsr_status dsr_cctde_stream_create(dsr_stream* samp1, dsr_stream* samp2, int fftLen, int nHeldMaxCC, int freqLowerLimit, int freqUpperLimit, const char* name,
                                   dsr_stream** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    const SampleSrc* a = as_op<const SampleSrc>(samp1, "CCTDE needs two SampleFeatures", true, DSR_E_TYPE);
    const SampleSrc* b = as_op<const SampleSrc>(samp2, "CCTDE needs two SampleFeatures", true, DSR_E_TYPE);
    if (a->sampleRate != b->sampleRate) throw Error(DSR_E_DIMENSION, "The sampling rates must be the same but %d != %d", a->sampleRate, b->sampleRate);   // CCTDE.cc:76-80
    if (a->size_ != b->size_) throw Error(DSR_E_DIMENSION, "Block sizes must be the same but %d != %d", a->size_, b->size_);
    (void) fftLen;                                                       // ignored there too: the length is the power of two that holds a block (CCTDE.cc:62-63)
    int N = 1; while (N < a->size_) N *= 2;
    ok(dsr_cctde_check(N, nHeldMaxCC));
    auto s = new_op<CctdeOp>(out, name, "CCTDE", nHeldMaxCC, DSR_T_DOUBLE);
    s->N = N; s->nHeld = nHeldMaxCC; s->lower = freqLowerLimit; s->upper = freqUpperLimit; s->vec.assign(nHeldMaxCC, 0.0); s->args.assign(nHeldMaxCC, 0); s->vals.assign(nHeldMaxCC, 0.0);
    s->checkOrder = false; hand_out(out, std::move(s), {samp1, samp2});
  });
}
dsr_status dsr_cctde_stream_next_x(dsr_stream* s, int chanX, int frameX, const void** data, size_t* n)
{ return guard([&] { CctdeOp& q = *cctde_op(s); if (!data) throw Error(DSR_E_PARAMETER, "null argument"); *data = q.nextX(chanX, frameX); if (n) *n = (size_t) q.nHeld; }); }
dsr_status dsr_cctde_stream_allsamples(dsr_stream* s, int fftLen) { return guard([&] { cctde_op(s)->allsamples(fftLen); }); }
dsr_status dsr_cctde_stream_get_sample_delays(dsr_stream* s, const int32_t** lags, size_t* n)
{ return guard([&] { CctdeOp& q = *cctde_op(s); if (!lags) throw Error(DSR_E_PARAMETER, "null argument"); *lags = q.args.data(); if (n) *n = q.args.size(); }); }
dsr_status dsr_cctde_stream_get_cc_values(dsr_stream* s, const double** values, size_t* n)
{ return guard([&] { CctdeOp& q = *cctde_op(s); if (!values) throw Error(DSR_E_PARAMETER, "null argument"); *values = q.vals.data(); if (n) *n = q.vals.size(); }); }
dsr_status dsr_cctde_stream_set_target_frequency_range(dsr_stream* s, int freqLowerLimit, int freqUpperLimit)
{ return guard([&] { CctdeOp& q = *cctde_op(s); q.lower = freqLowerLimit; q.upper = freqUpperLimit; }); }
int dsr_cctde_stream_fft_len(const dsr_stream* s) { const CctdeOp* q = dynamic_cast<const CctdeOp*>(s); return q ? q->N : 0; }
namespace { struct MccOp : dsr_stream {          // MCCLocalizer / MCCCalculator (MCCLocalizer.h:214-301): ups = the channels, a row = the best position / [cost, 0, 0]
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
}; }
dsr_status dsr_mcc_stream_create(dsr_mcc* mcc, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!mcc || !out) throw Error(DSR_E_PARAMETER, "null argument");
    auto s = new_op<MccOp>(out, name, "MCCSourceLocalizer", 3, DSR_T_DOUBLE); s->mcc = mcc; s->init(); s->checkOrder = false; hand_out(out, std::move(s));
  });
}
dsr_status dsr_mcccalc_stream_create(dsr_mcc* mcc, int normalizeVariance, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!mcc || !out) throw Error(DSR_E_PARAMETER, "null argument");
    auto s = new_op<MccOp>(out, name, "MCCCalculator", 3, DSR_T_DOUBLE); s->mcc = mcc; s->calc = true; s->normalize = normalizeVariance != 0; s->init(); s->checkOrder = false;
    hand_out(out, std::move(s));
  });
}
dsr_status dsr_mcc_stream_set_channel(dsr_stream* s, dsr_stream* chan)
{
  return guard([&] {
    MccOp* q = as_op<MccOp>(s, "not a MCC stream"); need(chan, DSR_T_FLOAT, "MCCLocalizer");
    if (!q->ups.empty() && q->ups[0]->size_ != chan->size_) throw Error(DSR_E_DIMENSION, "Block sizes must be the same but %d != %d", q->ups[0]->size_, chan->size_);
    q->add_up(chan);
  });
}
dsr_status dsr_mcccalc_stream_set_time_delays(dsr_stream* s, const double* delays, int n)
{
  return guard([&] {
    MccOp* q = as_op<MccOp>(s, "not a MCC stream"); if (!q->calc || !delays) throw Error(DSR_E_PARAMETER, "not an MCCCalculator stream");
    if (n != q->C) throw Error(DSR_E_DIMENSION, "%d delays for %d channels", n, q->C);
    q->delays.assign(delays, delays + n); q->haveDelays = true;
  });
}
dsr_status dsr_mcc_stream_get(dsr_stream* s, int what, int nth, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    MccOp* q = as_op<MccOp>(s, "not a MCC stream"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
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

}  // extern "C"
