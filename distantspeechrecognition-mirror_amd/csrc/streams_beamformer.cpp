// csrc/streams_beamformer.cpp -- the operators of btk/beamformer as streams: subband beamformers, SubbandMMI, the SRP DOA estimators, the
// spherical-array beamformers and trackers, the plane-wave simulator, the orthogonalizer (see stream_op.h).
#include "stream_op.h"
#include "srp_common.h"

extern "C" {

namespace { struct BfOp : dsr_stream {           // SubbandDS / SubbandGSC / SubbandMVDR as a stream
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
}; }
dsr_status dsr_subband_bf_create(dsr_bf* weights, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!weights || !out) throw Error(DSR_E_PARAMETER, "null argument");
    auto s = new_op<BfOp>(out, name, "SubbandBeamformer", dsr_bf_fft_len(weights), DSR_T_COMPLEX); s->w = weights; s->M = s->size_; s->checkOrder = false;
    hand_out(out, std::move(s));
  });
}
dsr_status dsr_subband_bf_set_channel(dsr_stream* bf, dsr_stream* chan)      // of every operator built on BfOp
{
  return guard([&] {
    BfOp* q = as_op<BfOp>(bf, "not a subband beamformer");
    need(chan, DSR_T_COMPLEX, "setChannel"); if (chan->size_ != q->M) throw Error(DSR_E_DIMENSION, "channel size %d != fftLen %d", chan->size_, q->M);
    q->add_up(chan); q->ready = false;
  });
}
namespace { struct MmiOp : BfOp {                // SubbandMMI as a stream (beamformer.cc:1973-2072); channels through dsr_subband_bf_set_channel
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
}; }
dsr_status dsr_subband_mmi_stream_create(dsr_mmi* weights, int fftLen, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!weights || !out) throw Error(DSR_E_PARAMETER, "null argument");
    auto s = new_op<MmiOp>(out, name, "SubbandMMI", fftLen, DSR_T_COMPLEX); s->w = nullptr; s->mm = weights; s->M = fftLen; s->checkOrder = false; hand_out(out, std::move(s));
  });
}

}  // extern "C"
namespace {
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

// a stream handle as the SRP operator Op, or Op's own refusal
template <class Op> Op& srp_op(dsr_stream* s, bool argsOk = true) { return *as_op<Op>(s, Op::Calls::notThis, argsOk); }

struct DoaOp : SrpFace<BfOp, LinSrp> { void pack_frames() override { pack_half(); } };
}  // namespace
extern "C" {
dsr_status dsr_doa_stream_create(dsr_doa* doa, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!doa || !out) throw Error(DSR_E_PARAMETER, "null argument");
    auto s = new_op<DoaOp>(out, name, "DOAEstimatorSRPDSBLAPtr", dsr_doa_fft_len(doa), DSR_T_COMPLEX); s->w = nullptr; s->est = doa; s->M = s->size_; s->checkOrder = false;
    hand_out(out, std::move(s));
  });
}
dsr_status dsr_doa_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n)
{ return guard([&] { srp_op<DoaOp>(s, out && n).get(what, out, outDoubles, n); }); }
dsr_status dsr_doa_stream_init_accs(dsr_stream* s) { return guard([&] { srp_op<DoaOp>(s).init_accs(); }); }
dsr_status dsr_doa_stream_final_nbest(dsr_stream* s) { return guard([&] { srp_op<DoaOp>(s).final_nbest(); }); }
namespace { struct SphBfOp : BfOp {              // EigenBeamformer / SphericalDSBeamformer and the further kinds (:1490-1542, :1858-1906, :2174-2222) as a stream (modalBeamformer.cc:347-399)
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
}; }
dsr_status dsr_sph_bf_stream_create(dsr_sph* sph, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!sph || !out) throw Error(DSR_E_PARAMETER, "null argument");
    static const char* const NAMES[] = {"EigenBeamformer", "SphericalDSBeamformer", "SphericalHWNCBeamformer", "SphericalGSCBeamformer",
                                        "SphericalHWNCGSCBeamformer", "SphericalSpatialDSBeamformer", "SphericalMOENBeamformer"};
    auto s = new_op<SphBfOp>(out, name, NAMES[dsr_sph_kind(sph)], dsr_sph_fft_len(sph), DSR_T_COMPLEX); s->w = nullptr; s->sph = sph; s->M = s->size_; s->checkOrder = false;
    hand_out(out, std::move(s));
  });
}
dsr_status dsr_sph_stream_get_eigenbeams(dsr_stream* s, double* out, size_t outDoubles, size_t* n)
{
  return guard([&] {
    SphBfOp* q = as_op<SphBfOp>(s, "not a spherical beamformer stream", out && n);
    if (q->F == 0) { q->F = q->M / 2 + 1; q->dim = dsr_sph_dim(q->sph); }
    const size_t need = (size_t) q->F * q->dim * 2;
    if (outDoubles < need) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, need);
    q->eigenbeams(out); *n = need;
  });
}
// the eigenbeams of the DOA operator: its range only, of the last ungated frame (a re-materialisation keeps it), anew after a settings change
namespace { struct SphDoaOp : SrpFace<SphBfOp, SphSrp> {
  void pack_frames() override { pack(); eigenRange = true; eigenLo = rangeUsed[0]; eigenHi = rangeUsed[1]; }   // the eigenbeams themselves only when getSnapShotArray asks
  bool moved() const override { return settings_moved(); }
  void served(int t) override { eigenFrame = t; }
}; }
dsr_status dsr_sph_doa_stream_create(dsr_sph* sph, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!sph || !out) throw Error(DSR_E_PARAMETER, "null argument");
    const char* dflt = "DirectionEstimatorSRPMB";               // both classes' default name (beamformer.i:539, :624)
    auto s = new_op<SphDoaOp>(out, name, dflt, dsr_sph_fft_len(sph), DSR_T_COMPLEX); s->w = nullptr; s->sph = s->est = sph; s->M = s->size_; s->checkOrder = false;
    hand_out(out, std::move(s));
  });
}
dsr_status dsr_sph_doa_stream_get(dsr_stream* s, int what, double* out, size_t outDoubles, size_t* n)
{ return guard([&] { srp_op<SphDoaOp>(s, out && n).get(what, out, outDoubles, n); }); }
dsr_status dsr_sph_doa_stream_init_accs(dsr_stream* s) { return guard([&] { srp_op<SphDoaOp>(s).init_accs(); }); }
dsr_status dsr_sph_doa_stream_final_nbest(dsr_stream* s) { return guard([&] { srp_op<SphDoaOp>(s).final_nbest(); }); }

// ModalSphericalArrayTracker / SpatialSphericalArrayTracker as a stream (tracker.cc:1280-1345 / :1356-1436) over a dsr_trk handle (not owned):
// ups = the 32 channels, a row = float (theta, phi).  The filter's state (position, K) belongs to the operator and outlives reset(), as in the
// reference; nextSpeaker() resets the stream and the state, setInitialPosition() moves the position alone.
namespace { struct TrkOp : dsr_stream {
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
}; }
dsr_status dsr_trk_stream_create(dsr_trk* trk, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!trk || !out) throw Error(DSR_E_ARG, "null argument");
    auto s = new_op<TrkOp>(out, name, "SphericalArrayTracker", 2, DSR_T_FLOAT); s->trk = trk; s->M = dsr_trk_fft_len(trk); s->checkOrder = false; hand_out(out, std::move(s));
  });
}
dsr_status dsr_trk_stream_set_channel(dsr_stream* s, dsr_stream* chan)
{
  return guard([&] {
    TrkOp* q = as_op<TrkOp>(s, "not a tracker stream"); need(chan, DSR_T_COMPLEX, "setChannel");
    if (chan->size_ != q->M) throw Error(DSR_E_DIMENSION, "channel size %d != fftLen %d", chan->size_, q->M);
    q->add_up(chan); q->ready = false;
  });
}
dsr_status dsr_trk_stream_next_speaker(dsr_stream* s)
{ return guard([&] { TrkOp* q = as_op<TrkOp>(s, "not a tracker stream"); q->reset(); ok(dsr_trk_next_speaker(q->trk)); q->stateReady = false; q->posPending = false; }); }
dsr_status dsr_trk_stream_set_initial_position(dsr_stream* s, double theta, double phi)
{
  return guard([&] {
    TrkOp* q = as_op<TrkOp>(s, "not a tracker stream"); q->posPending = true; q->pTheta = theta; q->pPhi = phi; q->ready = false;      // applied when the next frame is computed
  });
}
// PlaneWaveSimulator(source, modalDecomposition, channelX, theta, phi) (tracker.cc:1444-1488): ups[0] = the source spectrum; rows of fftLen bins
namespace { struct PwsOp : dsr_stream {
  int M = 0; std::vector<double2> hcoef; DevBuf<double2> coef; DevBuf<float2> src, Y; DevBuf<int> nf;
  void compute() override {
    const int T = ups[0]->nFrames, F = M / 2 + 1;
    alloc(T); if (T <= 0) return;
    if (!coef.p) coef.upload(hcoef);
    src.reserve((size_t) T * F); Y.reserve((size_t) T * M); op_pack_bins(ups[0]->d<double2>(), T, F, ups[0]->size_, src.p, S0); nf.upload(&T, 1);
    ok(dsr_pws_apply((const double*) coef.p, 1, (const float*) src.p, nf.p, 1, T, M, 1, (float*) Y.p, S0));
    op_expand_bins(Y.p, T, M, M, d<double2>(), S0);
  }
}; }
dsr_status dsr_pws_stream_create(dsr_stream* source, const dsr_trk* decomposition, unsigned channelX, double theta, double phi, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!decomposition || !out) throw Error(DSR_E_ARG, "null argument");
    need(source, DSR_T_COMPLEX, "PlaneWaveSimulator");
    const int M = dsr_trk_fft_len(decomposition), F = M / 2 + 1;
    if (channelX >= 32 || source->size_ < F) throw Error(DSR_E_ARG, "channel %u of 32, a source of at least %d bins", channelX, F);
    std::vector<double> all((size_t) 2 * 32 * F); ok(dsr_pws_coefficients(decomposition, theta, phi, all.data(), all.size()));
    auto s = new_op<PwsOp>(out, name, "Plane Wave Simulator", M, DSR_T_COMPLEX); s->M = M; s->checkOrder = false;
    const double2* row = reinterpret_cast<const double2*>(all.data()) + (size_t) channelX * F; s->hcoef.assign(row, row + F);
    hand_out(out, std::move(s), {source});
  });
}
namespace { struct OrthOp : dsr_stream {         // SubbandOrthogonalizer(beamformer, outChanX) (beamformer.cc:2817-2849): ups[0] = the SubbandMVDRGSC operator
  int outChanX = 0; DevBuf<float2> Z;
  void compute() override {
    BfOp* bf = as_op<BfOp>(ups[0], "SubbandOrthogonalizer needs a subband beamformer");
    const int T = bf->nFrames; alloc(T); if (T <= 0) return;
    if (outChanX <= 0) { DSR_HIP(hipMemcpyAsync(d<double2>(), bf->d<double2>(), sizeof(double2) * (size_t) T * size_, hipMemcpyDeviceToDevice, S0)); return; }
    const int F = bf->M / 2 + 1; Z.reserve((size_t) T * F);
    ok(dsr_bf_blocking_matrix_output(bf->w, (const float*) bf->X.p, 1, T, outChanX - 1, (float*) Z.p, S0));
    op_orth_assemble(Z.p, bf->d<double2>(), T, F, bf->M, d<double2>(), S0);
  }
}; }
dsr_status dsr_subband_orthogonalizer_create(dsr_stream* beamformer, int outChanX, const char* name, dsr_stream** out)
{
  return guard([&] {
    BfOp* q = as_op<BfOp>(beamformer, "not a subband beamformer"); if (!q->w || !out) throw Error(DSR_E_PARAMETER, "not a subband beamformer");
    auto s = new_op<OrthOp>(out, name, "SubbandOrthogonalizer", q->M, DSR_T_COMPLEX); s->outChanX = outChanX; s->checkOrder = false;
    hand_out(out, std::move(s), {beamformer});
  });
}

}  // extern "C"
