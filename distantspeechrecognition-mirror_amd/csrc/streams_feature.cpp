// csrc/streams_feature.cpp -- the operators of btk/feature, btk/lpc and btk/convolution as streams (see stream_op.h).
#include "stream_op.h"

extern "C" {

namespace { struct Preemph : dsr_stream { double mu; void compute() override { alloc(ups[0]->nFrames); op_preemph(ups[0]->d<float>(), nFrames, size_, mu, d<float>(), S0); } }; }
dsr_status dsr_preemphasis_create(dsr_stream* samp, double mu, const char* name, dsr_stream** out)
{ return guard([&] { need(samp, DSR_T_FLOAT, "PreemphasisFeature"); auto s = new_op<Preemph>(out, name, "Preemphasis", samp->size_, DSR_T_FLOAT); s->mu = mu; hand_out(out, std::move(s), {samp}); }); }
namespace { struct Hamming : dsr_stream {
  DevBuf<double> w;
  void compute() override {
    alloc(ups[0]->nFrames);
    if (ups[0]->type == DSR_T_SHORT) op_hamming_s(ups[0]->d<short>(), nFrames, size_, w.p, d<float>(), S0);
    else op_hamming_f(ups[0]->d<float>(), nFrames, size_, w.p, d<float>(), S0);
  }
}; }
dsr_status dsr_hamming_create(dsr_stream* samp, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!samp || (samp->type != DSR_T_FLOAT && samp->type != DSR_T_SHORT)) throw Error(DSR_E_TYPE, "HammingFeature needs a float or short stream");
    auto s = new_op<Hamming>(out, name, "Hamming", samp->size_, DSR_T_FLOAT);
    std::vector<double> w(samp->size_); const double temp = 2. * M_PI / (double) (samp->size_ - 1);
    for (int i = 0; i < samp->size_; i++) w[i] = 0.54 - 0.46 * cos(temp * i);
    require_device(); s->w.upload(w); hand_out(out, std::move(s), {samp});
  });
}
namespace { struct FFTOp : dsr_stream { int L; DevBuf<double2> tw; void compute() override { alloc(ups[0]->nFrames); op_fft(ups[0]->d<float>(), nFrames, L, size_, tw.p, d<double2>(), S0); } }; }
dsr_status dsr_fft_create(dsr_stream* samp, int fftLen, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "FFTFeature");
    if (!is_pow2((unsigned) fftLen) || fftLen < 2 || fftLen > 8192 || samp->size_ > fftLen) throw Error(DSR_E_DIMENSION, "fftLen=%d must be a power of two >= the window length %d", fftLen, samp->size_);
    auto s = new_op<FFTOp>(out, name, "FFT", fftLen, DSR_T_COMPLEX); s->L = samp->size_;
    std::vector<double2> tw(fftLen); for (int k = 0; k < fftLen; k++) { const double a = 2.0 * M_PI * k / fftLen; tw[k] = make_double2(cos(a), sin(a)); }
    require_device(); s->tw.upload(tw); hand_out(out, std::move(s), {samp});
  });
}
namespace { struct PowerOp : dsr_stream { int fftLen; void compute() override { alloc(ups[0]->nFrames); op_power(ups[0]->d<double2>(), nFrames, fftLen, size_, d<double>(), S0); } }; }
dsr_status dsr_spectral_power_create(dsr_stream* fft, int powN, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(fft, DSR_T_COMPLEX, "SpectralPowerFeature"); const int sz = powN == 0 ? fft->size_ : powN;
    if (sz != fft->size_ && sz != fft->size_ / 2 + 1) throw Error(DSR_E_CONSISTENCY, "Number of power coefficients %d does not match FFT length %d.", sz, fft->size_);
    auto s = new_op<PowerOp>(out, name, "Power", sz, DSR_T_DOUBLE); s->fftLen = fft->size_; hand_out(out, std::move(s), {fft});
  });
}
namespace { struct VtlnOp : dsr_stream {
  DevBuf<int> s, c, o; DevBuf<double> coef, div; int rf = 0;
  void compute() override { alloc(ups[0]->nFrames); op_vtln(ups[0]->d<double>(), nFrames, size_, s.p, c.p, o.p, coef.p, div.p, rf, d<double>(), S0); }
}; }
dsr_status dsr_vtln_create(dsr_stream* pow, int coeffN, double ratio, double edge, int version, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(pow, DSR_T_DOUBLE, "VTLNFeature"); const int N = coeffN == 0 ? pow->size_ : coeffN;
    if (N != pow->size_) throw Error(DSR_E_DIMENSION, "VTLN size %d != input size %d", N, pow->size_);
    if (version != 1 && version != 2) throw Error(DSR_E_PARAMETER, "unknown version number (%d)", version);
    auto s = new_op<VtlnOp>(out, name, "VTLN", N, DSR_T_DOUBLE); SparseRowsD r; build_vtln_rows(N, ratio, edge, version, r);
    require_device(); s->s.upload(r.start); s->c.upload(r.count); s->o.upload(r.off); s->coef.upload(r.coef); s->div.upload(r.div); s->rf = r.roundFloat;
    hand_out(out, std::move(s), {pow});
  });
}
namespace { struct MelOp : dsr_stream {
  DevBuf<int> s, c, o; DevBuf<float> coef; int inN;
  void compute() override { alloc(ups[0]->nFrames); op_mel(ups[0]->d<double>(), nFrames, inN, size_, s.p, c.p, o.p, coef.p, d<double>(), S0); }
}; }
dsr_status dsr_mel_create(dsr_stream* mag, int powN, float rate, float low, float up, int filterN, int version, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(mag, DSR_T_DOUBLE, "MelFeature"); const int P = powN == 0 ? mag->size_ : powN;
    auto s = new_op<MelOp>(out, name, "MelFFT", filterN, DSR_T_DOUBLE); SparseRowsF r; build_mel_rows(P, rate, low, up, filterN, version, r);
    if (mag->size_ < r.nReq) throw Error(DSR_E_CONSISTENCY, "Matrix columns differ: %d and %d.", mag->size_, r.nReq);
    for (size_t i = 0; i < r.start.size(); i++) if (r.start[i] + r.count[i] > mag->size_) throw Error(DSR_E_CONSISTENCY, "mel filter %zu reads past the input", i);
    require_device(); s->s.upload(r.start); s->c.upload(r.count); s->o.upload(r.off); s->coef.upload(r.coef); s->inN = mag->size_;
    hand_out(out, std::move(s), {mag});
  });
}
namespace { struct LogOp : dsr_stream { double m, a; int sphinx; void compute() override { alloc(ups[0]->nFrames); op_log(ups[0]->d<double>(), (long) nFrames * size_, m, a, sphinx, d<float>(), S0); } }; }
dsr_status dsr_log_create(dsr_stream* mel, double m, double a, int sphinx, const char* name, dsr_stream** out)
{ return guard([&] { need(mel, DSR_T_DOUBLE, "LogFeature"); auto s = new_op<LogOp>(out, name, "LogMel", mel->size_, DSR_T_FLOAT); s->m = m; s->a = a; s->sphinx = sphinx; hand_out(out, std::move(s), {mel}); }); }
namespace { struct GemvOp : dsr_stream {         // CepstralFeature and LinearTransformFeature
  DevBuf<float> A; std::vector<float> hA;
  void compute() override { alloc(ups[0]->nFrames); op_sgemv(ups[0]->d<float>(), nFrames, ups[0]->size_, size_, A.p, d<float>(), S0); }
}; }
dsr_status dsr_cepstral_create(dsr_stream* mel, int ncep, int type, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(mel, DSR_T_FLOAT, "CepstralFeature");
    auto s = new_op<GemvOp>(out, name, "Cepstral", ncep, DSR_T_FLOAT); build_dct(ncep, mel->size_, type, s->hA);
    require_device(); s->A.upload(s->hA); hand_out(out, std::move(s), {mel});
  });
}
dsr_status dsr_linear_transform_create(dsr_stream* src, int sz, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "LinearTransformFeature"); if (sz < 1) throw Error(DSR_E_DIMENSION, "bad output size %d", sz);
    auto s = new_op<GemvOp>(out, name, "Transform", sz, DSR_T_FLOAT); s->hA.assign((size_t) sz * src->size_, 0.0f);     // calloc'd matrix (feature.cc:2936)
    require_device(); s->A.upload(s->hA); hand_out(out, std::move(s), {src});
  });
}
dsr_status dsr_linear_transform_set(dsr_stream* s, const float* matrix)
{
  return guard([&] {
    GemvOp* q = as_op<GemvOp>(s, "not a linear transform", matrix != nullptr);
    q->hA.assign(matrix, matrix + q->hA.size()); q->A.upload(q->hA); q->ready = false;
  });
}
// LinearTransformFeature::load(fileName, old) (feature.cc:2972-2976): gsl_matrix_float_load into the operator's (size x srcSize) matrix, then the
// crop to (size x srcSize) -- which only ever shrinks (gslmatrix.cc:6-15), so a Janus file must carry exactly that shape.
dsr_status dsr_linear_transform_load(dsr_stream* s, const char* fileName, int old)
{
  return guard([&] {
    GemvOp* q = as_op<GemvOp>(s, "not a linear transform", fileName != nullptr);
    const int rows = q->size_, cols = q->ups[0]->size_;
    std::vector<float> m((size_t) rows * cols, 0.0f); int r2 = 0, c2 = 0;
    ok(dsr_fmat_load(fileName, old, rows, cols, m.data(), &r2, &c2));
    if (r2 < rows) throw Error(DSR_E_DIMENSION, "Cannot resize from %d to %d", r2, rows);           // the crop back to (size x srcSize)
    if (c2 < cols) throw Error(DSR_E_DIMENSION, "Cannot resize from %d to %d", c2, cols);
    q->hA = m; q->A.upload(q->hA); q->ready = false;
  });
}
namespace { struct StorageOp : dsr_stream {      // StorageFeature (feature.cc:2992-3085)
  void compute() override {
    if (ups[0]->nFrames > 100000) throw Error(DSR_E_DIMENSION, "Frame %d is greater than maximum number %d.", ups[0]->nFrames, 100000);
    alloc(ups[0]->nFrames); if (nFrames > 0) DSR_HIP(hipMemcpy(dev.p, ups[0]->dev.p, (size_t) nFrames * rowBytes(), hipMemcpyDeviceToDevice));
  }
}; }
dsr_status dsr_storage_create(dsr_stream* src, const char* name, dsr_stream** out)
{ return guard([&] { need(src, DSR_T_FLOAT, "StorageFeature"); auto s = new_op<StorageOp>(out, name, "Storage", src->size_, DSR_T_FLOAT); s->randomAccess = true; s->checkOrder = false; hand_out(out, std::move(s), {src}); }); }
// StorageFeature::write(fileName, plainText) / read(fileName) (feature.cc:3025-3067), quirks kept: the count that is written is _frameX -- the
// index of the last frame, one less than the number of frames that follow it; read() takes that number for _frameX and reads that many frames,
// i.e. one fewer than the file holds.  Binary: big-endian ints (write_int) and native-endian float blocks (gsl_vector_float_fwrite).
dsr_status dsr_storage_write(dsr_stream* s, const char* fileName, int plainText)
{
  return guard([&] {
    StorageOp* q = as_op<StorageOp>(s, "not a StorageFeature", fileName != nullptr);
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
    StorageOp* q = as_op<StorageOp>(s, "not a StorageFeature", fileName != nullptr);
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
namespace { struct CmnOp : dsr_stream {          // MeanSubtractionFeature(src, weight, devNormFactor, runon): ups[1] (optional) = the weight stream, element 0 of each frame
  int mode; double dnf;
  void compute() override {
    int T = ups[0]->nFrames;
    if (ups.size() > 1 && ups[1]->nFrames < T) T = ups[1]->nFrames;           // the weight stream ends first: so does the loop over the frames (feature.cc:2640-2644)
    alloc(T);
    op_cmn(ups[0]->d<float>(), nFrames, size_, mode, dnf, d<float>(), S0, ups.size() > 1 ? ups[1]->d<float>() : nullptr, ups.size() > 1 ? ups[1]->size_ : 0);
  }
}; }
dsr_status dsr_mean_subtraction_create(dsr_stream* src, double dnf, int runon, const char* name, dsr_stream** out)
{ return guard([&] { need(src, DSR_T_FLOAT, "MeanSubtractionFeature"); auto s = new_op<CmnOp>(out, name, "Mean Subtraction", src->size_, DSR_T_FLOAT); s->mode = runon ? 2 : 1; s->dnf = dnf; hand_out(out, std::move(s), {src}); }); }
dsr_status dsr_mean_subtraction_set_weight(dsr_stream* cmn, dsr_stream* weight)
{
  return guard([&] {
    CmnOp* q = as_op<CmnOp>(cmn, "not a MeanSubtractionFeature");
    need(weight, DSR_T_FLOAT, "MeanSubtractionFeature weight"); if (q->ups.size() > 1) throw Error(DSR_E_CONSISTENCY, "the weight stream is already set");
    q->add_up(weight); q->ready = false;
  });
}
namespace { struct AdjOp : dsr_stream {
  int delta;
  void compute() override { int T = ups[0]->nFrames; if (delta > 0 && T < delta) T = 0; alloc(T); op_adjacent(ups[0]->d<float>(), T, ups[0]->size_, delta, d<float>(), S0); }
}; }
dsr_status dsr_adjacent_create(dsr_stream* single, int delta, const char* name, dsr_stream** out)
{ return guard([&] { need(single, DSR_T_FLOAT, "AdjacentFeature"); auto s = new_op<AdjOp>(out, name, "Adjacent", (2 * delta + 1) * single->size_, DSR_T_FLOAT); s->delta = delta; hand_out(out, std::move(s), {single}); }); }
namespace { struct FirOp : dsr_stream {         // FilterFeature (feature.h:1315-1410, feature.cc:3206-3313)
  std::vector<double> a;
  void compute() override {
    const int T = ups[0]->nFrames, lenA = (int) a.size(), Tout = T + (lenA == 1 ? 1 : 0);
    dev.reserve((size_t) (Tout > 0 ? Tout : 1) * rowBytes()); alloc(dsr_fir_frames_count(T, lenA));
    if (Tout > 0) ok(dsr_fir_frames_run(ups[0]->d<float>(), nullptr, a.data(), lenA, 1, T, size_, d<float>(), S0));
  }
}; }
dsr_status dsr_filter_feature_create(dsr_stream* src, const double* a, int lenA, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "FilterFeature");
    if (!a || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (lenA < 1 || lenA % 2 != 1) throw Error(DSR_E_DIMENSION, "Length of filter (%d) is not odd.", lenA);                  // feature.cc:3219-3220
    auto s = new_op<FirOp>(out, name, "Filter", src->size_, DSR_T_FLOAT); s->a.assign(a, a + lenA); hand_out(out, std::move(s), {src});
  });
}
namespace { struct MergeOp : dsr_stream {       // MergeFeature (feature.cc:3318-3350): stat, delta, deltaDelta side by side
  void compute() override {
    alloc(shortest(this, 0, 3));
    size_t off = 0;
    for (int k = 0; k < 3; k++) {
      const size_t w = ups[k]->rowBytes();
      if (nFrames > 0) DSR_HIP(hipMemcpy2DAsync(dev.p + off, rowBytes(), ups[k]->dev.p, w, w, (size_t) nFrames, hipMemcpyDeviceToDevice, S0));
      off += w;
    }
  }
}; }
dsr_status dsr_merge_feature_create(dsr_stream* stat, dsr_stream* delta, dsr_stream* deltaDelta, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(stat, DSR_T_FLOAT, "MergeFeature"); need(delta, DSR_T_FLOAT, "MergeFeature"); need(deltaDelta, DSR_T_FLOAT, "MergeFeature");
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    hand_out(out, new_op<MergeOp>(out, name, "Merge", stat->size_ + delta->size_ + deltaDelta->size_, DSR_T_FLOAT), {stat, delta, deltaDelta});
  });
}
namespace { struct SrcOp : dsr_stream {         // SamplerateConversionFeature (feature.h:794-816, feature.cc:1607-1699)
  dsr_src* plan = nullptr;
  ~SrcOp() override { if (plan) dsr_src_destroy(plan); }
  void compute() override {
    const int64_t n = (int64_t) ups[0]->nFrames * ups[0]->size_, m = dsr_src_out_samples(plan, n);
    dev.reserve((size_t) (m > 0 ? m : 1) * sizeof(float)); alloc((int) (m / size_));
    if (m > 0) ok(dsr_src_apply(plan, ups[0]->d<float>(), nullptr, 1, 1, n, nullptr, 1, d<float>(), nullptr, m, S0));
  }
}; }
dsr_status dsr_src_stream_create(dsr_stream* src, unsigned srcRate, unsigned dstRate, unsigned len, const char* method, const char* name,
                                 dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "SamplerateConversionFeature");
    if (!method) throw Error(DSR_E_PARAMETER, "null argument");
    const unsigned size = len ? len : (unsigned) (unsigned) ((float) src->size_ * (float) dstRate / (float) srcRate);   // feature.cc:1612
    if (size < 1 || size > 0x7fffffffu) throw Error(DSR_E_DIMENSION, "SamplerateConversionFeature: blocks of %u samples", size);
    auto s = new_op<SrcOp>(out, name, "SamplerateConversion", (int) size, DSR_T_FLOAT);
    ok(dsr_src_create(srcRate, dstRate, method, &s->plan));
    hand_out(out, std::move(s), {src});
  });
}

// ---- btk/lpc
namespace { struct LpcOp : dsr_stream {         // WarpMVDR/BurgMVDR/WarpLPC/BurgLPC features (lpc.h:86-195,262-331)
  dsr_lpc* plan = nullptr;
  ~LpcOp() override { if (plan) dsr_lpc_destroy(plan); }
  void compute() override {
    alloc(ups[0]->nFrames);
    if (nFrames > 0) ok(dsr_lpc_run(plan, ups[0]->d<float>(), nFrames, d<double>(), S0));
  }
}; }
dsr_status dsr_lpc_feature_create(dsr_stream* src, int order, int correlate, float warp, int method, int kind, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, kind ? "LPCFeature" : "MVDRFeature");
    auto s = new_op<LpcOp>(out, name, kind ? "LPC" : "MVDR", src->size_ / 2 + 1, DSR_T_DOUBLE);
    ok(dsr_lpc_create(src->size_, order, correlate, warp, method, kind, &s->plan));
    hand_out(out, std::move(s), {src});
  });
}
namespace { struct WtMvdrOp : dsr_stream {      // WarpedTwiceMVDRFeature (lpc.h:205-246, lpc.cc:409-468)
  dsr_wtmvdr* plan = nullptr;
  ~WtMvdrOp() override { if (plan) dsr_wtmvdr_destroy(plan); }
  void compute() override {
    alloc(ups[0]->nFrames);
    if (nFrames > 0) ok(dsr_wtmvdr_run(plan, ups[0]->d<float>(), nullptr, nFrames, d<double>(), nullptr, nullptr, S0));
  }
}; }
dsr_status dsr_wtmvdr_feature_create(dsr_stream* src, int order, int correlate, float warp, int warpFactorFixed, float sensibility, const char* name,
                                     dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "WarpedTwiceMVDRFeature");
    auto s = new_op<WtMvdrOp>(out, name, "WTMVDR", src->size_ / 2 + 1, DSR_T_DOUBLE);
    ok(dsr_wtmvdr_create(src->size_, order, correlate, warp, warpFactorFixed, sensibility, &s->plan));
    hand_out(out, std::move(s), {src});
  });
}
namespace { struct SpecSmoothOp : dsr_stream {  // SpectralSmoothing (lpc.h:342-358, lpc.cc:485-529): ups[0] = adjustTo, ups[1] = adjustFrom
  void compute() override {
    alloc(shortest(this, 0, 2));
    if (nFrames > 0) ok(dsr_specsmooth_run(ups[0]->d<double>(), ups[1]->d<double>(), nFrames, size_, d<double>(), S0));
  }
}; }
dsr_status dsr_spectral_smoothing_create(dsr_stream* adjustTo, dsr_stream* adjustFrom, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(adjustTo, DSR_T_DOUBLE, "SpectralSmoothing"); need(adjustFrom, DSR_T_DOUBLE, "SpectralSmoothing");
    if (adjustTo->size_ != adjustFrom->size_) throw Error(DSR_E_DIMENSION, "Feature sizes (%d vs. %d) do not match.", adjustTo->size_, adjustFrom->size_);   // lpc.cc:476-477
    if (adjustTo->size_ < 2) throw Error(DSR_E_PARAMETER, "SpectralSmoothing needs at least 2 coefficients, got %d", adjustTo->size_);
    hand_out(out, new_op<SpecSmoothOp>(out, name, "Spectral Smoothing", adjustTo->size_, DSR_T_DOUBLE), {adjustTo, adjustFrom});
  });
}

// ---- btk/convolution
namespace {
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
void conv_create(int kind, dsr_stream* src, const double* h, int P, int fftLen, const char* name, const char* dflt, dsr_stream** out)
{
  need(src, DSR_T_FLOAT, dflt);
  if (!out) throw Error(DSR_E_PARAMETER, "null argument");
  if (!h) throw Error(DSR_E_PARAMETER, "null impulse response");
  auto s = new_op<ConvOp>(out, name, dflt, 0, DSR_T_FLOAT);
  ok(dsr_conv_create(kind, src->size_, P, fftLen, 1, &s->plan)); s->size_ = dsr_conv_size(s->plan);
  ok(dsr_conv_set_response(s->plan, h));
  hand_out(out, std::move(s), {src});
}
}  // namespace
dsr_status dsr_overlap_add_create(dsr_stream* src, const double* h, int P, int fftLen, const char* name, dsr_stream** out)
{ return guard([&] { conv_create(0, src, h, P, fftLen, name, "Overlap Add", out); }); }
dsr_status dsr_overlap_save_create(dsr_stream* src, const double* h, int P, const char* name, dsr_stream** out)
{ return guard([&] { conv_create(1, src, h, P, 0, name, "Overlap Save", out); }); }
dsr_status dsr_overlap_save_update(dsr_stream* s, const double* delta, int n)
{
  return guard([&] {
    ConvOp* q = as_op<ConvOp>(s, "not a OverlapSave stream");
    if (!delta) throw Error(DSR_E_PARAMETER, "null argument");
    if (n != q->ups[0]->size_)                                                                                                 // convolution.cc:284-286
      throw Error(DSR_E_DIMENSION, "Dimension of udpate vector (%d) does not match frequency response (%d).", n, q->ups[0]->size_);
    ok(dsr_conv_update(q->plan, 0, delta));
  });
}

// ---- the scalar feature operators of include/dsr.h section 6c (csrc/k_featops.hip), one utterance a call
namespace {
struct SignalPowerOp : dsr_stream { void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_signal_power_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, d<float>(), S0)); } };
struct ZcrOp : dsr_stream { void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_zcr_hamming_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, d<float>(), S0)); } };
}
dsr_status dsr_signal_power_create(dsr_stream* samp, const char* name, dsr_stream** out)
{ return guard([&] { need(samp, DSR_T_FLOAT, "SignalPowerFeature"); hand_out(out, new_op<SignalPowerOp>(out, name, "Signal Power", 1, DSR_T_FLOAT), {samp}); }); }
dsr_status dsr_zcr_hamming_create(dsr_stream* samp, const char* name, dsr_stream** out)
{ return guard([&] { need(samp, DSR_T_FLOAT, "ZeroCrossingRateHammingFeature"); hand_out(out, new_op<ZcrOp>(out, name, "Zero Crossing Rate Hamming", 1, DSR_T_FLOAT), {samp}); }); }
namespace { struct YinOp : dsr_stream {
  unsigned sr = 16000; float tr = 0.5f;
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_yin_pitch_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, sr, tr, d<float>(), nullptr, nullptr, S0)); }
}; }
dsr_status dsr_yin_pitch_create(dsr_stream* samp, unsigned samplerate, float threshold, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "YINPitchFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (samp->size_ < 2) throw Error(DSR_E_DIMENSION, "YIN needs frames of at least 2 samples, got %d.", samp->size_);
    auto s = new_op<YinOp>(out, name, "YIN Pitch", 1, DSR_T_FLOAT); s->sr = samplerate; s->tr = threshold; hand_out(out, std::move(s), {samp});
  });
}
namespace { struct SpikeOp : dsr_stream { int tapN = 3; void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_spike_filter_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, tapN, d<float>(), S0)); } }; }
dsr_status dsr_spike_filter_create(dsr_stream* src, unsigned tapN, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "SpikeFilter"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    ok(dsr_spike_filter_check(src->size_, tapN > 0x7fffffffu ? 0x7fffffff : (int) tapN));
    auto s = new_op<SpikeOp>(out, name, "Spike Filter", src->size_, DSR_T_FLOAT); s->tapN = (int) tapN; hand_out(out, std::move(s), {src});
  });
}
namespace { struct Spike2Op : dsr_stream {      // SpikeFilter2 (feature.cc:3701-3776): reset() sets _meanslope = _startslope, _count = 0
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
}; }
dsr_status dsr_spike_filter2_create(dsr_stream* src, unsigned width, float maxslope, float startslope, float thresh, float alpha, unsigned verbose, const char* name,
                                    dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "SpikeFilter2"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    (void) verbose;                                                                                                            // its printf passes floats to %d
    if (src->size_ > 16000) throw Error(DSR_E_DIMENSION, "SpikeFilter2 stages a block in LDS: %d samples exceed 16000.", src->size_);
    auto s = new_op<Spike2Op>(out, name, "Spike Filter 2", src->size_, DSR_T_FLOAT);
    s->width = width; s->maxslope = maxslope; s->startslope = startslope; s->thresh = thresh; s->alpha = alpha; hand_out(out, std::move(s), {src});
  });
}
dsr_status dsr_spike_filter2_spikes(dsr_stream* s, unsigned* n)
{ return guard([&] { Spike2Op* q = as_op<Spike2Op>(s, "not a SpikeFilter2 stream"); if (!n) throw Error(DSR_E_PARAMETER, "null argument"); *n = q->spikes; }); }
namespace { struct MinMaxOp : dsr_stream {      // ALogFeature / NormalizeFeature (feature.cc:1383-1514): (min, max) kept across reset() when runon
  int alog = 0, runon = 0; double p0 = 0.0, p1 = 0.0; bool fresh = true; DevBuf<double> state;
  void compute() override {
    alloc(ups[0]->nFrames);
    state.reserve(2);
    if (fresh || !runon) { ok(dsr_minmax_state_init(state.p, 1, S0)); fresh = false; }
    if (nFrames <= 0) return;
    if (alog) ok(dsr_alog_run(ups[0]->d<float>(), nullptr, 1, nFrames, ups[0]->size_, p0, p1, runon, state.p, d<float>(), S0));
    else ok(dsr_normalize_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, p0, p1, runon, state.p, d<float>(), S0));
  }
}; }
dsr_status dsr_alog_create(dsr_stream* samp, double m, double a, int runon, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "ALogFeature");
    auto s = new_op<MinMaxOp>(out, name, "ALog Power", 1, DSR_T_FLOAT); s->alog = 1; s->runon = runon != 0; s->p0 = m; s->p1 = a; hand_out(out, std::move(s), {samp});
  });
}
dsr_status dsr_normalize_create(dsr_stream* samp, double min, double max, int runon, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "NormalizeFeature");
    auto s = new_op<MinMaxOp>(out, name, "Normalize", samp->size_, DSR_T_FLOAT); s->runon = runon != 0; s->p0 = min; s->p1 = max; hand_out(out, std::move(s), {samp});
  });
}
dsr_status dsr_minmax_next_speaker(dsr_stream* s)
{ return guard([&] { as_op<MinMaxOp>(s, "not a ALogFeature or NormalizeFeature stream")->fresh = true; }); }
namespace { struct ThreshAmpOp : dsr_stream {   // ThresholdFeature (compare -1, 0, 1) and AmplificationFeature (compare 2)
  double value = 0.0, thresh = 1.0; int compare = 1;
  void compute() override {
    alloc(ups[0]->nFrames);
    if (nFrames <= 0) return;
    if (compare == 2) ok(dsr_amplify_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, value, d<float>(), S0));
    else ok(dsr_threshold_run(ups[0]->d<float>(), nullptr, 1, nFrames, size_, value, thresh, compare, d<float>(), S0));
  }
}; }
dsr_status dsr_threshold_create(dsr_stream* samp, double value, double thresh, const char* mode, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "ThresholdFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    int compare = 0; ok(dsr_threshold_mode(mode, &compare));
    auto s = new_op<ThreshAmpOp>(out, name, "Threshold", samp->size_, DSR_T_FLOAT); s->value = value; s->thresh = thresh; s->compare = compare; hand_out(out, std::move(s), {samp});
  });
}
dsr_status dsr_amplification_create(dsr_stream* src, double amplify, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "AmplificationFeature");
    auto s = new_op<ThreshAmpOp>(out, name, "Amplification", src->size_, DSR_T_FLOAT); s->value = amplify; s->compare = 2; hand_out(out, std::move(s), {src});
  });
}
namespace { struct ResampleOp : dsr_stream {
  double ratio = 16.0 / 22.05; int len = 0;
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_spectral_resample_run(ups[0]->d<double>(), nullptr, 1, nFrames, ups[0]->size_, ratio, len, d<double>(), S0)); }
}; }
dsr_status dsr_spectral_resampling_create(dsr_stream* src, double ratio, unsigned len, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_DOUBLE, "SpectralResamplingFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    int outN = 0; ok(dsr_spectral_resample_size(src->size_, ratio, (int) len, &outN));
    auto s = new_op<ResampleOp>(out, name, "Resampling", outN, DSR_T_DOUBLE); s->ratio = ratio; s->len = (int) len; hand_out(out, std::move(s), {src});
  });
}
namespace { struct SphinxMelOp : dsr_stream {
  dsr_sphinx_mel* plan = nullptr;
  ~SphinxMelOp() override { if (plan) dsr_sphinx_mel_destroy(plan); }
  void compute() override { alloc(ups[0]->nFrames); if (nFrames > 0) ok(dsr_sphinx_mel_apply(plan, ups[0]->d<double>(), nullptr, 1, nFrames, d<double>(), S0)); }
}; }
dsr_status dsr_sphinx_mel_feature_create(dsr_stream* mag, unsigned fftN, unsigned powerN, float sampleRate, float lowerF, float upperF, unsigned filterN,
                                         const char* name, dsr_stream** out)
{
  return guard([&] {
    need(mag, DSR_T_DOUBLE, "SphinxMelFeature"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    const unsigned pN = powerN == 0 ? (unsigned) mag->size_ : powerN;
    if ((int) pN != mag->size_) throw Error(DSR_E_DIMENSION, "SphinxMelFeature: powerN = %u does not match the source's size %d.", pN, mag->size_);   // gsl_blas_dgemv's own check
    auto s = new_op<SphinxMelOp>(out, name, "Sphinx Mel Filter Bank", (int) filterN, DSR_T_DOUBLE);
    ok(dsr_sphinx_mel_create(fftN, pN, sampleRate, lowerF, upperF, filterN, &s->plan)); hand_out(out, std::move(s), {mag});
  });
}

}  // extern "C"
