// csrc/streams.cpp -- what every stream handle answers, and the two sources: SampleFeature and the frame source (see stream_op.h).
#include "stream_op.h"

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
    auto s = new_op<SampleSrc>(out, name, "Sample", blockLen, DSR_T_FLOAT); s->blockLen = blockLen; s->shiftLen = shiftLen; s->padZeros = padZeros;
    s->checkOrder = true; hand_out(out, std::move(s));
  });
}
dsr_status dsr_sample_feature_set_samples(dsr_stream* s, const float* samples, size_t n, unsigned sampleRate)
{
  return guard([&] {
    SampleSrc* q = as_op<SampleSrc>(s, "not a SampleFeature", samples || !n);
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
    SampleSrc* q = as_op<SampleSrc>(s, "not a SampleFeature", fn != nullptr);
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
    const SampleSrc* q = as_op<const SampleSrc>(s, "not a SampleFeature", data && n);
    *data = q->samples.data(); *n = q->samples.size();
  });
}
namespace { struct FrameSrc : dsr_stream {       // PyFeatureStream-like source: the caller hands over all frames (pyStream.h:44-130)
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
}; }

dsr_status dsr_frame_source_create(int type, int size, const char* name, dsr_stream** out)
{
  return guard([&] {
    if (!out || size < 1 || type < 0 || type > DSR_T_COMPLEX) throw Error(DSR_E_PARAMETER, "bad argument");
    auto s = new_op<FrameSrc>(out, name, "PyFeatureStream", size, type); s->checkOrder = false; hand_out(out, std::move(s));
  });
}
dsr_status dsr_frame_source_set_frames(dsr_stream* s, const void* data, size_t nframes)
{
  return guard([&] {
    FrameSrc* q = as_op<FrameSrc>(s, "not a frame source", data || !nframes);
    q->frames.assign((const unsigned char*) data, (const unsigned char*) data + nframes * q->rowBytes()); q->T = (int) nframes;
    const bool f = q->filling; q->filling = true; q->reset(); q->filling = f; q->stale = false;          // fresh frames: nothing to refill
  });
}
dsr_status dsr_frame_source_set_refill(dsr_stream* s, int (*refill)(void*), void* user)
{ return guard([&] { FrameSrc* q = as_op<FrameSrc>(s, "not a frame source"); q->refill = refill; q->refillUser = user; }); }

}  // extern "C"
