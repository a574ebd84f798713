// csrc/stream_op.h -- the stream/feature-operator API (include/dsr.h section 7): what its translation units share.
//
// Mirrors FeatureStream<Type,item_type> (btk/stream/stream.h:36-75): reference-counted operators that
// hold their upstream(s), `next(frameX)` / `reset()` / `size()` / `name()` / `current()` / `isEnd()`,
// `frameX == -5` meaning "next", FrameResetX = -1, end of stream signalled as JITERATOR.
//
// The reference pulls one frame at a time through virtual calls; here an operator materialises its whole
// utterance on the device at the first next() after a reset() (every source of the path holds the full
// utterance in memory: SampleFeature::_samples, feature.cc:300-340) and then serves rows of its own
// host-side output buffer.  Compute always runs on the GPU (k_ops.hip / k_filterbank.hip / k_beamform.hip, reached through the entries of
// capi.cpp, filterbank.cpp and beamformer.cpp).
//
// One file per reference module, as dsr/btk/*.py and dsr/asr/*.py; an operator's struct is local to its file and followed by its entry points:
//   streams.cpp               retain/release/size/type/name/next/current/reset, SampleFeature (with the RIFF reader), the frame source
//   streams_feature.cpp       btk/feature and btk/lpc (pre-emphasis ... merge, the scalar operators, CMN, adjacent, linear transform, storage,
//                             LPC/MVDR/WTMVDR, spectral smoothing) and btk/convolution
//   streams_modulated.cpp     the five filter-bank operators and their bases
//   streams_beamformer.cpp    subband beamformers, SubbandMMI, the SRP DOA estimators, spherical beamformers, trackers, plane waves, orthogonalizer
//   streams_localization.cpp  CCTDE, MCC
//   streams_postfilter.cpp    Zelinski/McCowan/Lefkimmiatis, high-pass, spectral subtraction, Wiener, binary masks, threshold estimators
//   streams_enhance.cpp       echo cancellation (cancelVP), WPE (dereverberation)
//   streams_sad.cpp           VAD metrics, hangover segmenters, spectral-shape features
//   streams_asr.cpp           feature-space adaptation, the distribution set, decode_stream, gammaProbsDist
#pragma once
#include "common.h"
#include "ops.h"
#include <cmath>
#include <initializer_list>

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

constexpr hipStream_t S0 = nullptr;   // the null stream: every operator computes on it

struct SampleSrc : dsr_stream {      // SampleFeature (feature.cc:222-689)
  int blockLen, shiftLen, padZeros; std::vector<float> samples; DevBuf<float> dx; int sampleRate = 16000, nChan = 1;
  void compute() override {
    const int n = (int) samples.size(); int T;
    if (padZeros) T = (n + shiftLen - 1) / shiftLen; else { long a = (long) n - blockLen; T = a > 0 ? (int) ((a + shiftLen - 1) / shiftLen) : 0; }
    dx.upload(samples.data(), samples.size() ? samples.size() : 0); if (!dx.p) dx.reserve(1);
    alloc(T); op_frames(dx.p, n, T, blockLen, shiftLen, d<float>(), S0);
  }
};
namespace {
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
dsr_stream* need(dsr_stream* s, int type, const char* what) {
  if (!s) throw Error(DSR_E_PARAMETER, "null upstream for %s", what);
  if (s->type != type) throw Error(DSR_E_TYPE, "%s needs an upstream of element type %d, got %d", what, type, s->type);
  return s;
}

// The one way to make, find and hand out an operator.  A create function checks its arguments, makes the operator with new_op (which refuses a
// null `out` before anything is allocated), fills it -- a plan the operator owns is created into its member, so the destructor frees it when
// a later step throws -- and ends with hand_out, which takes the upstreams and gives the caller its reference.
template <class Op> std::unique_ptr<Op> new_op(dsr_stream** out, const char* name, const char* dflt, int size, int type)
{
  if (!out) throw Error(DSR_E_PARAMETER, "null argument");
  std::unique_ptr<Op> s(new Op()); s->name = (name && *name) ? name : dflt; s->size_ = size; s->type = type;
  return s;
}
template <class Op> void hand_out(dsr_stream** out, std::unique_ptr<Op> s, std::initializer_list<dsr_stream*> ups = {})
{
  for (dsr_stream* u : ups) s->add_up(u);
  *out = s.release();
}
// a stream handle as the operator Op, or the refusal `text`; argsOk folds in an argument check that shares the refusal
template <class Op, class S> Op* as_op(S* s, const char* text, bool argsOk = true, dsr_status refusal = DSR_E_PARAMETER)
{
  Op* q = dynamic_cast<Op*>(s);
  if (!q || !argsOk) throw Error(refusal, "%s", text);
  return q;
}
}  // namespace
