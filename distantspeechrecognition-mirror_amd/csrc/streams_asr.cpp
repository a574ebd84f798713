// csrc/streams_asr.cpp -- the asr side of the streams: FeatureSpaceAdaptationFeature, the distribution set, decoding and lattice
// posteriors straight from a feature stream (see stream_op.h).
#include "stream_op.h"
#include "lattice.h"
#include "multistream.h"

extern "C" {

// ---------------------------------------------------------------------------------------------------------------------------------
// FeatureSpaceAdaptationFeature as a stream operator (asr/train/fsa.cc:247-280): every frame of the source under transform 0 of the adaptation
// handle, which exists from distribSet() on.  The frames stay on the device, so a distribution set built on this stream decodes adapted
// features without a host round trip.  A changed transform or shift shows after the next reset(), as every operator here recomputes then.
namespace { struct FsaOp : dsr_stream {
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
}; }

dsr_status dsr_fsa_feature_create(dsr_stream* src, int maxAccu, int maxTran, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "FeatureSpaceAdaptationFeature");
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (maxAccu < 1 || maxTran < 1) throw Error(DSR_E_PARAMETER, "%d accumulators, %d transformations", maxAccu, maxTran);
    auto s = new_op<FsaOp>(out, name, "FeatureSpaceAdaptationFeature", src->size_, DSR_T_FLOAT); s->maxAccu = maxAccu; s->maxTran = maxTran; hand_out(out, std::move(s), {src});
  });
}
dsr_status dsr_fsa_feature_distrib_set(dsr_stream* s, dsr_gmm* gmm)
{
  return guard([&] {
    FsaOp* q = as_op<FsaOp>(s, "not a FeatureSpaceAdaptationFeature stream"); if (!gmm) throw Error(DSR_E_PARAMETER, "null argument");
    if (q->size_ != dsr_gmm_dim(gmm)) throw Error(DSR_E_DIMENSION, "Feature and codebook dimensions (%d vs. %d) do not match.", q->size_, dsr_gmm_dim(gmm));
    dsr_fsa* h = nullptr; ok(dsr_fsa_create(gmm, q->maxAccu, q->maxTran, &h));
    dsr_fsa_destroy(q->h); q->h = h; q->ready = false;
  });
}
dsr_fsa* dsr_fsa_feature_handle(dsr_stream* s) { FsaOp* q = dynamic_cast<FsaOp*>(s); return q ? q->h : nullptr; }

// ---------------------------------------------------------------------------------------------------------------------------------
// STCTransformer / LDATransformer as stream operators (asr/adapt/transform.cc:1836-1850, 1937-1959): every frame of the source under matrix 0
// of the operator's handle, the first size() rows of it for LDA.  The handle is a bare transformer (the identity, or a loaded matrix) until a
// model is named; then it is an estimator that keeps the matrix.  The frames stay on the device, as FeatureSpaceAdaptationFeature's do.
namespace {
struct StcOp : dsr_stream {
  dsr_stc* h = nullptr; int cascade = 0, mmi = 0;
  ~StcOp() override { dsr_stc_destroy(h); }
  void compute() override { alloc(ups[0]->nFrames); ok(dsr_stc_apply(h, ups[0]->d<float>(), nFrames, 0, d<float>(), S0)); }
};
struct LdaOp : dsr_stream {
  dsr_lda* h = nullptr;
  ~LdaOp() override { dsr_lda_destroy(h); }
  void compute() override { alloc(ups[0]->nFrames); ok(dsr_lda_apply(h, ups[0]->d<float>(), nFrames, 0, size_, d<float>(), S0)); }
};
}

dsr_status dsr_stc_feature_create(dsr_stream* src, int cascade, int mmiEstimation, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "STCTransformer");
    auto s = new_op<StcOp>(out, name, "STC Transformer", src->size_, DSR_T_FLOAT); s->cascade = cascade; s->mmi = mmiEstimation;
    ok(dsr_stc_create_transformer(src->size_, &s->h));
    hand_out(out, std::move(s), {src});
  });
}
dsr_status dsr_stc_feature_distrib_set(dsr_stream* s, dsr_gmm* gmm)
{
  return guard([&] {
    StcOp* q = as_op<StcOp>(s, "not an STCTransformer stream"); if (!gmm) throw Error(DSR_E_PARAMETER, "null argument");
    if (q->size_ != dsr_gmm_dim(gmm)) throw Error(DSR_E_DIMENSION, "Feature and codebook dimensions (%d vs. %d) do not match.", q->size_, dsr_gmm_dim(gmm));
    std::vector<double> A((size_t) q->size_ * q->size_); ok(dsr_stc_get_transform(q->h, 0, A.data(), nullptr));
    dsr_stc* h = nullptr; ok(dsr_stc_create(gmm, 1, q->cascade, q->mmi, &h));
    const dsr_status st = dsr_stc_set_transform(h, 0, A.data()); if (st) { dsr_stc_destroy(h); ok(st); }
    dsr_stc_destroy(q->h); q->h = h; q->ready = false;
  });
}
dsr_stc* dsr_stc_feature_handle(dsr_stream* s) { StcOp* q = dynamic_cast<StcOp*>(s); return q ? q->h : nullptr; }

dsr_status dsr_lda_feature_create(dsr_stream* src, int outDim, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(src, DSR_T_FLOAT, "LDATransformer");
    if (outDim < 1 || outDim > src->size_) throw Error(DSR_E_DIMENSION, "LDA output size %d of a %d-dimensional source", outDim, src->size_);
    auto s = new_op<LdaOp>(out, name, "LDA Transformer", outDim, DSR_T_FLOAT);
    ok(dsr_lda_create_transformer(src->size_, &s->h));
    hand_out(out, std::move(s), {src});
  });
}
dsr_status dsr_lda_feature_codebooks(dsr_stream* s, dsr_gmm* gmm, dsr_gmm* global)
{
  return guard([&] {
    LdaOp* q = as_op<LdaOp>(s, "not an LDATransformer stream"); if (!gmm || !global) throw Error(DSR_E_PARAMETER, "null argument");
    const int Din = q->ups[0]->size_;
    if (Din != dsr_gmm_dim(gmm)) throw Error(DSR_E_DIMENSION, "Feature and codebook dimensions (%d vs. %d) do not match.", Din, dsr_gmm_dim(gmm));
    std::vector<double> L((size_t) Din * Din); ok(dsr_lda_get_transform(q->h, 0, L.data()));
    dsr_lda* h = nullptr; ok(dsr_lda_create(gmm, global, 1, &h));
    const dsr_status st = dsr_lda_set_transform(h, 0, L.data()); if (st) { dsr_lda_destroy(h); ok(st); }
    dsr_lda_destroy(q->h); q->h = h; q->ready = false;
  });
}
dsr_lda* dsr_lda_feature_handle(dsr_stream* s) { LdaOp* q = dynamic_cast<LdaOp*>(s); return q ? q->h : nullptr; }

// ---------------------------------------------------------------------------------------------------------------------------------
// ASR side of the boundary: the distribution set as the decoder sees it.  The reference decoder asks _dist->find(distX-1)->score(_frameX)
// (asr/decoder/decoder.h:985); Distrib::score -> CodebookBasic::score pulls frame frameX of the feature stream and caches the codebook's
// score for that frame (asr/gaussian/distribBasic.h:48-50,110-114, codebookBasic.cc:431-465).  Here a distribution set is a GMM model bound to
// a feature stream handle: score(distX, frameX) scores ALL distributions of that frame on the device at the first request and serves the rest
// of the frame's requests from the host copy; decode_stream() keeps everything on the device (features -> scores -> token passing), no host
// round trip.
// A multi-stream set (include/dsr.h section 8b; the struct is multistream.h's) has two such sets as children and asks both, then combines.
namespace {
void null_check(const void* d) { if (!d) throw Error(DSR_E_PARAMETER, "null argument"); }
const dsr_gmm* names_of(const dsr_distribset* d) { return d->ms ? d->audio->gmm : d->gmm; }
int ndists(const dsr_distribset* d) { return dsr_gmm_num_dists(names_of(d)); }
void reset_cache(dsr_distribset* d) { d->cachedFrame = -1; if (d->ms) { reset_cache(d->audio); reset_cache(d->video); } }
void reset_feature(dsr_distribset* d) { d->cachedFrame = -1; if (d->ms) { reset_feature(d->audio); reset_feature(d->video); } else d->feat->reset(); }
// every distribution's score of frame frameX in d->d_row, on the device: the frame is pulled through the stream protocol (jiterator_error at
// the end of the stream, jindex_error out of order) unless the row is the cached one
void frame_row(dsr_distribset* d, int frameX)
{
  if (frameX == d->cachedFrame && frameX >= 0) return;
  const int K = ndists(d);
  d->d_row.reserve((size_t) K); d->hostRow = false;
  if (d->ms) {
    frame_row(d->audio, frameX); frame_row(d->video, frameX);
    ms_combine(d->audio->d_row.p, d->video->d_row.p, d->ms->d_table.p, 1, d->ms->KA, d->ms->KV, d->ms->wA, d->ms->wV, d->d_row.p, S0);
    d->cachedFrame = d->audio->cachedFrame;
    return;
  }
  (void) d->feat->next(frameX);
  const int t = d->feat->frameX;
  const float* x = reinterpret_cast<const float*>(d->feat->dev.p) + (size_t) t * d->feat->size_;
  ok(dsr_gmm_score(d->gmm, x, 1, d->mode, d->d_row.p, nullptr, S0));
  d->cachedFrame = t;
}
// the score matrix [T][ndists] of the utterance the stream(s) hold, on the device: a multi-stream set scores T = min frames of each child in the
// child's own mode and combines in place in the audio child's matrix
const float* score_matrix(dsr_distribset* d, int* T)
{
  if (d->ms) {
    int Ta = 0, Tv = 0;
    const float* sA = score_matrix(d->audio, &Ta); const float* sV = score_matrix(d->video, &Tv);
    *T = Ta < Tv ? Ta : Tv;
    if (*T > 0) ms_combine(sA, sV, d->ms->d_table.p, *T, d->ms->KA, d->ms->KV, d->ms->wA, d->ms->wV, d->audio->d_scores.p, S0);
    return d->audio->d_scores.p;
  }
  d->feat->materialize();
  *T = d->feat->nFrames;
  if (*T > 0) {
    const int K = ndists(d);
    d->d_scores.reserve((size_t) *T * K);
    ok(dsr_gmm_score(d->gmm, reinterpret_cast<const float*>(d->feat->dev.p), (int64_t) *T, d->mode, d->d_scores.p, nullptr, S0));
  }
  return d->d_scores.p;
}
// the reference has pulled the stream(s) to the end
void at_end(dsr_distribset* d, int T)
{
  if (d->ms) { at_end(d->audio, T); at_end(d->video, T); return; }
  if (T > 0) d->feat->frameX = T - 1;
  d->feat->endOfSamples = true;
}
}  // namespace

dsr_status dsr_distribset_create(dsr_gmm* gmm, dsr_stream* feature, int gmmMode, dsr_distribset** out)
{
  return guard([&] {
    if (!gmm || !feature || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (feature->type != DSR_T_FLOAT) throw Error(DSR_E_TYPE, "the feature stream of a codebook set delivers float vectors");
    if (feature->size_ != dsr_gmm_dim(gmm)) throw Error(DSR_E_DIMENSION, "Feature and codebook dimensions (%d vs. %d) do not match.", feature->size_, dsr_gmm_dim(gmm));
    if (gmmMode < 0 || gmmMode > 2) throw Error(DSR_E_PARAMETER, "bad scoring mode %d", gmmMode);
    auto d = std::make_unique<dsr_distribset>(); d->gmm = gmm; d->feat = feature; d->mode = gmmMode; dsr_stream_retain(feature); *out = d.release();
  });
}
void dsr_distribset_destroy(dsr_distribset* d)
{
  if (!d || --d->refs > 0) return;
  if (d->ms) { dsr_ms_destroy(d->ms); dsr_distribset_destroy(d->audio); dsr_distribset_destroy(d->video); }
  else dsr_stream_release(d->feat);
  delete d;
}
int dsr_distribset_ndists(const dsr_distribset* d) { return d ? ndists(d) : 0; }
dsr_status dsr_distribset_find(const dsr_distribset* d, const char* name, int* distX)
{ if (!d) return guard([&] { throw Error(DSR_E_PARAMETER, "null argument"); }); return dsr_gmm_find_dist(names_of(d), name, distX); }
const char* dsr_distribset_name(const dsr_distribset* d, int distX) { return d ? dsr_gmm_dist_name(names_of(d), distX) : ""; }
dsr_status dsr_distribset_reset_cache(dsr_distribset* d) { return guard([&] { null_check(d); reset_cache(d); }); }      // codebookBasic.cc:414-420
dsr_status dsr_distribset_reset_feature(dsr_distribset* d) { return guard([&] { null_check(d); reset_feature(d); }); }
dsr_status dsr_distribset_score(dsr_distribset* d, int distX, int frameX, float* score)
{
  return guard([&] {
    if (!d || !score) throw Error(DSR_E_PARAMETER, "null argument");
    const int K = ndists(d);
    if (distX < 0 || distX >= K) throw Error(DSR_E_INDEX, "distribution %d of %d", distX, K);
    frame_row(d, frameX);
    if (!d->hostRow) {
      d->row.resize((size_t) K);
      DSR_HIP(hipMemcpy(d->row.data(), d->d_row.p, sizeof(float) * (size_t) K, hipMemcpyDeviceToHost));
      d->hostRow = true;
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
    reset_feature(d);
    int T = 0; const float* scores = score_matrix(d, &T); const int K = ndists(d);
    if (T <= 0) { at_end(d, 0); throw Error(DSR_E_ITERATOR, "end of samples!"); }
    d->d_T.upload(&T, 1);
    ok(dsr_decoder_decode_batch(dec, scores, d->d_T.p, 1, T, K, res, arcs_out, words_out, maxPath, S0));
    at_end(d, T);
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
    reset_cache(d);                                                          // dss->resetCache()
    L->ensure_ops(); L->sorted.clear();                                      // _clearSorted()
    const bool plain = !d->ms; if (plain) d->feat->materialize();
    int T = plain ? d->feat->nFrames : 0; const int K = ndists(d);
    const float* scores = plain ? nullptr : score_matrix(d, &T);             // a multi-stream set knows its frame count from the matrix
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
      if (plain) scores = score_matrix(d, &T);
      DevBuf<int> dd, ds, de; DevBuf<double> dout; dd.upload(dist); ds.upload(start); de.upload(end); dout.reserve(link.size());
      op_link_ac(scores, K, dd.p, ds.p, de.p, (int) link.size(), dout.p, S0);
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
