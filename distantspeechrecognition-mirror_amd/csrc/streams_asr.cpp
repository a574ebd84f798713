// csrc/streams_asr.cpp -- the asr side of the streams: FeatureSpaceAdaptationFeature, the distribution set, decoding and lattice
// posteriors straight from a feature stream (see stream_op.h).
#include "stream_op.h"
#include "lattice.h"

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
struct dsr_distribset { dsr_gmm* gmm = nullptr; dsr_stream* feat = nullptr; int mode = 0; int cachedFrame = -1; std::vector<float> row; DevBuf<float> d_row, d_scores; DevBuf<int> d_T; };

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
