// csrc/fsa.cpp -- the host side of feature-space adaptation: the distribution mask, accumulator arithmetic, transforms and the files.
//
// Replaces FeatureSpaceAdaptationFeature::add / addAll (asr/train/fsa.cc:159-176, "fsa"), zeroAccu / scaleAccu / addAccu (fsa:435-465, 637-650),
// clear / compareTransform (fsa:467-503), saveAccu / loadAccu (fsa:505-583) and save / load (fsa:585-635).  Everything here is arithmetic over
// the host accumulators of csrc/fsa.h in the reference's order and precision.  Compiled with -ffp-contract=off.
#include "common.h"
#include "fsa.h"
#include "befile.h"
#include <cmath>

using namespace dsr;

namespace {

dsr_fsa& need(dsr_fsa* h) { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); return *h; }
const dsr_fsa& need(const dsr_fsa* h) { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); return *h; }

}  // namespace

extern "C" {

int dsr_fsa_dim(const dsr_fsa* h) { return h ? h->D : 0; }
int dsr_fsa_num_accus(const dsr_fsa* h) { return h ? h->nAccu : 0; }
int dsr_fsa_num_transforms(const dsr_fsa* h) { return h ? h->nTran : 0; }

dsr_status dsr_fsa_add(dsr_fsa* hp, int dsX)
{
  return guard([&] {
    dsr_fsa& h = need(hp);
    if (dsX < 0 || dsX >= h.K) throw Error(DSR_E_INDEX, "distribution %d of %d", dsX, h.K);      // DistribSet::find
    // fsa:165-167 compares the codebook's feature length with dimN (jdimension_error); every codebook of a dsr_gmm has the model's dimN
    h.on[dsX] = 1;
  });
}
dsr_status dsr_fsa_add_all(dsr_fsa* hp) { return guard([&] { dsr_fsa& h = need(hp); h.on.assign(h.K, 1); }); }

dsr_status dsr_fsa_set_top_n(dsr_fsa* hp, unsigned topN)
{
  return guard([&] {
    dsr_fsa& h = need(hp);
    if (topN > (unsigned) h.maxRef) throw Error(DSR_E_INDEX, "topN = %u beyond the %d Gaussians of the largest codebook", topN, h.maxRef);
    h.topN = topN;                                        // addCount is one-hot (codebookBasic.cc:431-554): the entries after the first add nothing
  });
}
unsigned dsr_fsa_top_n(const dsr_fsa* h) { return h ? h->topN : 0; }
dsr_status dsr_fsa_set_shift(dsr_fsa* hp, float shift) { return guard([&] { need(hp).shift = shift; }); }
float dsr_fsa_shift(const dsr_fsa* h) { return h ? h->shift : 0.0f; }

dsr_status dsr_fsa_upload_features(dsr_fsa* hp, const float* xScore_host, const float* xSrc_host, int64_t N, const float** xScore_dev, const float** xSrc_dev)
{
  return guard([&] {
    dsr_fsa& h = need(hp);
    if (!xScore_dev || !xSrc_dev || (N > 0 && (!xScore_host || !xSrc_host))) throw Error(DSR_E_PARAMETER, "null argument");
    if (N < 0) throw Error(DSR_E_PARAMETER, "negative frame count");
    h.d_featScore.reserve(1); h.d_featSrc.reserve(1);
    h.d_featScore.upload(xScore_host, (size_t) N * h.D); h.d_featSrc.upload(xSrc_host, (size_t) N * h.D);
    *xScore_dev = h.d_featScore.p; *xSrc_dev = h.d_featSrc.p;
  });
}

dsr_status dsr_fsa_count(const dsr_fsa* hp, int accuX, double* count)
{ return guard([&] { const dsr_fsa& h = need(hp); if (!count) throw Error(DSR_E_PARAMETER, "null argument"); h.check_accu(accuX, "FeatureSpaceAdaptationFeature::count"); *count = h.count[accuX]; }); }

dsr_status dsr_fsa_zero(dsr_fsa* hp, int accuX)
{
  return guard([&] {
    dsr_fsa& h = need(hp); h.check_accu(accuX, "FeatureSpaceAdaptationFeatureClearAccu");
    h.count[accuX] = 0.0; h.beta[accuX] = 0.0f;
    std::fill(h.z.begin() + (size_t) accuX * h.zsz(), h.z.begin() + (size_t) (accuX + 1) * h.zsz(), 0.0);
    std::fill(h.Gi.begin() + (size_t) accuX * h.gsz(), h.Gi.begin() + (size_t) (accuX + 1) * h.gsz(), 0.0);
  });
}

dsr_status dsr_fsa_scale(dsr_fsa* hp, float scale, int accuX)
{
  return guard([&] {
    dsr_fsa& h = need(hp); h.check_accu(accuX, "FeatureSpaceAdaptationFeatureClearAccu");
    h.count[accuX] *= scale; h.beta[accuX] *= scale;      // fsa:454-455
    double* z = h.z.data() + (size_t) accuX * h.zsz(); double* G = h.Gi.data() + (size_t) accuX * h.gsz();
    for (size_t e = 0; e < h.zsz(); e++) z[e] = z[e] * scale;
    for (size_t e = 0; e < h.gsz(); e++) G[e] = G[e] * scale;
  });
}

dsr_status dsr_fsa_add_accu(dsr_fsa* hp, int accuX, int accuY, float factor)
{
  return guard([&] {
    dsr_fsa& h = need(hp); h.check_accu(accuX, "FeatureSpaceAdaptationFeature::addAccu"); h.check_accu(accuY, "FeatureSpaceAdaptationFeature::addAccu");
    h.count[accuX] += factor * h.count[accuY];            // fsa:639-640: float x double, float x float
    h.beta[accuX] += factor * h.beta[accuY];
    double* z = h.z.data() + (size_t) accuX * h.zsz(); const double* zy = h.z.data() + (size_t) accuY * h.zsz();
    double* G = h.Gi.data() + (size_t) accuX * h.gsz(); const double* Gy = h.Gi.data() + (size_t) accuY * h.gsz();
    for (size_t e = 0; e < h.zsz(); e++) z[e] = z[e] + factor * zy[e];
    for (size_t e = 0; e < h.gsz(); e++) G[e] = G[e] + factor * Gy[e];
  });
}

dsr_status dsr_fsa_get_accu(const dsr_fsa* hp, int accuX, double* count, float* beta, double* z, double* G)
{
  return guard([&] {
    const dsr_fsa& h = need(hp); h.check_accu(accuX, "FeatureSpaceAdaptationFeature::getAccu");
    if (count) *count = h.count[accuX];
    if (beta) *beta = h.beta[accuX];
    if (z) std::copy(h.z.begin() + (size_t) accuX * h.zsz(), h.z.begin() + (size_t) (accuX + 1) * h.zsz(), z);
    if (G) std::copy(h.Gi.begin() + (size_t) accuX * h.gsz(), h.Gi.begin() + (size_t) (accuX + 1) * h.gsz(), G);
  });
}

dsr_status dsr_fsa_set_accu(dsr_fsa* hp, int accuX, const double* count, const float* beta, const double* z, const double* G)
{
  return guard([&] {
    dsr_fsa& h = need(hp); h.check_accu(accuX, "FeatureSpaceAdaptationFeature::setAccu");
    if (count) h.count[accuX] = *count;
    if (beta) h.beta[accuX] = *beta;
    if (z) std::copy(z, z + h.zsz(), h.z.begin() + (size_t) accuX * h.zsz());
    if (G) std::copy(G, G + h.gsz(), h.Gi.begin() + (size_t) accuX * h.gsz());
  });
}

dsr_status dsr_fsa_save_accu(const dsr_fsa* hp, const char* fileName, int accuX)
{
  return guard([&] {
    const dsr_fsa& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_accu(accuX, "FeatureSpaceAdaptationFeature::writeAccu");
    BEFile f(fileName, "wb");
    fwrite("SAS", 1, 3, f.fp); f.w32(h.D); f.wf((float) h.count[accuX]); f.wf(h.beta[accuX]);
    const double* z = h.z.data() + (size_t) accuX * h.zsz(); const double* G = h.Gi.data() + (size_t) accuX * h.gsz();
    for (size_t e = 0; e < h.zsz(); e++) f.wf((float) z[e]);
    for (size_t e = 0; e < h.gsz(); e++) f.wf((float) G[e]);                     // the upper triangle as it stands, fsa:527-530
  });
}

dsr_status dsr_fsa_load_accu(dsr_fsa* hp, const char* fileName, int accuX, float factor)
{
  return guard([&] {
    dsr_fsa& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_accu(accuX, "FeatureSpaceAdaptationFeature::readAccu");
    BEFile f(fileName, "rb");
    if (!f.magic("SAS")) throw Error(DSR_E_CONSISTENCY, "FeatureSpaceAdaptationFeature::readAccu: Couldn't find magic SAS in file %s.", fileName);
    const unsigned dimN = (unsigned) f.i32();
    if (dimN != (unsigned) h.D) throw Error(DSR_E_DIMENSION, "FeatureSpaceAdaptationFeature::readAccu: Dimension mismatch. Exptected dimN= %d, but got %d.", h.D, dimN);
    // read everything first: a short file leaves the accumulator as it was
    std::vector<float> v(2 + h.zsz() + h.gsz());
    for (size_t e = 0; e < v.size(); e++) v[e] = f.f32();
    h.count[accuX] += factor * v[0];                      // fsa:560: a float product
    h.beta[accuX] = (float) ((double) h.beta[accuX] + (double) factor * (double) v[1]);       // fsa:562
    double* z = h.z.data() + (size_t) accuX * h.zsz(); double* G = h.Gi.data() + (size_t) accuX * h.gsz();
    for (size_t e = 0; e < h.zsz(); e++) z[e] = z[e] + (double) factor * (double) v[2 + e];
    for (size_t e = 0; e < h.gsz(); e++) G[e] = G[e] + (double) factor * (double) v[2 + h.zsz() + e];
  });
}

int dsr_fsa_transform_status(const dsr_fsa* h, int tranX) { return (h && tranX >= 0 && tranX < h->nTran) ? h->status[tranX] : DSR_E_INDEX; }

dsr_status dsr_fsa_get_transform(const dsr_fsa* hp, int tranX, double* W)
{
  return guard([&] {
    const dsr_fsa& h = need(hp); if (!W) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_tran(tranX, "FeatureSpaceAdaptationFeature::getTransform");
    std::copy(h.W.begin() + (size_t) tranX * h.zsz(), h.W.begin() + (size_t) (tranX + 1) * h.zsz(), W);
  });
}

dsr_status dsr_fsa_set_transform(dsr_fsa* hp, int tranX, const double* W)
{
  return guard([&] {
    dsr_fsa& h = need(hp); if (!W) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_tran(tranX, "FeatureSpaceAdaptationFeature::setTransform");
    std::copy(W, W + h.zsz(), h.W.begin() + (size_t) tranX * h.zsz()); h.wDirty = true;
  });
}

dsr_status dsr_fsa_clear(dsr_fsa* hp, int tranX)
{
  return guard([&] {
    dsr_fsa& h = need(hp); h.check_tran(tranX, "FeatureSpaceAdaptationFeature::clear");
    double* W = h.W.data() + (size_t) tranX * h.zsz();
    for (int i = 0; i < h.D; i++) for (int j = 0; j <= h.D; j++) W[(size_t) i * (h.D + 1) + j] = (j == i + 1) ? 1.0 : 0.0;
    h.wDirty = true;
  });
}

dsr_status dsr_fsa_compare(const dsr_fsa* hp, int tranX, int tranY, float* out)
{
  return guard([&] {
    const dsr_fsa& h = need(hp); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_tran(tranX, "FeatureSpaceAdaptationFeature::compareTransform "); h.check_tran(tranY, "FeatureSpaceAdaptationFeature::compareTransform ");
    const double* X = h.W.data() + (size_t) tranX * h.zsz(); const double* Y = h.W.data() + (size_t) tranY * h.zsz();
    double sum = 0.0;                                     // fsa:494-500: columns 0 .. dimN - 1, the last column is left out as written
    for (int i = 0; i < h.D; i++) for (int j = 0; j < h.D; j++) { const double tmp = X[(size_t) i * (h.D + 1) + j] - Y[(size_t) i * (h.D + 1) + j]; sum += tmp * tmp; }
    *out = (float) sum;
  });
}

dsr_status dsr_fsa_save(const dsr_fsa* hp, const char* fileName, int tranX)
{
  return guard([&] {
    const dsr_fsa& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_tran(tranX, "FeatureSpaceAdaptationFeature::save");
    BEFile f(fileName, "wb");
    fwrite("SAW", 1, 3, f.fp); f.w32(h.D);
    const double* W = h.W.data() + (size_t) tranX * h.zsz();
    for (size_t e = 0; e < h.zsz(); e++) f.wf((float) W[e]);
  });
}

dsr_status dsr_fsa_load(dsr_fsa* hp, const char* fileName, int tranX)
{
  return guard([&] {
    dsr_fsa& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_tran(tranX, "FeatureSpaceAdaptationFeature::load");
    BEFile f(fileName, "rb");
    if (!f.magic("SAW")) throw Error(DSR_E_IO, "FeatureSpaceAdaptationFeature::load: Couldn't find magic SAW in file %s", fileName);
    const unsigned dimN = (unsigned) f.i32();
    if (dimN != (unsigned) h.D) throw Error(DSR_E_DIMENSION, "FeatureSpaceAdaptationFeature::load: Dimension mismatch. Expected dimN= %d but got %d.", h.D, dimN);
    std::vector<double> W(h.zsz());
    for (size_t e = 0; e < W.size(); e++) W[e] = (double) f.f32();
    std::copy(W.begin(), W.end(), h.W.begin() + (size_t) tranX * h.zsz()); h.wDirty = true;
  });
}

dsr_status dsr_fsa_set_timing(dsr_fsa* hp, int on) { return guard([&] { need(hp).timing = on != 0; }); }
dsr_status dsr_fsa_kernel_ms(const dsr_fsa* hp, float ms[5])
{ return guard([&] { const dsr_fsa& h = need(hp); if (!ms) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 5; i++) ms[i] = h.ms[i]; }); }

}  // extern "C"
