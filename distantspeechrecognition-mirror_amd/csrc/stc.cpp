// csrc/stc.cpp -- the host side of STC and LDA estimation: accumulator arithmetic, matrices and the files.
//
// Replaces STCEstimator::Accu::zero / save / load / increment (asr/train/estimateAdapt.cc:2511-2566, "eA"; estimateAdapt.h:681-697), transMatrix /
// save / load (eA:2318-2356), STCTransformer::save / load (asr/adapt/transform.cc:1852-1864, "tr"), LDAEstimator::Accu::zero / save / load
// (eA:2908-2980) and LDATransformer::save / load (tr:1961-1984).  Integers and floats of the accumulator files are big-endian (befile.h),
// matrices are raw native doubles as gsl_matrix_fwrite writes them.  Compiled with -ffp-contract=off.
#include "common.h"
#include "stc.h"
#include "stc_rows.h"
#include "befile.h"
#include <cmath>

using namespace dsr;

namespace {

template <class H> H& need(H* h) { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); return *h; }

// a bare transformer (dsr_*_create_transformer) has a matrix and no accumulators
template <class H> void need_accu(const H& h, const char* who) { if (!h.g) throw Error(DSR_E_CONSISTENCY, "%s: a transformer without a distribution set has no statistics", who); }

// copyUpperTriangle (eA:2658-2663, 2982-2987) of `count` matrices
void copy_up(double* M, int D, int count)
{
  for (int d = 0; d < count; d++) for (int i = 0; i < D; i++) for (int j = i + 1; j < D; j++) M[((size_t) d * D + i) * D + j] = M[((size_t) d * D + j) * D + i];
}

void wraw(BEFile& f, const double* p, size_t n) { if (fwrite(p, sizeof(double), n, f.fp) != n) throw Error(DSR_E_IO, "write failed"); }
void rraw(BEFile& f, double* p, size_t n) { if (fread(p, sizeof(double), n, f.fp) != n) throw Error(DSR_E_IO, "premature end of file"); }

// A^-1 by the device's own elimination (stc_rows.h) with one thread; false for a singular matrix
bool invert(const double* A, int D, double* Ai)
{
  std::vector<double> mem(StcWork::doubles(D, 1) + D); StcWork w; w.carve(mem.data(), D, 1);
  std::copy(A, A + (size_t) D * D, w.A);
  if (!stc_invert(w, D, 0, 1, [] {})) return false;
  for (size_t e = 0; e < (size_t) D * D; e++) if (!stc_finite(w.Ai[e])) return false;
  std::copy(w.Ai, w.Ai + (size_t) D * D, Ai);
  return true;
}

void set_matrix(dsr_stc& h, int estX, const double* A, const char* who)
{
  std::vector<double> Ai(h.msz());
  if (!invert(A, h.D, Ai.data())) throw Error(DSR_E_CONSISTENCY, "%s: the matrix has no inverse; the estimator keeps its own", who);
  std::copy(A, A + h.msz(), h.A.begin() + (size_t) estX * h.msz()); std::copy(Ai.begin(), Ai.end(), h.Ainv.begin() + (size_t) estX * h.msz());      // eA:2352-2355
  h.aDirty = true;
}

double log_abs_det(const double* A, int D)
{
  std::vector<double> a(A, A + (size_t) D * D); double sum = 0.0;
  for (int k = 0; k < D; k++) {
    int pr = k; for (int r = k + 1; r < D; r++) if (fabs(a[(size_t) r * D + k]) > fabs(a[(size_t) pr * D + k])) pr = r;
    if (pr != k) for (int c = 0; c < D; c++) std::swap(a[(size_t) k * D + c], a[(size_t) pr * D + c]);
    const double pv = a[(size_t) k * D + k]; sum += log(fabs(pv));
    for (int r = k + 1; r < D; r++) { const double f = a[(size_t) r * D + k] / pv; for (int c = k; c < D; c++) a[(size_t) r * D + c] -= f * a[(size_t) k * D + c]; }
  }
  return sum;
}

template <class H> void upload_features(H& h, const float* xScore_host, const float* xSrc_host, int64_t N, const float** xScore_dev, const float** xSrc_dev)
{
  if (!xScore_dev || !xSrc_dev || (N > 0 && (!xScore_host || !xSrc_host))) throw Error(DSR_E_PARAMETER, "null argument");
  if (N < 0) throw Error(DSR_E_PARAMETER, "negative frame count");
  h.d_featScore.reserve(1); h.d_featSrc.reserve(1);
  h.d_featScore.upload(xScore_host, (size_t) N * h.D); h.d_featSrc.upload(xSrc_host, (size_t) N * h.D);
  *xScore_dev = h.d_featScore.p; *xSrc_dev = h.d_featSrc.p;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------------------------------------------------------------- STC
int dsr_stc_dim(const dsr_stc* h) { return h ? h->D : 0; }
int dsr_stc_num_estimators(const dsr_stc* h) { return h ? h->nEst : 0; }

dsr_status dsr_stc_upload_features(dsr_stc* hp, const float* xScore_host, const float* xSrc_host, int64_t N, const float** xScore_dev, const float** xSrc_dev)
{ return guard([&] { upload_features(need(hp), xScore_host, xSrc_host, N, xScore_dev, xSrc_dev); }); }

dsr_status dsr_stc_increment(dsr_stc* hp, int estX, double totalPr, unsigned totalT)
{ return guard([&] { dsr_stc& h = need(hp); h.check_est(estX, "STCEstimator::increment"); need_accu(h, "STCEstimator::increment"); h.totalPr[estX] += totalPr; h.totalT[estX] += totalT; }); }

dsr_status dsr_stc_zero(dsr_stc* hp, int estX)
{
  return guard([&] {
    dsr_stc& h = need(hp); h.check_est(estX, "STCEstimator::zeroAccu"); need_accu(h, "STCEstimator::zeroAccu");
    h.count[estX] = h.denCount[estX] = h.totalPr[estX] = 0.0; h.totalT[estX] = 0;              // eA:2511-2519; _E is kept
    std::fill(h.sumOsq.begin() + (size_t) estX * h.ssz(), h.sumOsq.begin() + (size_t) (estX + 1) * h.ssz(), 0.0);
    std::fill(h.regSq.begin() + (size_t) estX * h.ssz(), h.regSq.begin() + (size_t) (estX + 1) * h.ssz(), 0.0);
  });
}

dsr_status dsr_stc_get_accu(dsr_stc* hp, int estX, int throughAccessor, double* count, double* denCount, double* totalPr, unsigned* totalT, double* sumOsq, double* regSq)
{
  return guard([&] {
    dsr_stc& h = need(hp); h.check_est(estX, "STCEstimator::getAccu"); need_accu(h, "STCEstimator::getAccu");
    if (throughAccessor) { copy_up(h.sumOsq.data() + (size_t) estX * h.ssz(), h.D, h.D); copy_up(h.regSq.data() + (size_t) estX * h.ssz(), h.D, h.D); }
    if (count) *count = h.count[estX];
    if (denCount) *denCount = h.denCount[estX];
    if (totalPr) *totalPr = h.totalPr[estX];
    if (totalT) *totalT = h.totalT[estX];
    if (sumOsq) std::copy(h.sumOsq.begin() + (size_t) estX * h.ssz(), h.sumOsq.begin() + (size_t) (estX + 1) * h.ssz(), sumOsq);
    if (regSq) std::copy(h.regSq.begin() + (size_t) estX * h.ssz(), h.regSq.begin() + (size_t) (estX + 1) * h.ssz(), regSq);
  });
}

dsr_status dsr_stc_set_accu(dsr_stc* hp, int estX, const double* count, const double* denCount, const double* totalPr, const unsigned* totalT, const double* sumOsq,
                            const double* regSq)
{
  return guard([&] {
    dsr_stc& h = need(hp); h.check_est(estX, "STCEstimator::setAccu"); need_accu(h, "STCEstimator::setAccu");
    if (count) h.count[estX] = *count;
    if (denCount) h.denCount[estX] = *denCount;
    if (totalPr) h.totalPr[estX] = *totalPr;
    if (totalT) h.totalT[estX] = *totalT;
    if (sumOsq) std::copy(sumOsq, sumOsq + h.ssz(), h.sumOsq.begin() + (size_t) estX * h.ssz());
    if (regSq) std::copy(regSq, regSq + h.ssz(), h.regSq.begin() + (size_t) estX * h.ssz());
  });
}

dsr_status dsr_stc_save_accu(dsr_stc* hp, const char* fileName, int estX)
{
  return guard([&] {
    dsr_stc& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_est(estX, "STCEstimator::saveAccu"); need_accu(h, "STCEstimator::saveAccu");
    double* S = h.sumOsq.data() + (size_t) estX * h.ssz(); double* R = h.regSq.data() + (size_t) estX * h.ssz();
    copy_up(S, h.D, h.D); copy_up(R, h.D, h.D);           // save reads through sumOsq() / regSq() (eA:2531-2535)
    BEFile f(fileName, "wb");
    f.w32(h.D); f.w32(1); f.wf((float) h.count[estX]); f.wf((float) h.denCount[estX]); f.wf((float) h.totalPr[estX]); f.w32((int) h.totalT[estX]);
    wraw(f, S, h.ssz()); wraw(f, R, h.ssz());
  });
}

dsr_status dsr_stc_load_accu(dsr_stc* hp, const char* fileName, int estX)
{
  return guard([&] {
    dsr_stc& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_est(estX, "STCEstimator::loadAccu"); need_accu(h, "STCEstimator::loadAccu");
    BEFile f(fileName, "rb");
    const unsigned sublen = (unsigned) f.i32();
    if (sublen != (unsigned) h.D) throw Error(DSR_E_DIMENSION, "Sub-feature lengths (%d vs. %d) do not match.", h.D, sublen);
    const unsigned nsub = (unsigned) f.i32();
    if (nsub != 1u) throw Error(DSR_E_DIMENSION, "Number of sub-features (%d vs. %d) do not match.", 1, nsub);
    // read everything first: a short file leaves the accumulator as it was
    const float c = f.f32(), dc = f.f32(), pr = f.f32(); const unsigned T = (unsigned) f.i32();
    std::vector<double> S(h.ssz()), R(h.ssz()); rraw(f, S.data(), S.size()); rraw(f, R.data(), R.size());
    h.count[estX] += c; h.denCount[estX] += dc; h.totalPr[estX] += pr; h.totalT[estX] += T;   // eA:2548-2552
    double* s = h.sumOsq.data() + (size_t) estX * h.ssz(); double* r = h.regSq.data() + (size_t) estX * h.ssz();
    for (size_t e = 0; e < h.ssz(); e++) { s[e] += S[e]; r[e] += R[e]; }
  });
}

int dsr_stc_status(const dsr_stc* h, int estX) { return (h && estX >= 0 && estX < h->nEst) ? h->status[estX] : DSR_E_INDEX; }
dsr_status dsr_stc_E(const dsr_stc* hp, int estX, double* E)
{ return guard([&] { const dsr_stc& h = need(hp); if (!E) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "STCEstimator::E"); *E = h.E[estX]; }); }

dsr_status dsr_stc_aux(const dsr_stc* hp, int estX, const double* A, double E, double* out)
{
  return guard([&] {
    const dsr_stc& h = need(hp); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    h.check_est(estX, "STCEstimator::calcAuxFunc"); need_accu(h, "STCEstimator::calcAuxFunc");
    const int D = h.D; if (!A) A = h.A.data() + (size_t) estX * h.msz();
    const double gamma = h.mmi ? h.denCount[estX] * E : h.count[estX];
    const double* S = h.sumOsq.data() + (size_t) estX * h.ssz(); const double* R = h.regSq.data() + (size_t) estX * h.ssz();
    double aux = 2.0 * gamma * log_abs_det(A, D);
    for (int d = 0; d < D; d++) for (int i = 0; i < D; i++) {
      double sum = 0.0;
      for (int j = 0; j < D; j++) { const size_t e = ((size_t) d * D + (i > j ? i : j)) * D + (i > j ? j : i); sum += A[(size_t) d * D + j] * (S[e] + E * R[e]); }
      aux -= A[(size_t) d * D + i] * sum;
    }
    *out = aux;
  });
}

dsr_status dsr_stc_get_transform(const dsr_stc* hp, int estX, double* A, double* Ainv)
{
  return guard([&] {
    const dsr_stc& h = need(hp); h.check_est(estX, "STCTransformer::matrix");
    if (A) std::copy(h.A.begin() + (size_t) estX * h.msz(), h.A.begin() + (size_t) (estX + 1) * h.msz(), A);
    if (Ainv) std::copy(h.Ainv.begin() + (size_t) estX * h.msz(), h.Ainv.begin() + (size_t) (estX + 1) * h.msz(), Ainv);
  });
}

dsr_status dsr_stc_set_transform(dsr_stc* hp, int estX, const double* A)
{ return guard([&] { dsr_stc& h = need(hp); if (!A) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "STCTransformer::matrix"); set_matrix(h, estX, A, "STCEstimator"); }); }

dsr_status dsr_stc_trans_matrix(const dsr_stc* hp, int estX, float* out)
{
  return guard([&] {
    const dsr_stc& h = need(hp); if (!out) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "STCEstimator::transMatrix");
    for (size_t e = 0; e < h.msz(); e++) out[e] = (float) h.A[(size_t) estX * h.msz() + e];      // eA:2318-2325
  });
}

dsr_status dsr_stc_save(const dsr_stc* hp, const char* fileName, int estX)
{
  return guard([&] {
    const dsr_stc& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "STCTransformer::save");
    BEFile f(fileName, "wb"); wraw(f, h.A.data() + (size_t) estX * h.msz(), h.msz());          // tr:1852-1857
  });
}

dsr_status dsr_stc_load(dsr_stc* hp, const char* fileName, int estX)
{
  return guard([&] {
    dsr_stc& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "STCEstimator::load");
    BEFile f(fileName, "rb"); std::vector<double> A(h.msz()); rraw(f, A.data(), A.size());
    set_matrix(h, estX, A.data(), "STCEstimator::load");
  });
}

dsr_status dsr_stc_save_float(const dsr_stc* hp, const char* fileName, int estX, const float* trans)
{
  return guard([&] {
    const dsr_stc& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "STCEstimator::save");
    const int D = h.D; std::vector<float> T(h.msz()), out(h.msz());
    for (size_t e = 0; e < h.msz(); e++) T[e] = (float) h.A[(size_t) estX * h.msz() + e];
    if (!trans) out = T;
    else for (int i = 0; i < D; i++) for (int j = 0; j < D; j++) {                              // gsl_blas_sgemm, eA:2338-2339: a float sum, k ascending
      float s = 0.0f;
      for (int k = 0; k < D; k++) s += T[(size_t) i * D + k] * trans[(size_t) k * D + j];
      out[(size_t) i * D + j] = s;
    }
    BEFile f(fileName, "wb"); if (fwrite(out.data(), sizeof(float), out.size(), f.fp) != out.size()) throw Error(DSR_E_IO, "write failed");
  });
}

dsr_status dsr_stc_set_timing(dsr_stc* hp, int on) { return guard([&] { need(hp).timing = on != 0; }); }
dsr_status dsr_stc_kernel_ms(const dsr_stc* hp, float ms[5])
{ return guard([&] { const dsr_stc& h = need(hp); if (!ms) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 5; i++) ms[i] = h.ms[i]; }); }

// ---------------------------------------------------------------------------------------------------------------------------------- LDA
int dsr_lda_dim(const dsr_lda* h) { return h ? h->D : 0; }
int dsr_lda_num_estimators(const dsr_lda* h) { return h ? h->nEst : 0; }

dsr_status dsr_lda_upload_features(dsr_lda* hp, const float* xScore_host, const float* xSrc_host, int64_t N, const float** xScore_dev, const float** xSrc_dev)
{ return guard([&] { upload_features(need(hp), xScore_host, xSrc_host, N, xScore_dev, xSrc_dev); }); }

dsr_status dsr_lda_zero(dsr_lda* hp, int estX)
{
  return guard([&] {
    dsr_lda& h = need(hp); h.check_est(estX, "LDAEstimator::zeroAccu"); need_accu(h, "LDAEstimator::zeroAccu");
    h.count[estX] = 0.0;
    for (std::vector<double>* M : { &h.within, &h.between, &h.mixture }) std::fill(M->begin() + (size_t) estX * h.msz(), M->begin() + (size_t) (estX + 1) * h.msz(), 0.0);
  });
}

dsr_status dsr_lda_get_accu(dsr_lda* hp, int estX, int throughAccessor, double* count, double* within, double* between, double* mixture)
{
  return guard([&] {
    dsr_lda& h = need(hp); h.check_est(estX, "LDAEstimator::getAccu"); need_accu(h, "LDAEstimator::getAccu");
    std::vector<double>* M[3] = { &h.within, &h.between, &h.mixture }; double* dst[3] = { within, between, mixture };
    if (count) *count = h.count[estX];
    for (int m = 0; m < 3; m++) {
      if (throughAccessor) copy_up(M[m]->data() + (size_t) estX * h.msz(), h.D, 1);
      if (dst[m]) std::copy(M[m]->begin() + (size_t) estX * h.msz(), M[m]->begin() + (size_t) (estX + 1) * h.msz(), dst[m]);
    }
  });
}

dsr_status dsr_lda_set_accu(dsr_lda* hp, int estX, const double* count, const double* within, const double* between, const double* mixture)
{
  return guard([&] {
    dsr_lda& h = need(hp); h.check_est(estX, "LDAEstimator::setAccu"); need_accu(h, "LDAEstimator::setAccu");
    std::vector<double>* M[3] = { &h.within, &h.between, &h.mixture }; const double* src[3] = { within, between, mixture };
    if (count) h.count[estX] = *count;
    for (int m = 0; m < 3; m++) if (src[m]) std::copy(src[m], src[m] + h.msz(), M[m]->begin() + (size_t) estX * h.msz());
  });
}

dsr_status dsr_lda_save_accu(dsr_lda* hp, const char* fileName, int estX)
{
  return guard([&] {
    dsr_lda& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "LDAEstimator::saveAccu"); need_accu(h, "LDAEstimator::saveAccu");
    BEFile f(fileName, "wb"); f.w32(h.D); f.w32(1);
    for (std::vector<double>* M : { &h.within, &h.between, &h.mixture }) { double* p = M->data() + (size_t) estX * h.msz(); copy_up(p, h.D, 1); wraw(f, p, h.msz()); }
    f.wf((float) h.count[estX]);                          // eA:2948
  });
}

dsr_status dsr_lda_load_accu(dsr_lda* hp, const char* fileName, int estX)
{
  return guard([&] {
    dsr_lda& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "LDAEstimator::loadAccu"); need_accu(h, "LDAEstimator::loadAccu");
    BEFile f(fileName, "rb");
    const unsigned sublen = (unsigned) f.i32();
    if (sublen != (unsigned) h.D) throw Error(DSR_E_DIMENSION, "Sub-feature lengths (%d vs. %d) do not match.", h.D, sublen);
    const unsigned nsub = (unsigned) f.i32();
    if (nsub != 1u) throw Error(DSR_E_DIMENSION, "Number of sub-features (%d vs. %d) do not match.", 1, nsub);
    std::vector<double> in(3 * h.msz()); rraw(f, in.data(), in.size()); const float c = f.f32();
    std::vector<double>* M[3] = { &h.within, &h.between, &h.mixture };
    for (int m = 0; m < 3; m++) { double* p = M[m]->data() + (size_t) estX * h.msz(); for (size_t e = 0; e < h.msz(); e++) p[e] += in[m * h.msz() + e]; }
    h.count[estX] += c;                                   // eA:2977
  });
}

int dsr_lda_status(const dsr_lda* h, int estX) { return (h && estX >= 0 && estX < h->nEst) ? h->status[estX] : DSR_E_INDEX; }

dsr_status dsr_lda_eigenvalues(const dsr_lda* hp, int estX, double* withinEv, double* betweenEv)
{
  return guard([&] {
    const dsr_lda& h = need(hp); h.check_est(estX, "LDAEstimator::eigenvalues");
    const double* ev = h.ev.data() + (size_t) estX * 2 * h.D;
    if (withinEv) std::copy(ev, ev + h.D, withinEv);
    if (betweenEv) std::copy(ev + h.D, ev + 2 * h.D, betweenEv);
  });
}

dsr_status dsr_lda_get_transform(const dsr_lda* hp, int estX, double* L)
{
  return guard([&] {
    const dsr_lda& h = need(hp); if (!L) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "LDATransformer::matrix");
    std::copy(h.L.begin() + (size_t) estX * h.msz(), h.L.begin() + (size_t) (estX + 1) * h.msz(), L);
  });
}

dsr_status dsr_lda_set_transform(dsr_lda* hp, int estX, const double* L)
{
  return guard([&] {
    dsr_lda& h = need(hp); if (!L) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "LDATransformer::matrix");
    std::copy(L, L + h.msz(), h.L.begin() + (size_t) estX * h.msz()); h.lDirty = true;
  });
}

dsr_status dsr_lda_save(const dsr_lda* hp, const char* fileName, int estX)
{
  return guard([&] {
    const dsr_lda& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "LDATransformer::save");
    std::vector<float> T(h.msz());                        // float32, the reference's "HACK" (tr:1967-1973); load reads float64
    for (size_t e = 0; e < h.msz(); e++) T[e] = (float) h.L[(size_t) estX * h.msz() + e];
    BEFile f(fileName, "wb"); if (fwrite(T.data(), sizeof(float), T.size(), f.fp) != T.size()) throw Error(DSR_E_IO, "write failed");
  });
}

dsr_status dsr_lda_load(dsr_lda* hp, const char* fileName, int estX)
{
  return guard([&] {
    dsr_lda& h = need(hp); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); h.check_est(estX, "LDATransformer::load");
    BEFile f(fileName, "rb"); std::vector<double> L(h.msz()); rraw(f, L.data(), L.size());      // tr:1979-1984
    std::copy(L.begin(), L.end(), h.L.begin() + (size_t) estX * h.msz()); h.lDirty = true;
  });
}

dsr_status dsr_lda_set_timing(dsr_lda* hp, int on) { return guard([&] { need(hp).timing = on != 0; }); }
dsr_status dsr_lda_kernel_ms(const dsr_lda* hp, float ms[5])
{ return guard([&] { const dsr_lda& h = need(hp); if (!ms) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 5; i++) ms[i] = h.ms[i]; }); }

}  // extern "C"
