// csrc/beamformer.cpp -- the host side of the subband beamformers (dsr_bf_*): weight design, the RLS set-up and the C entries.  The kernels
// and their launchers: csrc/k_beamform.hip, reached through csrc/beamformer.h.
//
// Weight design is set-up work exactly as in the reference (done once per array geometry):
//   beamformerWeights::calcMainlobe              btk/beamformer/beamformer.cc:531-594
//   SubbandMVDR::setDiffuseNoiseModel            :2486-2553      divideNonDiagonalElements  beamformer.h:362-378
//   SubbandMVDR::setAllLevelsOfDiagonalLoading   :2555-2567      setNoiseSpatialSpectralMatrix :2454-2477
//   pseudoinverse (complex<float> SVD)           :253-305        calcMVDRWeights :2392-2446
//   _calcBlockingMatrix                          :398-479        calcSidelobeCancellerP_f :761-783
#include "beamformer.h"
#include "dev_math.h"
#include "svd_linpack.h"
#include "gsc_weights.h"
#include <complex>
#include <cmath>

namespace dsr {

// beamformer.cc:253-305: the reference's pseudo-inverse runs LINPACK's csvdc in complex<float>; svd_linpack.cpp restates that routine
// operation for operation (pinned against the reference's own csvdc: tests/golden/linpack_csvdc.npz).  A, invA row-major n x n.  Returns
// false when a singular value fell below the threshold (the caller then uses identity, :2425-2427).
static bool pseudoinverse_cf(const zc* A, zc* invA, int n, float thr) { return linpack::pseudoinverse(A, invA, n, n, thr); }

static double sinc_pi(double x) { return std::fabs(x) < 1e-300 ? 1.0 : std::sin(M_PI * x) / (M_PI * x); }   // gsl_sf_sinc

static void calc_mainlobe(BfState& s, double fs, const double* delays)
{
  const int M = s.M, C = s.C, M2 = M / 2;
  s.wq.assign((size_t) M * C, zc(0, 0));
  if (s.halfBandShift) {                                   // beamformer.cc:544-555
    const float fshift = 0.5f;
    for (int f = 0; f < M2; f++)
      for (int c = 0; c < C; c++) {
        const double val = -2.0 * M_PI * (fshift + f) * fs * delays[c] / M;
        s.wq[(size_t) f * C + c] = std::polar(1.0, val) / (double) C;
        s.wq[(size_t) (M - 1 - f) * C + c] = std::polar(1.0, -val) / (double) C;
      }
  } else {                                                  // :557-581
    for (int c = 0; c < C; c++) s.wq[c] = std::polar(1.0, 0.0) / (double) C;
    for (int f = 1; f < M2; f++)
      for (int c = 0; c < C; c++) {
        const double val = -2.0 * M_PI * f * delays[c] * fs / M;
        s.wq[(size_t) f * C + c] = std::polar(1.0, val) / (double) C;
        s.wq[(size_t) (M - f) * C + c] = std::polar(1.0, -val) / (double) C;
      }
    for (int c = 0; c < C; c++) { const double val = -M_PI * fs * delays[c]; s.wq[(size_t) M2 * C + c] = std::polar(1.0, val) / (double) C; }
  }
  s.haveWq = true; s.dirty = true;
}

static void blocking_matrix(const zc* d, int C, zc* B) { blocking_matrix_nc(d, C, 1, B); }   // NC = 1, beamformer.cc:398-479 (csrc/gsc_weights.h)

static void update_wl(BfState& s, int f)          // calcSidelobeCancellerP_f / U_f: wl = B wa (beamformer.cc:761-799)
{
  const int C = s.C, bs = C - 1;
  if (s.wl.size() != (size_t) s.M * C) s.wl.assign((size_t) s.M * C, zc(0, 0));
  sidelobe_wl(&s.B[(size_t) f * C * bs], &s.wa[(size_t) f * bs], C, bs, &s.wl[(size_t) f * C]);
}

static void refresh_effective(BfState& s)
{
  const int M = s.M, C = s.C;
  // halfBandShift == true: every one of the M bins is computed on its own -- no mirror, no special bin 0 (SubbandDS::next beamformer.cc:1159-1175,
  // SubbandGSC::next :1321-1330); the snapshots then carry all M bins, [U][C][Tmax][M].  SubbandMVDR refuses the flag at construction (:2324-2327).
  const int F = s.halfBandShift ? M : M / 2 + 1;
  if (s.halfBandShift && (s.mode == 1 || s.mode == 4)) throw Error(DSR_E_ALLOCATION, "halfBandShift==true is not yet supported");
  s.eff.assign((size_t) F * C, zc(0, 0));
  if (s.mode == 0) {
    if (!s.haveWq) throw Error(DSR_E_ERROR, "call calcArrayManifoldVectorsX() once");          // beamformer.cc:1140-1143
    for (int f = 0; f < F; f++) for (int c = 0; c < C; c++) s.eff[(size_t) f * C + c] = s.wq[(size_t) f * C + c];
  } else if (s.mode == 1) {
    if (!s.haveMvdr) throw Error(DSR_E_ERROR, "call calcMVDRWeights() once");                    // :2591-2594
    s.eff = s.mvdr;
  } else if (s.mode == 4) {                                                                        // SubbandMVDRGSC::next (beamformer.cc:2764-2817)
    if (!s.haveB) throw Error(DSR_E_ERROR, "call calcArrayManifoldVectorsX() once");
    if (!s.haveMvdr) throw Error(DSR_E_ERROR, "call calcMVDRWeights() once");
    for (int c = 0; c < C; c++) s.eff[c] = s.mvdr[c];
    for (int f = 1; f < F; f++) for (int i = 0; i < C; i++) s.eff[(size_t) f * C + i] = s.mvdr[(size_t) f * C + i] - s.wl[(size_t) f * C + i];
  } else {
    if (!s.haveWq || !s.haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");          // :1310-1313
    const int bs = C - 1;
    if (!s.halfBandShift) for (int c = 0; c < C; c++) s.eff[c] = s.wq[c];                       // bin 0: wq only (:1335-1338)
    for (int f = s.halfBandShift ? 0 : 1; f < F; f++) {
      double nrm = 0;
      for (int i = 0; i < C; i++) {
        zc wl(0, 0); for (int j = 0; j < bs; j++) wl += s.B[((size_t) f * C + i) * bs + j] * s.wa[(size_t) f * bs + j];
        const zc w = s.wq[(size_t) f * C + i] - wl; s.eff[(size_t) f * C + i] = w; nrm += std::norm(w);
      }
      if (s.mode == 3) { nrm = std::sqrt(nrm); for (int i = 0; i < C; i++) s.eff[(size_t) f * C + i] /= (nrm * C); }   // :1272-1281
    }
  }
  std::vector<float2> w((size_t) F * C);
  for (size_t i = 0; i < w.size(); i++) w[i] = make_float2((float) s.eff[i].real(), (float) s.eff[i].imag());
  s.d_w.upload(w);
  if (!s.halfBandShift) {
    std::vector<float2> wT((size_t) C * (F + 1), make_float2(0.f, 0.f));
    for (int f = 0; f < F; f++) for (int c = 0; c < C; c++) wT[(size_t) c * (F + 1) + f] = w[(size_t) f * C + c];
    s.d_wT.upload(wT);
  }
  s.dirty = false;
}

// what other units read of a beamformer (csrc/beamformer.h)
bool bf_has_fixed_weights(const dsr_bf* s) { return s && !s->rlsOn && !s->halfBandShift; }
const float2* bf_fixed_weights_dev(dsr_bf* s) { if (!bf_has_fixed_weights(s)) return nullptr; if (s->dirty) refresh_effective(*s); return s->d_wT.p; }
bool bf_gsc_fixed_weights(const dsr_bf* s, int* M, int* C, int* halfBandShift, const zc** wq, const zc** B)
{ if (!s || !s->haveWq || !s->haveB) return false; *M = s->M; *C = s->C; *halfBandShift = s->halfBandShift; *wq = s->wq.data(); *B = s->B.data(); return true; }

}  // namespace dsr

using namespace dsr;

static void gsc_rls_apply(BfState& s, const float* X, const int32_t* nframes, int U, int Tmax, float* Y, double* waOut, hipStream_t st)
{
  if (!s.haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");                                                    // beamformer.cc:1562-1565
  if (!s.haveP0) throw Error(DSR_E_ERROR, "set the precision matrix with initPrecisionMatrix() or setPrecisionMatrix()");   // :1566-1569
  if (s.halfBandShift) throw Error(DSR_E_ERROR, "not yet implemented");                                                     // :1580-1583
  if (s.C > 64) throw Error(DSR_E_DIMENSION, "SubbandGSCRLS: at most 64 channels (%d)", s.C);
  if (U <= 0 || Tmax <= 0) return;
  const int C = s.C, n = C - 1, F = s.M / 2 + 1;
  if (s.rlsDirty || s.dirty) {
    std::vector<double2> a((size_t) F * C), b((size_t) F * C * n), p((size_t) F * n * n);
    for (size_t i = 0; i < a.size(); i++) a[i] = make_double2(s.wq[i].real(), s.wq[i].imag());
    for (size_t i = 0; i < b.size(); i++) b[i] = make_double2(s.B[i].real(), s.B[i].imag());
    for (size_t i = 0; i < p.size(); i++) p[i] = make_double2(s.rlsP0[i].real(), s.rlsP0[i].imag());
    s.d_wq.upload(a); s.d_B.upload(b); s.d_P0.upload(p); s.d_diag.upload(s.rlsDiag); s.rlsDirty = false;
  }
  bf_launch_rls(s, X, nframes, U, Tmax, Y, waOut, st);
}

extern "C" {

dsr_status dsr_bf_create(int fftLen, int chanN, int halfBandShift, dsr_bf** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftLen < 2 || (fftLen & 1) || chanN < 1) throw Error(DSR_E_DIMENSION, "bad fftLen=%d chanN=%d", fftLen, chanN);
    dsr_bf* s = new dsr_bf(); s->M = fftLen; s->C = chanN; s->halfBandShift = halfBandShift; *out = s;
  });
}
void dsr_bf_destroy(dsr_bf* s) { delete s; }
int dsr_bf_fft_len(const dsr_bf* s) { return s->M; }
int dsr_bf_chan_n(const dsr_bf* s) { return s->C; }
int dsr_bf_half_band_shift(const dsr_bf* s) { return s->halfBandShift ? 1 : 0; }
int dsr_bf_is_adaptive(const dsr_bf* s) { return (s && s->rlsOn) ? 1 : 0; }
int dsr_bf_bins(const dsr_bf* s) { return s->halfBandShift ? s->M : s->M / 2 + 1; }

dsr_status dsr_bf_calc_array_manifold(dsr_bf* s, double fs, const double* delays)
{ return guard([&] { if (!s || !delays) throw Error(DSR_E_PARAMETER, "null argument"); calc_mainlobe(*s, fs, delays); }); }

dsr_status dsr_calc_delays_polar2(float azimuth, float elevation, const double* micPos, int C, double* delays)
{
  return guard([&] {
    if (!micPos || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    // superdirectiveBeamformer.cc:118-137 -- float arithmetic, float sin/cos overloads, mm/s
    const float c_x = -sinf(elevation) * cosf(azimuth), c_y = -sinf(elevation) * sinf(azimuth), c_z = -cosf(elevation);
    for (int i = 0; i < C; i++) {
      const float x = (float) micPos[3 * i], y = (float) micPos[3 * i + 1], z = (float) micPos[3 * i + 2];
      const float t = (c_x * x + c_y * y + c_z * z) / 343740.0;
      delays[i] = t;
    }
  });
}

dsr_status dsr_bf_set_diffuse_noise_model(dsr_bf* s, const double* mp, double fs, double sspeed)
{
  return guard([&] {
    if (!s || !mp) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = s->C, M = s->M, F = M / 2 + 1;
    std::vector<double> dm((size_t) C * C, 0.0);
    for (int m = 0; m < C; m++) for (int n = 0; n < m; n++) {
      const double dx = mp[3*m] - mp[3*n], dy = mp[3*m+1] - mp[3*n+1], dz = mp[3*m+2] - mp[3*n+2];
      dm[(size_t) m * C + n] = std::sqrt(dx * dx + dy * dy + dz * dz);
    }
    s->R.assign((size_t) F * C * C, zc(0, 0));
    for (int f = 0; f < F; f++) {
      const double odc = 2.0 * fs * f / (M * sspeed);
      zc* Rf = &s->R[(size_t) f * C * C];
      for (int m = 0; m < C; m++) for (int n = 0; n < m; n++) Rf[(size_t) m * C + n] = zc(sinc_pi(odc * dm[(size_t) m * C + n]), 0.0);
      for (int m = 0; m < C; m++) Rf[(size_t) m * C + m] = zc(1.0, 0.0);
      for (int m = 0; m < C; m++) for (int n = m + 1; n < C; n++) Rf[(size_t) m * C + n] = Rf[(size_t) n * C + m];
    }
    s->haveR = true;
  });
}
dsr_status dsr_bf_divide_nondiagonal(dsr_bf* s, float myu)
{
  return guard([&] {
    if (!s || !s->haveR) throw Error(DSR_E_ERROR, "Construct first a noise covariance matrix");
    const int C = s->C, F = s->M / 2 + 1;
    for (int f = 0; f < F; f++) for (int x = 0; x < C; x++) for (int y = 0; y < C; y++)
      if (x != y) s->R[((size_t) f * C + x) * C + y] /= zc(1.0 + myu, 0.0);
  });
}
dsr_status dsr_bf_diagonal_loading(dsr_bf* s, float w)
{
  return guard([&] {
    if (!s || !s->haveR) throw Error(DSR_E_ERROR, "Construct first a noise covariance matrix");
    const int C = s->C, F = s->M / 2 + 1;
    for (int f = 0; f < F; f++) for (int c = 0; c < C; c++) s->R[((size_t) f * C + c) * C + c] += (double) w;
  });
}
dsr_status dsr_bf_set_noise_matrix(dsr_bf* s, int f, const double* Rnn)
{
  return guard([&] {
    if (!s || !Rnn) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = s->C, F = s->M / 2 + 1;
    if (f < 0 || f >= F) throw Error(DSR_E_INDEX, "frequency bin %d out of range", f);
    if (!s->haveR) { s->R.assign((size_t) F * C * C, zc(0, 0)); s->haveR = true; }
    for (int i = 0; i < C * C; i++) s->R[(size_t) f * C * C + i] = zc(Rnn[2 * i], Rnn[2 * i + 1]);
  });
}
// pseudoinverse(A, invA, dThreshold) (beamformer.cc:253-305) by itself: host-side, no device needed
dsr_status dsr_pseudoinverse(const double* A, int rows, int cols, float dThreshold, double* invA, int* ok, float* svals)
{
  return guard([&] {
    if (!A || !invA || rows < 1 || cols < 1) throw Error(DSR_E_PARAMETER, "bad argument");
    const bool r = linpack::pseudoinverse(reinterpret_cast<const zc*>(A), reinterpret_cast<zc*>(invA), rows, cols, dThreshold, svals);
    if (ok) *ok = r ? 1 : 0;
  });
}
dsr_status dsr_bf_calc_mvdr_weights(dsr_bf* s, double fs, double thr)
{
  (void) fs;
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveR) throw Error(DSR_E_ALLOCATION, "Set a spatial spectral matrix before calling calcMVDRWeights()");
    if (!s->haveWq) throw Error(DSR_E_ERROR, "call calcArrayManifoldVectorsX() once");
    const int C = s->C, F = s->M / 2 + 1;
    s->mvdr.assign((size_t) F * C, zc(0, 0));
    std::vector<zc> invR((size_t) C * C), tmpH(C);
    for (int c = 0; c < C; c++) s->mvdr[c] = zc(1.0, 0.0);                          // :2413-2415
    for (int f = 1; f < F; f++) {
      const zc* d = &s->wq[(size_t) f * C];
      if (!pseudoinverse_cf(&s->R[(size_t) f * C * C], invR.data(), C, (float) thr)) {
        for (int i = 0; i < C * C; i++) invR[i] = zc(0, 0);
        for (int c = 0; c < C; c++) invR[(size_t) c * C + c] = zc(1, 0);
      }
      for (int i = 0; i < C; i++) { zc acc(0, 0); for (int j = 0; j < C; j++) acc += std::conj(invR[(size_t) j * C + i]) * d[j]; tmpH[i] = acc; }
      zc Lambda(0, 0); for (int i = 0; i < C; i++) Lambda += std::conj(tmpH[i]) * d[i];
      const zc norm = Lambda * (double) C;
      for (int c = 0; c < C; c++) {
        const double2 q = gsl_div(make_double2(tmpH[c].real(), tmpH[c].imag()), make_double2(norm.real(), norm.imag()));
        s->mvdr[(size_t) f * C + c] = zc(q.x, q.y);
      }
    }
    s->haveMvdr = true; s->dirty = true;
  });
}
dsr_status dsr_bf_calc_gsc_weights(dsr_bf* s, double fs, const double* delays)
{
  return guard([&] {
    if (!s || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    if (s->C <= 1) throw Error(DSR_E_DIMENSION, "The number of channels must be > 1 but it is %d", s->C);
    calc_mainlobe(*s, fs, delays);
    const int C = s->C, M = s->M, bs = C - 1;
    s->B.assign((size_t) M * C * bs, zc(0, 0)); s->wa.assign((size_t) M * bs, zc(0, 0)); s->wl.assign((size_t) M * C, zc(0, 0));
    for (int f = 0; f < M; f++) blocking_matrix(&s->wq[(size_t) f * C], C, &s->B[(size_t) f * C * bs]);
    s->haveB = true; s->dirty = true;
  });
}
dsr_status dsr_bf_set_active_weights(dsr_bf* s, int f, const double* packed)
{
  return guard([&] {
    if (!s || !packed) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
    if (f < 0 || f >= s->M) throw Error(DSR_E_DIMENSION, "Must be a frequency bin %d < the length of FFT %d", f, s->M);
    for (int c = 0; c < s->C - 1; c++) s->wa[(size_t) f * (s->C - 1) + c] = zc(packed[2 * c], packed[2 * c + 1]);
    update_wl(*s, f);
    s->dirty = true;
  });
}
dsr_status dsr_bf_zero_active_weights(dsr_bf* s)
{
  return guard([&] {
    if (!s || !s->haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
    std::fill(s->wa.begin(), s->wa.end(), zc(0, 0)); for (int f = 0; f < s->M; f++) update_wl(*s, f); s->dirty = true;
  });
}
dsr_status dsr_bf_select(dsr_bf* s, int mode)
{ return guard([&] { if (!s || mode < 0 || mode > 4) throw Error(DSR_E_PARAMETER, "bad mode"); s->mode = mode; s->dirty = true; }); }

dsr_status dsr_bf_get(const dsr_bf* cs, int kind, double* out, size_t nd)
{
  return guard([&] {
    dsr_bf* s = const_cast<dsr_bf*>(cs);
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    const std::vector<zc>* v = nullptr;
    if (kind == 4) { if (s->dirty) { require_device(); refresh_effective(*s); } v = &s->eff; }
    else v = kind == 0 ? &s->wq : kind == 1 ? &s->mvdr : kind == 2 ? &s->R : kind == 3 ? &s->B : nullptr;
    if (!v) throw Error(DSR_E_PARAMETER, "bad kind %d", kind);
    if (nd < 2 * v->size()) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, need %zu", nd, 2 * v->size());
    for (size_t i = 0; i < v->size(); i++) { out[2 * i] = (*v)[i].real(); out[2 * i + 1] = (*v)[i].imag(); }
  });
}

dsr_status dsr_bf_apply(dsr_bf* s, const float* X, int U, int Tmax, float* Y, void* stream)
{
  return guard([&] {
    if (!s || !X || !Y) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    if (s->rlsOn) { gsc_rls_apply(*s, X, nullptr, U, Tmax, Y, nullptr, (hipStream_t) stream); return; }
    if (s->dirty) refresh_effective(*s);
    if (U <= 0 || Tmax <= 0) return;
    const int F = s->halfBandShift ? s->M : s->M / 2 + 1;
    const size_t lds = sizeof(float2) * (size_t) F * s->C;
    if (lds > 160 * 1024) throw Error(DSR_E_DIMENSION, "beamformer weights need %zu bytes of LDS", lds);
    bf_launch_apply(X, s->d_w.p, s->C, F, U, Tmax, Y, (hipStream_t) stream);
  });
}


// SubbandGSCRLS(fftLen, halfBandShift, myu, sigma2) (beamformer.h:230-262).  rls_config switches dsr_bf_apply to the recursive-least-squares
// GSC (the object must hold GSC weights: calcGSCWeights); sigma2 is the constructor's diagonal weight of the active-weight update.
dsr_status dsr_bf_rls_config(dsr_bf* s, float myu, float sigma2)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!(myu > 0.0f)) throw Error(DSR_E_PARAMETER, "the forgetting factor must be positive (%g)", (double) myu);
    s->rlsOn = true; s->rlsMyu = (double) myu; s->rlsDiag.assign((size_t) s->M / 2 + 1, (double) sigma2); s->rlsDirty = true;
    if (s->mode < 2) s->mode = 2;
  });
}
// initPrecisionMatrix(sigma2): P = I / sigma2 for every bin, active weights zeroed (beamformer.cc:1526-1538)
dsr_status dsr_bf_rls_init_precision(dsr_bf* s, float sigma2)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
    const int n = s->C - 1, F = s->M / 2 + 1;
    s->rlsP0.assign((size_t) F * n * n, zc(0, 0));
    for (int f = 0; f < F; f++) for (int i = 0; i < n; i++) s->rlsP0[((size_t) f * n + i) * n + i] = zc((double) (1 / sigma2), 0.0);
    std::fill(s->wa.begin(), s->wa.end(), zc(0, 0));
    s->haveP0 = true; s->rlsDirty = true; s->dirty = true; s->rlsHaveState = false;
  });
}
// setPrecisionMatrix(fbinX, Pz) (:1540-1552); Pz [C-1][C-1] complex128
dsr_status dsr_bf_rls_set_precision(dsr_bf* s, int fbinX, const double* Pz)
{
  return guard([&] {
    if (!s || !Pz) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
    const int n = s->C - 1, F = s->M / 2 + 1;
    if (fbinX < 0 || fbinX >= F) throw Error(DSR_E_DIMENSION, "Must be a frequency bin %d <= %d", fbinX, F - 1);
    if (s->rlsP0.size() != (size_t) F * n * n) s->rlsP0.assign((size_t) F * n * n, zc(0, 0));
    for (int e = 0; e < n * n; e++) s->rlsP0[(size_t) fbinX * n * n + e] = zc(Pz[2 * e], Pz[2 * e + 1]);
    s->haveP0 = true; s->rlsDirty = true; s->rlsHaveState = false;
  });
}
dsr_status dsr_bf_rls_quadratic_constraint(dsr_bf* s, float alpha, int qctype)
{ return guard([&] { if (!s || qctype < 0 || qctype > 2) throw Error(DSR_E_PARAMETER, "bad quadratic constraint type"); s->rlsAlpha = (double) alpha; s->rlsQc = qctype; }); }
dsr_status dsr_bf_rls_adapt(dsr_bf* s, int flag) { return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->rlsAdapt = flag != 0; }); }
// batch entry with the final active weights: wa_out_dev (optional) [U][M/2+1][C-1] complex128
dsr_status dsr_bf_gsc_rls(dsr_bf* s, const float* X, const int32_t* nframes_dev, int U, int Tmax, float* Y, double* wa_out_dev, void* stream)
{
  return guard([&] {
    if (!s || !X || !Y) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->rlsOn) throw Error(DSR_E_ERROR, "not a SubbandGSCRLS object: call dsr_bf_rls_config first");
    require_device();
    gsc_rls_apply(*s, X, nframes_dev, U, Tmax, Y, wa_out_dev, (hipStream_t) stream);
  });
}
dsr_status dsr_bf_rls_path(int chanN, int path[3], int64_t lds[2])
{
  return guard([&] {
    if (!path) throw Error(DSR_E_PARAMETER, "null argument");
    if (chanN < 2 || chanN > 64) throw Error(DSR_E_DIMENSION, "SubbandGSCRLS: 2 to 64 channels (%d)", chanN);
    const RlsPath r = rls_path(chanN);
    path[0] = r.ct; path[1] = r.cap; path[2] = r.residence;
    if (lds) { lds[0] = (int64_t) r.stateBytes; lds[1] = (int64_t) r.ldsBytes; }
  });
}
// dsr_bf_apply with per-utterance frame counts: rows t >= nframes[u] are zero; an adapting (RLS) object stops adapting there
dsr_status dsr_bf_apply_frames(dsr_bf* s, const float* X, const int32_t* nframes_dev, int U, int Tmax, float* Y, void* stream)
{
  if (s && s->rlsOn) return dsr_bf_gsc_rls(s, X, nframes_dev, U, Tmax, Y, nullptr, stream);
  return dsr_bf_apply(s, X, U, Tmax, Y, stream);               // fixed weights: the padded rows of X are zero, so are the outputs
}
// carry on: every call continues from the precision matrices and active weights the previous call left (same U); the first call after
// rls_reset_state / rls_init_precision / rls_set_precision starts from those matrices and zero weights
dsr_status dsr_bf_rls_carry(dsr_bf* s, int on)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->rlsCarry = on != 0; if (!on) s->rlsHaveState = false; }); }
dsr_status dsr_bf_rls_reset_state(dsr_bf* s)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->rlsHaveState = false; }); }


// SubbandMVDRGSC (beamformer.h:394-425, beamformer.cc:2637-2817): the MVDR vector as the quiescent weight of a GSC whose active weights are
// set from outside.  calcBlockingMatrix1: a fresh weight object with the delay-and-sum vectors and their blocking matrices (:2671-2676) -- the
// same state as calcGSCWeights; calcBlockingMatrix2: fresh object, bins 1..M/2 get the MVDR vector as quiescent vector and its blocking
// matrix (:2682-2706), everything else stays zero.
dsr_status dsr_bf_calc_blocking_matrix2(dsr_bf* s)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveMvdr) throw Error(DSR_E_ERROR, "You have to call calcMVDRWeights() first");
    if (s->halfBandShift) throw Error(DSR_E_ERROR, "Not yet implemented");
    const int C = s->C, M = s->M, bs = C - 1;
    s->wq.assign((size_t) M * C, zc(0, 0)); s->B.assign((size_t) M * C * bs, zc(0, 0)); s->wa.assign((size_t) M * bs, zc(0, 0)); s->wl.assign((size_t) M * C, zc(0, 0));
    for (int f = 1; f <= M / 2; f++) {
      for (int c = 0; c < C; c++) s->wq[(size_t) f * C + c] = s->mvdr[(size_t) f * C + c];
      blocking_matrix(&s->wq[(size_t) f * C], C, &s->B[(size_t) f * C * bs]);
    }
    s->haveWq = true; s->haveB = true; s->dirty = true; s->rlsDirty = true;
  });
}
// upgradeBlockingMatrix (:2708-2727): blocking matrices orthogonal to the entire weight wq - wl, bins 1..M-1; the cached wl stays as it is
dsr_status dsr_bf_upgrade_blocking_matrix(dsr_bf* s)
{
  return guard([&] {
    if (!s || !s->haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
    const int C = s->C, M = s->M, bs = C - 1; std::vector<zc> w(C);
    if (s->wl.size() != (size_t) M * C) s->wl.assign((size_t) M * C, zc(0, 0));
    for (int f = 1; f < M; f++) {
      for (int c = 0; c < C; c++) w[c] = s->wq[(size_t) f * C + c] - s->wl[(size_t) f * C + c];
      blocking_matrix(w.data(), C, &s->B[(size_t) f * C * bs]);
    }
    s->dirty = true; s->rlsDirty = true;
  });
}
// blockingMatrixOutput(outChanX) (:2729-2753) for a batch: Y[u][t][f] = B_f[:, outChanX]^H X[u][:][t][f], f = 0..M/2
dsr_status dsr_bf_blocking_matrix_output(dsr_bf* s, const float* X, int U, int Tmax, int outChanX, float* Y, void* stream)
{
  return guard([&] {
    if (!s || !X || !Y) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveB) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
    const int C = s->C, bs = C - 1, F = s->M / 2 + 1;
    if (outChanX < 0 || outChanX >= bs) throw Error(DSR_E_INDEX, "blocking matrix column %d of %d", outChanX, bs);
    require_device();
    if (U <= 0 || Tmax <= 0) return;
    std::vector<float2> w((size_t) F * C);
    for (int f = 0; f < F; f++) for (int c = 0; c < C; c++) { const zc b = s->B[((size_t) f * C + c) * bs + outChanX]; w[(size_t) f * C + c] = make_float2((float) b.real(), (float) b.imag()); }
    DevBuf<float2>& dW = s->d_wB.at((hipStream_t) stream); dW.upload(w, (hipStream_t) stream);
    bf_launch_apply(X, dW.p, C, F, U, Tmax, Y, (hipStream_t) stream);
  });
}

}  // extern "C"
