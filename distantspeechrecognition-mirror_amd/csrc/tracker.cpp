// csrc/tracker.cpp -- host side of the spherical-array speaker trackers of btk/beamformer/tracker.{h,cc} (kernels: csrc/k_tracker.hip; what the two
// share: csrc/tracker.h).  Line numbers are tracker.cc's.
//
// Set-up work, as in the reference: the EigenMike geometry (:195-297, the table of csrc/sph_math.h), _bn = 4 pi i^n b_n(ka) with
// modalCoefficient's own closed forms (:474-628), the conjugated harmonics at the sensors (:117-130), _calculateNormalization per mode, the
// per-bin observation-noise Cholesky blocks (setV :961-981) and the plane-wave coefficients (:1453-1465).  Then the dsr_trk_* / dsr_pws_* entries.
#include "tracker.h"
#include <algorithm>

using namespace dsr;

typedef std::complex<double> zc;

namespace {

constexpr double SSPEED = 343740.0;                          // BaseDecomposition::_SpeedOfSound (:86)

// _calculateNormalization (:381-403)
double trk_norm(int order, int degree)
{
  double norm = std::sqrt((2 * order + 1) / (4.0 * M_PI)), factor = 1.0;
  if (degree >= 0) { int m = degree; while (m > -degree) { factor *= (order + m); m--; } norm /= std::sqrt(factor); }
  else { int m = -degree; while (m > degree) { factor *= (order + m); m--; } norm *= std::sqrt(factor); }
  return norm;
}

zc modal_coefficient(unsigned order, double ka)              // :474-628
{
  if (ka == 0.0) return zc(1.0, 0.0);
  const double c = std::cos(ka), s = std::sin(ka);
  const double ka2 = ka * ka, ka3 = ka2 * ka, ka4 = ka2 * ka2, ka5 = ka4 * ka, ka6 = ka5 * ka, ka7 = ka6 * ka, ka8 = ka7 * ka, ka9 = ka8 * ka;
  auto mul_imag = [](zc a, double y) { return zc(-y * a.imag(), y * a.real()); };
  switch (order) {
  case 0: {
    const double j0 = gsinc(ka / M_PI);
    const zc h0(j0, -c / ka);
    const double val1 = ka * c - s;
    const zc val2 = gmul(zc(ka, 1), zc(c, s));
    const zc grad = gdiv(zc(val1, 0), val2), g = gmul(grad, h0);
    return zc(j0 - g.real(), 0.0 - g.imag());
  }
  case 1: return gmulr(gdiv(zc(-c, s), zc(ka2 - 2, 2 * ka)), ka);
  case 2: return mul_imag(gdiv(zc(c, -s), zc(ka3 - 9 * ka, 4 * ka2 - 9)), ka2);
  case 3: return gmulr(gdiv(zc(c, -s), zc(ka4 - 27 * ka2 + 60, 7 * ka3 - 60 * ka)), ka3);
  case 4: return gmulr(gdiv(zc(s, c), zc(ka5 - 65 * ka3 + 525 * ka, 11 * ka4 - 240 * ka2 + 525)), ka4);
  case 5: return gmulr(gdiv(zc(c, -s), zc(ka6 - 135 * ka4 + 2625 * ka2 - 5670, 16 * ka5 - 735 * ka3 + 5670 * ka)), ka5);
  case 6: return mul_imag(gdiv(zc(c, -s), zc(ka7 - 252 * ka5 + 9765 * ka3 - 72765 * ka, 22 * ka6 - 1890 * ka4 + 34020 * ka2 - 72765)), ka6);
  case 7: return gmulr(gdiv(zc(c, -s), zc(1081080 - 509355 * ka2 + 29925 * ka4 - 434 * ka6 + ka8, -1081080 * ka + 148995 * ka3 - 4284 * ka5 + 29 * ka7)), ka7);
  case 8: return gmulr(gdiv(zc(s, c), zc(18243225 * ka - 2567565 * ka3 + 79695 * ka5 - 702 * ka7 + ka9,
                                         18243225 - 8648640 * ka2 + 530145 * ka4 - 8820 * ka6 + 37 * ka8)), ka8);
  default: {
    const double jn = sph_jl(order, ka), yn = sph_yl(order, ka);
    const double jp = sph_jl(order - 1, ka), jnn = sph_jl(order + 1, ka), yp = sph_yl(order - 1, ka), ynn = sph_yl(order + 1, ka);
    const double djn = (jp - jnn) / 2;
    const zc hn(jn, yn), hp(jp, yp), hnn(jnn, ynn);
    const zc val = gdivr(hn + gmulr(hnn, ka), ka);
    const zc dhn = gmulr(hp - val, 0.5);
    const zc grad = gdiv(zc(djn, 0), dhn), g = gmul(grad, hn);
    return zc(-g.real() + jn, -g.imag());
  }
  }
}

zc host_harmonic(int n, int m, double theta, double phi)
{
  const Harm h = trk_harm(n, m, std::cos(theta), std::sin(theta), phi, trk_norm(n, m));
  return zc(h.yr, h.yi);
}

}  // namespace

extern "C" {

dsr_status dsr_trk_create(int kind, int orderN, int fftLen, double a, double sampleRate, int useSubbandsN, double sigma2_u, double sigma2_v, double sigma2_init,
                          int maxLocalN, int chanN, dsr_trk** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_ARG, "out is null");
    *out = nullptr;
    if (chanN != CHAN) throw Error(DSR_E_ARG, "the trackers are built for the EigenMike's %d channels, not %d", CHAN, chanN);
    if (kind != DSR_TRK_MODAL && kind != DSR_TRK_SPATIAL) throw Error(DSR_E_ARG, "kind %d: DSR_TRK_MODAL or DSR_TRK_SPATIAL", kind);
    if (orderN < 0 || orderN > MAX_ORDER_N) throw Error(DSR_E_ARG, "orderN %d outside [0, %d]", orderN, MAX_ORDER_N);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_ARG, "fftLen %d: an even length >= 2", fftLen);
    const int F = fftLen / 2 + 1;
    if (useSubbandsN < 0 || useSubbandsN > F) throw Error(DSR_E_ARG, "useSubbandsN %d outside [0, %d]", useSubbandsN, F);
    if (maxLocalN < 1 || maxLocalN > 255) throw Error(DSR_E_ARG, "maxLocalN %d outside [1, 255]", maxLocalN);
    if (!(sigma2_u >= 0.0) || !(sigma2_v >= 0.0) || !(sigma2_init >= 0.0)) throw Error(DSR_E_ARG, "negative variance");
    std::unique_ptr<dsr_trk> s(new dsr_trk());
    s->spatial = kind == DSR_TRK_SPATIAL; s->orderN = orderN; s->modesN = (orderN + 1) * (orderN + 1); s->M = fftLen; s->F = F;
    s->K = useSubbandsN == 0 ? F : useSubbandsN; s->L = s->spatial ? CHAN : s->modesN; s->N = s->K * s->L; s->maxLocalN = maxLocalN;
    s->a = a; s->fs = sampleRate; s->s2u = sigma2_u; s->s2v = sigma2_v; s->s2init = sigma2_init;
    const long lim = trk_max_rows(s->modesN, orderN, s->spatial, s->K);
    if (2L * s->N > lim) throw Error(DSR_E_ARG, "2N = 2 x %d x %d = %ld rows exceed the %ld the workgroup's LDS holds", s->K, s->L, 2L * s->N, lim);
    s->lds = trk_lds_bytes(*s);
    const int O1 = orderN + 1;
    s->bn.resize((size_t) F * O1); s->absbn.resize((size_t) F * O1);
    static const zc IN[4] = {zc(1, 0), zc(0, 1), zc(-1, 0), zc(0, -1)};      // _calc_in (:299-312)
    for (int f = 0; f < F; f++) {
      const double ka = 2.0 * M_PI * f * a * sampleRate / (fftLen * SSPEED);
      for (int n = 0; n < O1; n++) {
        const zc b = gmul(gmul(zc(4.0 * M_PI, 0.0), IN[n % 4]), modal_coefficient(n, ka));
        s->bn[(size_t) f * O1 + n] = b; s->absbn[(size_t) f * O1 + n] = std::hypot(b.real(), b.imag());
      }
    }
    s->sc.resize((size_t) s->modesN * CHAN); s->norm.resize(s->modesN);
    int idx = 0;
    for (int n = 0; n <= orderN; n++)
      for (int m = -n; m <= n; m++, idx++) {
        s->norm[idx] = trk_norm(n, m);
        for (int c = 0; c < CHAN; c++) s->sc[(size_t) idx * CHAN + c] = std::conj(host_harmonic(n, m, EM_THETA[c] * M_PI / 180.0, EM_PHI[c] * M_PI / 180.0));
      }
    *out = s.release();
  });
}

void dsr_trk_destroy(dsr_trk* s) { delete s; }
int dsr_trk_state_doubles(const dsr_trk*) { return STATE_DOUBLES; }
int dsr_trk_modes_n(const dsr_trk* s) { return s ? s->modesN : 0; }
int dsr_trk_subband_length(const dsr_trk* s) { return s ? s->L : 0; }
int dsr_trk_use_subbands_n(const dsr_trk* s) { return s ? s->K : 0; }
int dsr_trk_fft_len(const dsr_trk* s) { return s ? s->M : 0; }
int64_t dsr_trk_max_rows(int kind, int orderN, int useSubbandsN) { return trk_max_rows((orderN + 1) * (orderN + 1), orderN, kind == DSR_TRK_SPATIAL, useSubbandsN); }

dsr_status dsr_trk_set_v(dsr_trk* s, const double* Vk, size_t nDoubles, unsigned subbandX)
{
  return guard([&] {
    if (!s || !Vk) throw Error(DSR_E_ARG, "null argument");
    const int L = s->L, L2 = 2 * L;
    if ((int) subbandX >= s->F) throw Error(DSR_E_ARG, "subband %u outside [0, %d)", subbandX, s->F);
    if (nDoubles != (size_t) 2 * L * L) throw Error(DSR_E_ARG, "Vk: %d x %d complex values expected", L, L);
    std::vector<double> B((size_t) L2 * L2, 0.0);
    if (!s->V.empty()) std::copy(s->V.begin() + (size_t) subbandX * L2 * L2, s->V.begin() + (size_t) (subbandX + 1) * L2 * L2, B.begin());
    else for (int n = 0; n < L2; n++) B[(size_t) n * L2 + n] = std::sqrt(s->s2v);
    for (int m = 0; m < L; m++)                              // :965-974: the lower triangle only; (m + L, n) with n > m keeps its contents
      for (int n = 0; n <= m; n++) {
        const double c = Vk[2 * ((size_t) m * L + n)], sg = Vk[2 * ((size_t) m * L + n) + 1];
        B[(size_t) m * L2 + n] = c; B[(size_t) (m + L) * L2 + n + L] = c; B[(size_t) (m + L) * L2 + n] = sg;
      }
    std::vector<double> C((size_t) L2 * L2, 0.0);            // the Cholesky factor of the lower triangle, row by row; the strict upper part zero
    for (int i = 0; i < L2; i++) {
      for (int j = 0; j < i; j++) {
        double sum = 0.0; for (int k = 0; k < j; k++) sum += C[(size_t) i * L2 + k] * C[(size_t) j * L2 + k];
        C[(size_t) i * L2 + j] = (B[(size_t) i * L2 + j] - sum) / C[(size_t) j * L2 + j];
      }
      double sum = 0.0; for (int k = 0; k < i; k++) sum += C[(size_t) i * L2 + k] * C[(size_t) i * L2 + k];
      const double d = B[(size_t) i * L2 + i] - sum;
      if (!(d > 0.0)) throw Error(DSR_E_ARG, "setV: the block of subband %u is not positive definite", subbandX);
      C[(size_t) i * L2 + i] = std::sqrt(d);
    }
    if (s->V.empty()) {
      s->V.assign((size_t) s->F * L2 * L2, 0.0);
      for (int f = 0; f < s->F; f++) for (int n = 0; n < L2; n++) s->V[((size_t) f * L2 + n) * L2 + n] = std::sqrt(s->s2v);
    }
    std::copy(C.begin(), C.end(), s->V.begin() + (size_t) subbandX * L2 * L2);
    s->vDirty = true;
  });
}

dsr_status dsr_trk_get_v(const dsr_trk* s, unsigned subbandX, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_ARG, "null argument");
    const int L2 = 2 * s->L;
    if ((int) subbandX >= s->F || outDoubles != (size_t) L2 * L2) throw Error(DSR_E_ARG, "subband %u, %d x %d doubles expected", subbandX, L2, L2);
    if (s->V.empty()) { std::fill(out, out + outDoubles, 0.0); for (int n = 0; n < L2; n++) out[(size_t) n * L2 + n] = std::sqrt(s->s2v); }
    else std::copy(s->V.begin() + (size_t) subbandX * L2 * L2, s->V.begin() + (size_t) (subbandX + 1) * L2 * L2, out);
  });
}

dsr_status dsr_trk_set_initial_position(dsr_trk* s, double theta, double phi)
{ return guard([&] { if (!s) throw Error(DSR_E_ARG, "null handle"); s->th0 = theta; s->ph0 = phi; }); }
dsr_status dsr_trk_next_speaker(dsr_trk* s)
{ return guard([&] { if (!s) throw Error(DSR_E_ARG, "null handle"); s->th0 = 0.5; s->ph0 = 0.0; }); }

dsr_status dsr_trk_init_state(dsr_trk* s, double* state_dev, int U, int positionOnly, void* stream)
{
  return guard([&] {
    if (!s || !state_dev || U <= 0) throw Error(DSR_E_ARG, "null argument or U <= 0");
    require_device();
    trk_launch_init(state_dev, U, s->th0, s->ph0, std::sqrt(std::sqrt(s->s2init)), positionOnly, (hipStream_t) stream);
  });
}

dsr_status dsr_trk_bn(const dsr_trk* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out || outDoubles != 2 * s->bn.size()) throw Error(DSR_E_ARG, "bn: [fftLen/2+1][orderN+1] complex128 expected");
    memcpy(out, s->bn.data(), sizeof(double) * outDoubles);
  });
}
dsr_status dsr_trk_sensor_harmonics(const dsr_trk* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out || outDoubles != 2 * s->sc.size()) throw Error(DSR_E_ARG, "sensor harmonics: [modesN][32] complex128 expected");
    memcpy(out, s->sc.data(), sizeof(double) * outDoubles);
  });
}
dsr_status dsr_trk_geometry(double* theta_s, double* phi_s, int n)
{
  return guard([&] {
    if (!theta_s || !phi_s || n != CHAN) throw Error(DSR_E_ARG, "the geometry has %d sensors", CHAN);
    for (int c = 0; c < CHAN; c++) { theta_s[c] = EM_THETA[c] * M_PI / 180.0; phi_s[c] = EM_PHI[c] * M_PI / 180.0; }
  });
}

dsr_status dsr_trk_harmonic(int order, int degree, double theta, double phi, double* out2)
{
  return guard([&] {
    if (!out2 || order < 0 || degree > order || -degree > order) throw Error(DSR_E_ARG, "|degree| <= order expected");
    const zc y = host_harmonic(order, degree, theta, phi); out2[0] = y.real(); out2[1] = y.imag();
  });
}
dsr_status dsr_trk_harmonic_deriv_polar(int order, int degree, double theta, double phi, double* out2)
{
  return guard([&] {
    if (!out2 || order < 0 || degree > order || -degree > order) throw Error(DSR_E_ARG, "|degree| <= order expected");
    const Harm h = trk_harm(order, degree, std::cos(theta), std::sin(theta), phi, trk_norm(order, degree)); out2[0] = h.tr; out2[1] = h.ti;
  });
}
dsr_status dsr_trk_harmonic_deriv_azimuth(int order, int degree, double theta, double phi, double* out2)
{
  return guard([&] {
    if (!out2 || order < 0 || degree > order || -degree > order) throw Error(DSR_E_ARG, "|degree| <= order expected");
    const Harm h = trk_harm(order, degree, std::cos(theta), std::sin(theta), phi, trk_norm(order, degree)); out2[0] = h.pr; out2[1] = h.pi;
  });
}
dsr_status dsr_trk_modal_coefficient(unsigned order, double ka, double* out2)
{
  return guard([&] {
    if (!out2) throw Error(DSR_E_ARG, "null argument");
    const zc b = modal_coefficient(order, ka); out2[0] = b.real(); out2[1] = b.imag();
  });
}

dsr_status dsr_trk_run(dsr_trk* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, double* state_dev, float* pos_dev, double* pos64_dev,
                       int32_t* info_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !nframes_dev || !state_dev || !pos_dev || !pos64_dev || !info_dev) throw Error(DSR_E_ARG, "null argument");
    if (U <= 0 || Tmax <= 0) throw Error(DSR_E_ARG, "U and Tmax must be positive");
    require_device();
    trk_launch_run(*s, X_dev, nframes_dev, U, Tmax, state_dev, pos_dev, pos64_dev, info_dev, (hipStream_t) stream);
  });
}

dsr_status dsr_pws_coefficients(const dsr_trk* s, double theta, double phi, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out || outDoubles != (size_t) 2 * CHAN * s->F) throw Error(DSR_E_ARG, "coefficients: [32][fftLen/2+1] complex128 expected");
    const int O1 = s->orderN + 1;
    std::vector<zc> Y(s->modesN);
    int idx = 0;
    for (int n = 0; n <= s->orderN; n++) for (int m = -n; m <= n; m++) Y[idx++] = host_harmonic(n, m, theta, phi);
    for (int c = 0; c < CHAN; c++)
      for (int f = 0; f < s->F; f++) {                       // :1453-1465
        zc coefficient(0, 0);
        for (int n = 0; n < O1; n++) {
          zc coeff_n(0, 0);
          for (int i = n * n; i < (n + 1) * (n + 1); i++) coeff_n += gmul(s->sc[(size_t) i * CHAN + c], Y[i]);
          coefficient += gmul(s->bn[(size_t) f * O1 + n], coeff_n);
        }
        out[2 * ((size_t) c * s->F + f)] = coefficient.real(); out[2 * ((size_t) c * s->F + f) + 1] = coefficient.imag();
      }
  });
}

dsr_status dsr_pws_apply(const double* coef_dev, int chanN, const float* src_dev, const int32_t* nframes_dev, int U, int Tmax, int fftLen, int full, float* out_dev,
                         void* stream)
{
  return guard([&] {
    if (!coef_dev || !src_dev || !nframes_dev || !out_dev) throw Error(DSR_E_ARG, "null argument");
    if (chanN <= 0 || U <= 0 || Tmax <= 0 || fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_ARG, "chanN, U, Tmax positive and fftLen even expected");
    require_device();
    pws_launch_apply(coef_dev, chanN, src_dev, nframes_dev, U, Tmax, fftLen, full, out_dev, (hipStream_t) stream);
  });
}

}  // extern "C"
