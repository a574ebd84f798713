// csrc/k_sph.hip -- spherical-array (modal) beamforming and 2-D steered-response-power DOA estimation:
// EigenBeamformer, SphericalDSBeamformer, DOAEstimatorSRPEB, DOAEstimatorSRPSphDSB (btk/beamformer/modalBeamformer.{h,cc}).
//
// Host side (set-up work, as in the reference): the rigid-sphere mode amplitudes b_n(ka) (modeAmplitude :37-170, _calcModeAmplitudes),
// the conjugated spherical harmonics at the sensors sh_s [dim][C] (sphericalHarmonic :189-217, _calcSphericalHarmonicsAtEachPosition),
// the look-direction weights (EigenBeamformer::_calcWeights :304-345, SphericalDSBeamformer::_calcWeights :1022-1058, calcDCWeights),
// the (theta, phi) grid and steering table (_calcSteeringUnitTable :793-858, :1190-1246) and the final N-best from the accumulators.
// The spherical Bessel functions are computed here (series below x = l + 1, upward recurrence above; y_l upward): no GSL.
//
// Device side, a batch of utterances X [U][C][Tmax][M/2+1] complex64 (the layout dsr_fb_analysis writes):
//   k_sph_apply  the beamformer: F = sh_s X per bin and frame (sphericalHarmonicsTransformation), y = w^H F, optionally F itself.  One
//                thread per (utterance, frame, bin) on the VALU, the eigenbeams 8 at a time in registers; X is re-read per group of 8
//                from L1/L2.  S and w are wave-uniform or per-bin reads.
//   k_sph_srp    rp[u][t][unit] = sum_f g_f |w_unit,f^H (S X_f)|^2 / (fbinMax - fbinMin + 1) fused on v_mfma_f64_16x16x4_f64: the
//                staging, frame tiles and energy of k_doa_srp; stage 1 forms the 16 frames' eigenbeams F (rows dim, 16 a tile, K = C)
//                in registers; stage 2 contracts them with 16-unit tiles.  The MFMA's result register q of lane l holds
//                F[16 dt + (l >> 4) + 4 q][frame l & 15], exactly the B operand of a K step q whose k index is (l >> 4): the weights are
//                pre-permuted to that order ([bin][unit tile][dim tile][q][lane], conjugated), so F never leaves the registers.
//   folded       W_f^H S precomputed on the host as a [units][C] table and run through k_doa_srp (csrc/k_doa.hip) unchanged: exact up to
//                fp64 rounding, cheaper when dim (C + units) >= C units.  The host picks by that flop count; DSR_SPH_SRP_PATH=fused|folded
//                forces one.
//   k_sph_frame  per frame, one wave: the gate and the frame's N-best by (rp descending, unit ascending), which is the reference's strict-">"
//                insertion (:922-943) since every rp >= 0 > -10e10; nBest rounds of a wave arg-max over the frame's row
//   k_doa_acc    (csrc/k_doa.hip) acc[u][unit] += rp of every ungated frame, frame by frame in order
//   k_sph_beams_valu / k_sph_beams_mfma   NB <= 16 beams in one pass over X: Y[u][b][t][f] = v_{b,f}^H X[u][:,t,f] with sensor-domain vectors v
//                (the modal kinds' w_eff^H S folded on the host in fp64, the sensor-domain kinds' weights as they are).  Up to 4 beams: one thread
//                per (t, f) on the VALU, x read once (the (t, f) plane of a channel is contiguous: coalesced whatever F is), the beams'
//                accumulators in registers (fp64), conj(v) staged in LDS a few channels at a time.  Above 4: the complex GEMM of k_doa_srp
//                (rows 16 beams zero padded, columns 16 frames a wave, K = C) without the power reduction; every result is stored.
// The further kinds (SphericalHWNCBeamformer :1387-1478, SphericalGSCBeamformer :1483-1594, SphericalHWNCGSCBeamformer :1599-1713,
// SphericalMOENBeamformer :1804-2099, SphericalSpatialDSBeamformer :2106-2270) are host weight designs below; all of them run on the beams kernels.
// The MFMA's lane map: csrc/mfma64.h; the frame tiling (FB, bin_chunk) and the shared kernel parts: csrc/srp_common.h.
#include "launch.h"
#include "srp_common.h"
#include "sph_math.h"
#include "gsc_weights.h"
#include "svd_linpack.h"
#include <algorithm>
#include <cmath>
#include <complex>

using namespace dsr;

typedef std::complex<double> zc;

namespace {

constexpr double SSPEED = 343740.0;                          // mm/s (beamformer.h:47)
constexpr int MAX_ORDER = 8;                                 // dim = maxOrder^2 <= 64: four 16-row tiles of the fused kernel
constexpr int MAX_BEAMS = 16;                               // one MFMA row tile
constexpr long MAX_TABLE = 1L << 27;                         // (fbinMax+1) units max(dim, C) complex128 entries: 2 GiB per table copy

}  // namespace

struct dsr_sph {
  int kind = DSR_SPH_EB, nBest = 1, M = 0, C = 0, maxOrder = 1, dim = 1; unsigned sampleRate = 16000; bool normalize = false;
  float sigma2 = 0.0f, wgain = 1.0f;
  double a = 0.0; std::vector<double> thS, phS;              // geometry: radius (mm) and the sensors' (theta_s, phi_s)
  double lookTheta = 0.0, lookPhi = 0.0;
  double minTheta = -M_PI, maxTheta = M_PI, minPhi = -M_PI, maxPhi = M_PI, widthTheta = 0.25, widthPhi = 0.25;  // DOAEstimatorSRPBase (beamformer.cc:2922-2938)
  int fbinMin = 1, fbinMax = 0; float threshold = 0.0f;
  std::vector<zc> B, SH;                                     // B [M/2+1][maxOrder], SH [dim][C] (conj Y at the sensors); empty until the geometry is set
  std::vector<zc> look; bool lookDirty = true;               // look [M/2+1][dim]: bin 0 the DC weights
  bool tbl = false; unsigned tableGen = 0; int nTheta = 0, nPhi = 0, tblFbinMax = 0;
  unsigned settingsGen = 0;                                  // bumped by every geometry / look-direction / sigma2 / gain change
  std::vector<double> uTheta, uPhi; std::vector<zc> W;       // W [tblFbinMax+1][units][dim]
  DevBuf<double2> dS, dSp, dLook, dWp; bool dSDirty = true, dLookDirty = true, dWDirty = true; int NT = 0, DT = 0, KS = 0;
  dsr_doa fold; unsigned foldGen = ~0u;                      // the folded path's [units][C] table, driven through k_doa_srp
  PerStream<DevBuf<double>> ws;
  // the further kinds
  float ratio = 1.0f; int NC = 1; bool lookSet = false;      // HWNC's _ratio; the GSC kinds' number of constraints; setLookDirection called
  std::vector<zc> Bm, wl;                                    // GSC: B [M/2+1][dim][dim-NC] (bin 0 stays zero), wl [M/2+1][dim] = B wa as last set
  std::vector<float> diag; bool fixedTerms = false;          // MOEN: _diagonalWeights [M/2+1], _isTermFixed
  std::vector<zc> fixedW; bool fixedWValid = false;          // MOEN: (A^H A + l I)^+ A^H [M/2+1][C][dim] (bin 0 unused), direction independent
  double beamTheta[MAX_BEAMS] = {0}, beamPhi[MAX_BEAMS] = {0}; bool beamSet[MAX_BEAMS] = {false}; unsigned beamGen = 0;   // beams 1.. (0 is the look direction)
  std::vector<zc> V; int vNB = 0; unsigned vSetGen = ~0u, vBeamGen = ~0u;   // V [NB][M/2+1][C]: y = v^H x
  DevBuf<double2> dV; int dVLayout = -1; bool dVDirty = true; // device copy, conjugated: layout 0 MFMA [F][KS][64], n > 0 VALU [C][n][F]
};

namespace {

// the GSL-shaped complex arithmetic (gmul, gdiv, gdivr, gmulr, gsinc), sph_plm and the EigenMike tables: csrc/sph_math.h

}  // namespace

namespace dsr {

// spherical Bessel j_l(x): the power series below x = l + 1 (terms shrink from the first), upward recurrence from j_0, j_1 above (stable for l < x)
double sph_jl(int l, double x)
{
  if (x == 0.0) return l == 0 ? 1.0 : 0.0;
  if (l == 0) return std::sin(x) / x;
  if (x < l + 1.0) {
    double lead = 1.0;                                       // x^l / (2l+1)!!
    for (int i = 1; i <= l; i++) lead *= x / (2.0 * i + 1.0);
    const double h = -0.5 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 200; k++) {
      term *= h / (k * (2.0 * l + 2.0 * k + 1.0));
      sum += term;
      if (std::fabs(term) < 1e-17 * std::fabs(sum)) break;
    }
    return lead * sum;
  }
  double jm = std::sin(x) / x, j = std::sin(x) / (x * x) - std::cos(x) / x;
  for (int n = 1; n < l; n++) { const double jn = (2.0 * n + 1.0) / x * j - jm; jm = j; j = jn; }
  return j;
}
// spherical Bessel y_l(x), x > 0: upward recurrence from y_0, y_1 (always stable)
double sph_yl(int l, double x)
{
  double ym = -std::cos(x) / x;
  if (l == 0) return ym;
  double y = -std::cos(x) / (x * x) - std::sin(x) / x;
  for (int n = 1; n < l; n++) { const double yn = (2.0 * n + 1.0) / x * y - ym; ym = y; y = yn; }
  return y;
}

// modeAmplitude (:37-170): orders 0-3 the reference's closed forms in its order of operations, from 4 on the j_l / y_l formula
zc mode_amplitude(int order, double ka)
{
  if (ka == 0) return zc(1, 0);
  const double s = std::sin(ka), c = std::cos(ka);
  switch (order) {
  case 0: {
    const double ka2 = ka * ka, j0 = gsinc(ka / M_PI), y0 = -c / ka;
    const zc h0(j0, y0);
    const double val1 = c / ka - s / ka2;
    const zc eika = std::polar(1.0, ka);
    const zc val2 = gdivr(gmul(zc(ka, 1), eika), ka2);
    const zc grad = gdiv(zc(val1, 0), val2);
    return zc(j0, 0) - gmul(grad, h0);
  }
  case 1: {
    const double ka2 = ka * ka, ka3 = ka2 * ka;
    const double j1 = (s / ka2) - (c / ka), y1 = -(c / ka2) - (s / ka);
    const zc h1(j1, y1);
    const double val1 = (-0.5 / ka) * (-c / ka + s / ka2) + 0.5 * (3 * c / ka2 + s / ka - (3 - ka2) * s / ka3);
    const double j0 = gsinc(ka / M_PI), y0 = -c / ka;
    const zc h0(j0, y0);
    const double j2 = (3 / ka3 - 1 / ka) * s - (3 / ka2) * c, y2 = -(3 / ka3 - 1 / ka) * c - (3 / ka2) * s;
    const zc h2(j2, y2);
    const zc val2 = gdivr((h0 - h2) - gdivr(h1, ka), 2);
    const zc grad = gdiv(zc(val1, 0), val2);
    return zc(j1, 0) - gmul(grad, h1);
  }
  case 2: {
    const double ka2 = ka * ka, ka3 = ka2 * ka, ka4 = ka3 * ka;
    const double j2 = (3 / ka3 - 1 / ka) * s - (3 * c / ka2), y2 = -(3 / ka3 - 1 / ka) * c - (3 * s / ka2);
    const zc h2(j2, y2);
    const double val1 = 0.5 * (-c / ka + s / ka2 + (18 - ka2) * c / ka3 + (-18 + 7 * ka2) * s / ka4);
    const double j1 = (s / ka2) - (c / ka), y1 = -(c / ka2) - (s / ka);
    const zc h1(j1, y1);
    const double j3 = (-15 + ka2) * c / ka3 - (-15 + 6 * ka2) * s / ka4, y3 = (-15 + ka2) * s / ka3 + (-15 + 6 * ka2) * c / ka4;
    const zc h3(j3, y3);
    const zc val2 = gdivr((h1 - h3) - gdivr(h2, ka), 2);
    const zc grad = gdiv(zc(val1, 0), val2);
    return zc(j2, 0) - gmul(grad, h2);
  }
  case 3: {
    const double ka2 = ka * ka, ka3 = ka2 * ka, ka4 = ka2 * ka2, ka5 = ka4 * ka;
    const double j3 = (-15 + ka2) * c / ka3 - (-15 + 6 * ka2) * s / ka4, y3 = (-15 + ka2) * s / ka3 + (-15 + 6 * ka2) * c / ka4;
    const zc h3(j3, y3);
    const double val1 = 0.5 * (-3 * c / ka2 + (3 - ka2) * s / ka3 + (120 - 11 * ka2) * c / ka4 + (-120 + 51 * ka2 - ka4) * s / ka5);
    const double j2 = (3 / ka3 - 1 / ka) * s - (3 * c / ka2), y2 = -(3 / ka3 - 1 / ka) * c - (3 * s / ka2);
    const zc h2(j2, y2);
    const double j4 = (-105 + 10 * ka2) * c / ka4 + (105 - 45 * ka2 + ka4) * s / ka5, y4 = (-105 + 10 * ka2) * s / ka4 - (105 - 45 * ka2 + ka4) * c / ka5;
    const zc h4(j4, y4);
    const zc val2 = gdivr((h2 - h4) - gdivr(h3, ka), 2);
    const zc grad = gdiv(zc(val1, 0), val2);
    return zc(j3, 0) - gmul(grad, h3);
  }
  default: {
    const double jn = sph_jl(order, ka), yn = sph_yl(order, ka);
    const double jp = sph_jl(order - 1, ka), jnn = sph_jl(order + 1, ka), yp = sph_yl(order - 1, ka), ynn = sph_yl(order + 1, ka);
    const double djn = (jp - jn / ka - jnn) / 2;
    const zc hn(jn, yn), hp(jp, yp), hnn(jnn, ynn);
    const zc dhn = gdivr((hp - hnn) - gdivr(hn, ka), 2);
    const zc grad = gdiv(zc(djn, 0), dhn);
    return zc(-gmul(grad, hn).real() + jn, -gmul(grad, hn).imag());
  }
  }
}

// sphericalHarmonic(degree m, order n, theta, phi) (:189-217): (-1)^|m| sphPlm(n, |m|) for m < 0, times e^{i m phi}
zc sph_harmonic(int m, int n, double theta, double phi)
{
  double p = sph_plm(n, m >= 0 ? m : -m, std::cos(theta));
  if (m < 0 && ((-m) % 2) != 0) p = -p;
  return gmulr(std::polar(1.0, m * phi), p);
}

}  // namespace dsr

namespace {

void need_geometry(const dsr_sph& s)
{
  if (s.thS.empty() || s.a == 0.0) throw Error(DSR_E_ERROR, "set the array geometry first (setArrayGeometry / setEigenMikeGeometry, radius > 0)");
}

void ensure_modes(dsr_sph& s)                                // _calcModeAmplitudes, bins 0..M/2
{
  need_geometry(s);
  if (!s.B.empty()) return;
  const int F = s.M / 2 + 1;
  s.B.resize((size_t) F * s.maxOrder);
  for (int f = 0; f < F; f++) {
    const double ka = 2.0 * M_PI * f * s.a * s.sampleRate / (s.M * SSPEED);
    for (int n = 0; n < s.maxOrder; n++) s.B[(size_t) f * s.maxOrder + n] = mode_amplitude(n, ka);
  }
}

inline bool hwnc(int kind) { return kind == DSR_SPH_HWNC || kind == DSR_SPH_HWNCGSC; }
inline bool gsc_kind(int kind) { return kind == DSR_SPH_GSC || kind == DSR_SPH_HWNCGSC; }
inline bool sensor_kind(int kind) { return kind == DSR_SPH_SPATIALDS || kind == DSR_SPH_MOEN; }   // weights of length C, no transform

void normalize_weights(zc* w, int n, float wgain)            // normalizeWeights (:23-29): wgain / ||w||_2
{
  double ss = 0.0;
  for (int i = 0; i < n; i++) ss += std::norm(w[i]);
  const double nrm = wgain / std::sqrt(ss);
  for (int i = 0; i < n; i++) w[i] = gmulr(w[i], nrm);
}

double hwnc_wng(const dsr_sph& s, int f)                     // SphericalHWNCBeamformer::calcWNG (:1397-1418): n < maxOrder, as the reference sums
{
  const double nrm = s.C / (16 * M_PI * M_PI);
  double val = 0.0;
  for (int n = 0; n < s.maxOrder; n++) val += (2 * n + 1) * std::norm(s.B[(size_t) f * s.maxOrder + n]);
  return nrm * val * s.ratio;
}

// _calcWeights of bin f for the direction (theta, phi) into w[dim], with the unit's harmonics Y [dim] at that direction precomputed
void calc_weights(const dsr_sph& s, int f, const zc* Y, zc* w)
{
  static const zc IN[4] = {zc(1, 0), zc(0, 1), zc(-1, 0), zc(0, -1)};
  const unsigned norm = (unsigned) s.dim * (unsigned) s.C;
  for (int n = 0, idx = 0; n < s.maxOrder; n++) {
    const zc bn = s.B[(size_t) f * s.maxOrder + n], in = IN[n % 4];
    if (s.kind == DSR_SPH_EB || hwnc(s.kind)) {             // :304-345, the HMDI beamformer (:1433-1462 the same)
      const double bn2 = std::norm(bn) + (double) s.sigma2, de = norm * bn2;
      const zc inbn = gmul(in, bn);
      for (int m = -n; m <= n; m++, idx++) w[idx] = gdivr(gmul(gmulr(std::conj(Y[idx]), 4 * M_PI), inbn), de);
    } else {                                                 // :1022-1058
      for (int m = -n; m <= n; m++, idx++) w[idx] = std::conj(gmulr(gmul(Y[idx], std::conj(gmul(in, bn))), 4 * M_PI));
    }
  }
  if (hwnc(s.kind)) {                                        // SphericalHWNCBeamformer::_calcWeights (:1464-1475); no normalizeWeight here
    if (s.ratio > 0.0f) normalize_weights(w, s.dim, (float) (2 * std::sqrt(M_PI / (s.C * hwnc_wng(s, f)))));   // (normalizeWeights takes a float)
    else {
      const double coeff = (16 * M_PI * M_PI) / (s.C * s.maxOrder * s.maxOrder);
      for (int i = 0; i < s.dim; i++) w[i] = gmulr(w[i], coeff);
    }
  } else if (s.normalize) normalize_weights(w, s.dim, s.wgain);
}

// SphericalSpatialDSBeamformer::_calcWeights (:2119-2172): w [C] of bin f in the sensor domain; Y the harmonics at the direction
void calc_spatial_ds(const dsr_sph& s, int f, const zc* Y, zc* w)
{
  static const zc IN[4] = {zc(1, 0), zc(0, 1), zc(-1, 0), zc(0, -1)};
  for (int c = 0; c < s.C; c++) {
    zc weight(0, 0);
    for (int n = 0, idx = 0; n < s.maxOrder; n++) {
      const zc inbn = gmul(IN[n % 4], s.B[(size_t) f * s.maxOrder + n]);
      zc tmp(0, 0);
      for (int m = -n; m <= n; m++, idx++) tmp += gmul(std::conj(s.SH[(size_t) idx * s.C + c]), std::conj(Y[idx]));
      weight += gmul(inbn, tmp);
    }
    w[c] = gmulr(weight, 4 * M_PI / s.C);
  }
}

// SphericalMOENBeamformer: _A of bin f (:1949-1981) and (A^H A + l I)^+ A^H (_calcMOENWeights :2003-2027), kept until the geometry or the loading moves
void ensure_fixed_w(dsr_sph& s)
{
  if (s.fixedWValid) return;
  static const zc IN[4] = {zc(1, 0), zc(0, 1), zc(-1, 0), zc(0, -1)};
  const int F = s.M / 2 + 1, C = s.C, D = s.dim;
  s.fixedW.assign((size_t) F * C * D, zc(0, 0));
  std::vector<zc> A((size_t) D * C), tmp((size_t) C * C), inv((size_t) C * C);
  for (int f = 1; f < F; f++) {
    for (int n = 0, idx = 0; n < s.maxOrder; n++) {
      const zc inbn = gmul(IN[n % 4], s.B[(size_t) f * s.maxOrder + n]);
      for (int m = -n; m <= n; m++, idx++)
        for (int c = 0; c < C; c++) A[(size_t) idx * C + c] = gmulr(gmul(s.SH[(size_t) idx * C + c], inbn), 4 * M_PI);
    }
    const double beta = (double) s.diag[f];                  // zherk(Upper, ConjTrans, 1, A, l, I), then the lower triangle mirrored (:2009-2013)
    for (int i = 0; i < C; i++)
      for (int j = i; j < C; j++) {
        zc acc(0, 0);
        for (int d = 0; d < D; d++) acc += gmul(std::conj(A[(size_t) d * C + i]), A[(size_t) d * C + j]);
        if (i == j) acc = zc(acc.real() + beta, 0.0);
        tmp[(size_t) i * C + j] = acc; tmp[(size_t) j * C + i] = std::conj(acc);
      }
    linpack::pseudoinverse(tmp.data(), inv.data(), C, C, 1.0E-8f);   // the result is taken whatever it returns (:2014-2025)
    zc* fw = &s.fixedW[(size_t) f * C * D];
    for (int c = 0; c < C; c++)
      for (int d = 0; d < D; d++) {
        zc acc(0, 0);
        for (int k = 0; k < C; k++) acc += gmul(inv[(size_t) c * C + k], std::conj(A[(size_t) d * C + k]));
        fw[(size_t) c * D + d] = acc;
      }
  }
  s.fixedWValid = true;
}

// SphericalMOENBeamformer::_calcWeights (:1937-2040): w [C] = CN fixedW BN, BN = 2 pi conj Y at the direction.  fixTerms(true): the reference
// frees and zeroes _fixedW before it uses it (:1993-1996, :2031-2034), so every weight is 0 (NaN with normalizeWeight: 0 times wgain / 0).
void calc_moen(const dsr_sph& s, int f, const zc* Y, zc* w)
{
  const int C = s.C, D = s.dim;
  const double CN = 2.0 / (s.maxOrder * s.maxOrder);
  for (int c = 0; c < C; c++) {
    zc acc(0, 0);
    if (!s.fixedTerms)
      for (int d = 0; d < D; d++) acc += gmul(s.fixedW[((size_t) f * C + c) * D + d], gmulr(std::conj(Y[d]), 2 * M_PI));
    w[c] = gmulr(acc, CN);
  }
  if (s.normalize) normalize_weights(w, C, s.wgain);
}

// the weights of every bin for the direction (theta, phi): modal kinds [M/2+1][dim], bin 0 the DC weights (_calcSteeringUnit :703-734);
// SpatialDS [M/2+1][C] with bin 0 computed like the others (:2244-2270); MOEN [M/2+1][C], bin 0 calcDCWeights written into the C-long
// vector: (1, 0) then zeros (the vector starts zeroed, beamformer.cc:916; only min(dim, C) entries are written here, the reference writes
// past the end when dim > C)
void dir_weights(dsr_sph& s, double theta, double phi, std::vector<zc>& W);

void harmonics_at(const dsr_sph& s, double theta, double phi, zc* Y)
{
  for (int n = 0, idx = 0; n < s.maxOrder; n++)
    for (int m = -n; m <= n; m++, idx++) Y[idx] = sph_harmonic(m, n, theta, phi);
}

void dir_weights(dsr_sph& s, double theta, double phi, std::vector<zc>& W)
{
  const int F = s.M / 2 + 1, D = s.dim, L = sensor_kind(s.kind) ? s.C : D;
  W.assign((size_t) F * L, zc(0, 0));
  std::vector<zc> Y(D); harmonics_at(s, theta, phi, Y.data());
  if (s.kind == DSR_SPH_SPATIALDS) { for (int f = 0; f < F; f++) calc_spatial_ds(s, f, Y.data(), &W[(size_t) f * L]); return; }
  W[0] = zc(1, 0);                                           // calcDCWeights: 1 for n = 0
  if (s.kind == DSR_SPH_MOEN) { ensure_fixed_w(s); for (int f = 1; f < F; f++) calc_moen(s, f, Y.data(), &W[(size_t) f * L]); return; }
  for (int f = 1; f < F; f++) calc_weights(s, f, Y.data(), &W[(size_t) f * D]);
}

void ensure_look(dsr_sph& s)                                 // _calcSteeringUnit(0): DC weights at bin 0, _calcWeights at 1..M/2
{
  ensure_modes(s);
  if (!s.lookDirty) return;
  const int F = s.M / 2 + 1, D = s.dim;
  if (gsc_kind(s.kind) && (s.NC < 1 || s.NC >= D))           // beamformerWeights allocates no B then (beamformer.cc:921-924) and calcBlockingMatrix throws
    throw Error(DSR_E_PARAMETER, "NC %d: the blocking matrix of a %d-dimensional quiescent vector needs 1 <= NC < %d", s.NC, D, D);
  dir_weights(s, s.lookTheta, s.lookPhi, s.look);
  if (gsc_kind(s.kind)) {                                    // calcBlockingMatrix per bin 1..M/2 (_calcSteeringUnit(0, isGSC) :727-729); wl stays as last set
    // _calcBlockingMatrix projects with I - conj(d) d^T / ||d||^2: its columns are orthogonal to conj(d).  The reference hands it wq itself, so
    // with the complex modal wq its B does not block wq (|B^H wq| / ||wq|| up to 0.9) and the look direction's eigenbeams, which are
    // proportional to wq, leak into the sidelobe path.  Here it gets conj(wq): B^H wq = 0, a blocking matrix in fact (a deviation).
    const int bs = D - s.NC;
    s.Bm.assign((size_t) F * D * bs, zc(0, 0));
    if (s.wl.size() != (size_t) F * D) s.wl.assign((size_t) F * D, zc(0, 0));
    std::vector<zc> cq(D);
    for (int f = 1; f < F; f++) {
      for (int d = 0; d < D; d++) cq[d] = std::conj(s.look[(size_t) f * D + d]);
      zc* B = &s.Bm[(size_t) f * D * bs];
      if (!blocking_matrix_nc(cq.data(), D, s.NC, B)) throw Error(DSR_E_ERROR, "_calcBlockingMatrix() failed");
      // its classical Gram-Schmidt loses the orthogonality to wq over many columns (1e-5 of ||wq|| over the 63 of order 8, whose wq spans 20
      // decades at the low bins): one projection of every column against wq restores it (the columns move by that much, no more)
      double n2 = 0.0;
      for (int d = 0; d < D; d++) n2 += std::norm(cq[d]);
      for (int j = 0; j < bs; j++) {
        zc ip(0, 0);
        for (int d = 0; d < D; d++) ip += cq[d] * B[(size_t) d * bs + j];           // wq^H B_j
        ip = zc(ip.real() / n2, ip.imag() / n2);
        for (int d = 0; d < D; d++) B[(size_t) d * bs + j] -= ip * std::conj(cq[d]);
      }
    }
  }
  s.lookDirty = false; s.dLookDirty = true;
}

// what the output applies: the look weights; for the GSC kinds calcOutputOfGSC's (wq - wl), with normalizeWeight divided by ||.|| dim, at bins >= 1
// (beamformer.cc:1251-1287; SphericalGSCBeamformer::next :1508-1533).  wl: null for a beam other than the look direction (no active weights).
void effective(const dsr_sph& s, const std::vector<zc>& wq, const zc* wl, std::vector<zc>& eff)
{
  eff = wq;
  if (!gsc_kind(s.kind)) return;
  const int F = s.M / 2 + 1, D = s.dim;
  for (int f = 1; f < F; f++) {
    zc* e = &eff[(size_t) f * D];
    if (wl) for (int d = 0; d < D; d++) e[d] = e[d] - wl[(size_t) f * D + d];
    if (s.normalize) {
      double ss = 0.0;
      for (int d = 0; d < D; d++) ss += std::norm(e[d]);
      const double de = std::sqrt(ss) * (unsigned) D;
      for (int d = 0; d < D; d++) e[d] = gdivr(e[d], de);
    }
  }
}

// v [F][C] = S^H w per bin for modal weights w [F][dim] (v^H x = w^H (S x)); sensor-domain weights are v already
void fold(const dsr_sph& s, const std::vector<zc>& w, zc* v)
{
  const int F = s.M / 2 + 1, D = s.dim, C = s.C;
  if (sensor_kind(s.kind)) { std::copy(w.begin(), w.end(), v); return; }
  for (int f = 0; f < F; f++) {
    zc* vf = v + (size_t) f * C;
    for (int c = 0; c < C; c++) vf[c] = zc(0, 0);
    for (int d = 0; d < D; d++) {
      const zc wd = w[(size_t) f * D + d];
      if (wd == zc(0, 0)) continue;
      const zc* sh = &s.SH[(size_t) d * C];
      for (int c = 0; c < C; c++) vf[c] += wd * std::conj(sh[c]);
    }
  }
}

void ensure_beams(dsr_sph& s, int NB)                        // V [NB][F][C]: beam 0 the look direction with the active weights, beams 1.. as set
{
  if (NB < 1 || NB > MAX_BEAMS) throw Error(DSR_E_DIMENSION, "%d beams (1..%d supported)", NB, MAX_BEAMS);
  for (int b = 1; b < NB; b++) if (!s.beamSet[b]) throw Error(DSR_E_ERROR, "beam %d of %d has no direction (dsr_sph_set_beam)", b, NB);
  ensure_look(s);
  if (s.vNB == NB && s.vSetGen == s.settingsGen && s.vBeamGen == s.beamGen) return;
  const size_t FC = (size_t) (s.M / 2 + 1) * s.C;
  s.V.assign((size_t) NB * FC, zc(0, 0));
  std::vector<zc> w, eff;
  effective(s, s.look, gsc_kind(s.kind) ? s.wl.data() : nullptr, eff);
  fold(s, eff, s.V.data());
  for (int b = 1; b < NB; b++) {
    dir_weights(s, s.beamTheta[b], s.beamPhi[b], w);
    effective(s, w, nullptr, eff);
    fold(s, eff, &s.V[(size_t) b * FC]);
  }
  s.vNB = NB; s.vSetGen = s.settingsGen; s.vBeamGen = s.beamGen; s.dVDirty = true;
}

int grid_n(double mn, double mx, double w)                   // (unsigned)((max - min) / width + 0.5) (:803-804)
{
  const double v = (mx - mn) / w + 0.5;
  return v >= 1.0 && v < 1e9 ? (int) (unsigned) v : 0;
}

void build_table(dsr_sph& s)                                 // _calcSteeringUnitTable (:793-858 / :1190-1246)
{
  if (s.tbl) return;
  if (s.kind > DSR_SPH_DS)                                   // the reference searches with the EB and DS weights only (DOAEstimatorSRPEB, DOAEstimatorSRPSphDSB)
    throw Error(DSR_E_ERROR, "kind %d has no steering table: the SRP DOA estimators exist for DSR_SPH_EB and DSR_SPH_DS only", s.kind);
  check_range(s.fbinMin, s.fbinMax, s.M, s.M / 2);
  const int nT = grid_n(s.minTheta, s.maxTheta, s.widthTheta), nP = grid_n(s.minPhi, s.maxPhi, s.widthPhi);
  if (nT >= 1 && nP >= 1 && (long) nT * nP * (s.fbinMax + 1) * std::max(s.dim, s.C) > MAX_TABLE)
    throw Error(DSR_E_DIMENSION, "search grid of %d x %d directions: the steering table of bins 0..%d would hold %ld entries, at most %ld are supported",
                nT, nP, s.fbinMax, (long) nT * nP * (s.fbinMax + 1) * std::max(s.dim, s.C), MAX_TABLE);
  if (nT < 1 || nP < 1)
    throw Error(DSR_E_PARAMETER, "search grid of %d x %d directions (theta %g..%g by %g, phi %g..%g by %g)", nT, nP, s.minTheta, s.maxTheta, s.widthTheta,
                s.minPhi, s.maxPhi, s.widthPhi);
  ensure_modes(s);
  const int nU = nT * nP, D = s.dim;
  s.uTheta.assign(nU, 0.0); s.uPhi.assign(nU, 0.0); s.W.assign((size_t) (s.fbinMax + 1) * nU * D, zc(0, 0));
  std::vector<zc> Y(D);
  int unit = 0; double theta = s.minTheta;
  for (int it = 0; it < nT; it++, theta += s.widthTheta) {   // theta and phi accumulated in double, theta-major, as the reference's loops
    double phi = s.minPhi;
    for (int ip = 0; ip < nP; ip++, phi += s.widthPhi, unit++) {
      s.uTheta[unit] = theta; s.uPhi[unit] = phi;
      harmonics_at(s, theta, phi, Y.data());
      for (int d = 0; d < D; d++) s.W[(size_t) unit * D + d] = zc(1, 0);       // bin 0: (1, 0) unless the range starts at 0
      for (int f = s.fbinMin; f <= s.fbinMax; f++) calc_weights(s, f, Y.data(), &s.W[((size_t) f * nU + unit) * D]);
    }
  }
  s.nTheta = nT; s.nPhi = nP; s.tblFbinMax = s.fbinMax; s.tbl = true; s.tableGen++; s.dWDirty = true;
}

int units(const dsr_sph& s) { return s.nTheta * s.nPhi; }

// ---- device ----

// y[u][t][f] = w_f^H (S X_f), Fo[u][t][f][d] = (S X_f)_d (optional), for t < nframes[u], f = 0..M/2
__global__ __launch_bounds__(256) void k_sph_apply(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ S,
                                                   const double2* __restrict__ Wl, int C, int Tmax, int F, int dim, float2* __restrict__ Y, float2* __restrict__ Fo)
{
  const long k = (long) blockIdx.x * blockDim.x + threadIdx.x;
  const int u = blockIdx.y;
  if (k >= (long) Tmax * F) return;
  const int t = (int) (k / F), f = (int) (k - (long) t * F);
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  if (t >= N) return;
  const float2* x = X + ((long) u * C * Tmax + t) * F + f;   // + c Tmax F
  const double2* w = Wl + (long) f * dim;
  double yr = 0.0, yi = 0.0;
  float2* fo = Fo ? Fo + (((long) u * Tmax + t) * F + f) * dim : nullptr;
  for (int d0 = 0; d0 < dim; d0 += 8) {
    double fr[8], fi[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { fr[j] = 0.0; fi[j] = 0.0; }
    for (int c = 0; c < C; c++) {
      const float2 v = x[(long) c * Tmax * F]; const double xr = v.x, xi = v.y;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (d0 + j >= dim) break;
        const double2 sc = S[(long) (d0 + j) * C + c];       // wave-uniform
        fr[j] += sc.x * xr - sc.y * xi; fi[j] += sc.x * xi + sc.y * xr;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (d0 + j >= dim) break;
      const double2 wd = w[d0 + j];                          // conj(w) F
      yr += wd.x * fr[j] + wd.y * fi[j]; yi += wd.x * fi[j] - wd.y * fr[j];
      if (fo) fo[d0 + j] = make_float2((float) fr[j], (float) fi[j]);
    }
  }
  Y[((long) u * Tmax + t) * F + f] = make_float2((float) yr, (float) yi);
}

// the fused SRP: see the file header.  Sp [DT][KS][64] (S as the A operand), Wp [F][NT][DT][4][64] (conj w in stage 2's K order)
template <int TG, int DT>
__global__ __launch_bounds__(256) void k_sph_srp(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ Sp,
                                                 const double2* __restrict__ Wp, int C, int Tmax, int F, int M2, int fbinMin, int fbinMax, int nUnits,
                                                 int NT, int KS, int BC, double* __restrict__ rpOut, float* __restrict__ energy, float2* __restrict__ Y)
{
  extern __shared__ float2 xs[];                             // [C][FB][pitch]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int th0 = blockIdx.x * TG, t0 = blockIdx.y * FB, u = blockIdx.z;
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  if (t0 >= N) return;                                       // workgroup-uniform
  const int BP = bin_pitch(BC), tw = t0 + wave * 16 + i;
  const float2* Xu = X + (long) u * C * Tmax * F;
  const bool doEnergy = blockIdx.x == 0 && threadIdx.x < FB;
  const int lastTile = (nUnits - 1) >> 4, lastRow = (nUnits - 1) & 15;
  d4 rp[TG];
#pragma unroll
  for (int g = 0; g < TG; g++) rp[g] = (d4){0.0, 0.0, 0.0, 0.0};
  float e = 0.0f;
  for (int f0 = fbinMin; f0 <= fbinMax; f0 += BC) {
    const int nb = fbinMax - f0 + 1 < BC ? fbinMax - f0 + 1 : BC;
    srp_stage_chunk(xs, Xu, C, Tmax, F, BC, BP, t0, N, f0, nb);
    if (doEnergy) e = srp_energy_chunk(xs, C, FB, BP, threadIdx.x, f0, nb, M2, e);   // calcEnergy (beamformer.cc:3043-3074)
    for (int b = 0; b < nb; b++) {
      const int f = f0 + b;
      const double g = f < M2 ? 2.0 : 1.0;
      d4 Fr[DT], Fi[DT];                                     // stage 1: the 16 frames' eigenbeams, rows 16 dt + kq + 4 q
      const float2* xb = xs + (kq * FB + wave * 16 + i) * BP + b;   // + 4 ks FB BP: channel 4 ks + kq
#pragma unroll
      for (int dt = 0; dt < DT; dt++) {
        d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
        const double2* sp = Sp + (long) dt * KS * 64 + lane;
        int ks = 0;
        for (; ks + 2 <= KS; ks += 2) {
          double2 a[2]; float2 x[2];
#pragma unroll
          for (int j = 0; j < 2; j++) { a[j] = sp[(ks + j) * 64]; x[j] = ks * 4 + 4 * j + kq < C ? xb[(ks + j) * 4 * FB * BP] : make_float2(0.f, 0.f); }
#pragma unroll
          for (int j = 0; j < 2; j++) cmfma(a[j].x, a[j].y, (double) x[j].x, (double) x[j].y, cr, ci);
        }
        for (; ks < KS; ks++) {
          const double2 a = sp[ks * 64];
          const float2 x = ks * 4 + kq < C ? xb[ks * 4 * FB * BP] : make_float2(0.f, 0.f);
          cmfma(a.x, a.y, (double) x.x, (double) x.y, cr, ci);
        }
        Fr[dt] = cr; Fi[dt] = ci;
      }
#pragma unroll
      for (int tg = 0; tg < TG; tg++) {                      // stage 2: 16 units a tile, K = dim in the permuted order
        const int th = th0 + tg;
        if (th >= NT) break;                                 // uniform
        d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
        const double2* wp = Wp + ((long) f * NT + th) * DT * 256 + lane;
#pragma unroll
        for (int dt = 0; dt < DT; dt++) {
          double2 a[4];
#pragma unroll
          for (int q = 0; q < 4; q++) a[q] = wp[(dt * 4 + q) * 64];
#pragma unroll
          for (int q = 0; q < 4; q++) cmfma(a[q].x, a[q].y, Fr[dt][q], Fi[dt][q], cr, ci);
        }
        srp_accumulate(rp[tg], cr, ci, g, Y, th == lastTile, lastRow, kq, tw < N, (long) u * Tmax + tw, F, f);
      }
    }
  }
  srp_write_rp(rp, th0, NT, kq, nUnits, tw < N, (long) u * Tmax + tw, fbinMin, fbinMax, rpOut);
  if (doEnergy && t0 + (int) threadIdx.x < N) energy[(long) u * Tmax + t0 + threadIdx.x] = srp_energy_final(e, M2, C);
}

// true when (r, k) ranks before (br, bk): rp descending, unit ascending
__device__ __forceinline__ bool ahead(double r, int k, double br, int bk) { return r > br || (r == br && k < bk); }

// per frame, one wave: gate + N-best of the frame (next :892-947); nbIdx -1 = an empty rank (rp -10e10, DOA (-pi, -pi))
__global__ __launch_bounds__(256) void k_sph_frame(const double* __restrict__ rp, const float* __restrict__ energy, const int* __restrict__ nframes, int U,
                                                   int Tmax, int nUnits, int nBest, float thr, double* __restrict__ nbRp, int* __restrict__ nbIdx,
                                                   int* __restrict__ gated)
{
  const long k = (long) blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= (long) U * Tmax) return;                          // wave-uniform
  const int u = (int) (k / Tmax), t = (int) (k - (long) u * Tmax);
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  if (t >= N) return;
  const bool gate = energy[k] < thr;
  if (gated && lane == 0) gated[k] = gate ? 1 : 0;
  const double* r = rp + k * nUnits;
  double pr = INFINITY; int pk = -1; bool done = gate;
  for (int n = 0; n < nBest; n++) {
    double br = -INFINITY; int bk = 0x7fffffff;
    if (!done) {
      for (int j = lane; j < nUnits; j += 64) {
        const double v = r[j];
        if (ahead(pr, pk, v, j) && ahead(v, j, br, bk)) { br = v; bk = j; }   // after the previous rank, before the best so far
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double orr = __shfl_xor(br, o); const int ok = __shfl_xor(bk, o);
        if (ahead(orr, ok, br, bk)) { br = orr; bk = ok; }
      }
      if (bk == 0x7fffffff) done = true;
    }
    if (lane == 0) { nbRp[k * nBest + n] = done ? -10e10 : br; nbIdx[k * nBest + n] = done ? -1 : bk; }
    pr = br; pk = bk;
  }
}

// Y[u][b][t][f] = sum_c Vc[c][b][f] X[u][c][t][f] for NB beams (Vc = conj v, [C][NB][F]); one thread per E elements k = t F + f of a channel's
// contiguous (t, f) plane, so the float2 loads are coalesced whatever F is.  sv: conj(v) of CC channels at a time, [CC][NB][F].  Rows from
// nframes[u] on are written as zeros.
template <int NB, int E>
__global__ __launch_bounds__(256) void k_sph_beams_valu(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ Vc,
                                                        int C, int Tmax, int F, int CC, int nbOut, float2* __restrict__ Y)
{
  extern __shared__ double2 sv[];
  const int u = blockIdx.y, tid = threadIdx.x;
  int N = nframes[u]; if (N > Tmax) N = Tmax; if (N < 0) N = 0;
  const long TF = (long) Tmax * F, live = (long) N * F, base = (long) blockIdx.x * (256 * E);
  double yr[E][NB], yi[E][NB]; int fe[E]; long ke[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    ke[e] = base + e * 256 + tid; fe[e] = (int) (ke[e] % F);
#pragma unroll
    for (int b = 0; b < NB; b++) { yr[e][b] = 0.0; yi[e][b] = 0.0; }
  }
  if (base < live) {                                         // workgroup-uniform
    const float2* Xu = X + (long) u * C * TF;
    for (int c0 = 0; c0 < C; c0 += CC) {
      const int nc = C - c0 < CC ? C - c0 : CC;
      __syncthreads();
      for (int idx = tid; idx < nc * NB * F; idx += 256) sv[idx] = Vc[(long) c0 * NB * F + idx];
      __syncthreads();
      for (int cc = 0; cc < nc; cc++) {
        float2 x[E];
#pragma unroll
        for (int e = 0; e < E; e++) x[e] = ke[e] < live ? Xu[(long) (c0 + cc) * TF + ke[e]] : make_float2(0.f, 0.f);
#pragma unroll
        for (int e = 0; e < E; e++) {
          const double xr = x[e].x, xi = x[e].y;
#pragma unroll
          for (int b = 0; b < NB; b++) {
            const double2 v = sv[(cc * NB + b) * F + fe[e]];
            yr[e][b] += v.x * xr - v.y * xi; yi[e][b] += v.x * xi + v.y * xr;
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; e++) {
    if (ke[e] >= TF) continue;
#pragma unroll
    for (int b = 0; b < NB; b++)
      if (b < nbOut) Y[((long) u * nbOut + b) * TF + ke[e]] = make_float2((float) yr[e][b], (float) yi[e][b]);
  }
}

// the same as one complex GEMM per bin on v_mfma_f64_16x16x4_f64: the staging and operand layout of k_doa_srp with one row tile (the beams, zero
// padded to 16), Vp [F][KS][64] = conj v as the A operand; result register q of lane l is beam (l >> 4) + 4 q of frame l & 15.  A chunk's results
// are kept as float2 and stored a beam row at a time (consecutive bins of one frame).  Frames from nframes[u] on are staged as zeros.
template <int BCT>
__global__ __launch_bounds__(256) void k_sph_beams_mfma(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ Vp,
                                                        int C, int Tmax, int F, int NB, int KS, float2* __restrict__ Y)
{
  extern __shared__ float2 xs[];                             // [C][FB][pitch]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int t0 = blockIdx.x * FB, u = blockIdx.y;
  int N = nframes[u]; if (N > Tmax) N = Tmax; if (N < 0) N = 0;
  const int BP = bin_pitch(BCT), tw = t0 + wave * 16 + i;
  const float2* Xu = X + (long) u * C * Tmax * F;
  if (t0 >= N) {                                             // workgroup-uniform: nothing to read, the rows are zero
    const int nt = Tmax - t0 < FB ? Tmax - t0 : FB;
    for (int b = 0; b < NB; b++)
      for (int idx = threadIdx.x; idx < nt * F; idx += 256) Y[(((long) u * NB + b) * Tmax + t0) * F + idx] = make_float2(0.f, 0.f);
    return;
  }
  for (int f0 = 0; f0 < F; f0 += BCT) {
    const int nb = F - f0 < BCT ? F - f0 : BCT;
    srp_stage_chunk(xs, Xu, C, Tmax, F, BCT, BP, t0, N, f0, nb);
    float2 out[BCT][4];
#pragma unroll
    for (int b = 0; b < BCT; b++) {
      d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
      if (b < nb) {                                          // uniform
        const double2* vp = Vp + (long) (f0 + b) * KS * 64 + lane;   // lane: conj(v[beam = l & 15][c = 4 ks + (l >> 4)])
        const float2* xb = xs + (kq * FB + wave * 16 + i) * BP + b;  // + 4 ks FB BP: channel 4 ks + (l >> 4)
        int ks = 0;
        for (; ks + 4 <= KS; ks += 4) {
          double2 a[4]; float2 x[4];
#pragma unroll
          for (int j = 0; j < 4; j++) { a[j] = vp[(ks + j) * 64]; x[j] = ks * 4 + 4 * j + kq < C ? xb[(ks + j) * 4 * FB * BP] : make_float2(0.f, 0.f); }
#pragma unroll
          for (int j = 0; j < 4; j++) cmfma(a[j].x, a[j].y, (double) x[j].x, (double) x[j].y, cr, ci);
        }
        for (; ks < KS; ks++) {
          const double2 a = vp[ks * 64];
          const float2 x = ks * 4 + kq < C ? xb[ks * 4 * FB * BP] : make_float2(0.f, 0.f);
          cmfma(a.x, a.y, (double) x.x, (double) x.y, cr, ci);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) out[b][q] = make_float2((float) cr[q], (float) ci[q]);
    }
    if (tw < Tmax) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int beam = kq + 4 * q;
        if (beam >= NB) continue;
        float2* y = Y + (((long) u * NB + beam) * Tmax + tw) * F + f0;
#pragma unroll
        for (int b = 0; b < BCT; b++) if (b < nb) y[b] = out[b][q];
      }
    }
  }
}

int beams_bin_chunk(int C)                                   // the staged chunk's bins: the power of two <= 8 whose rows fit (srp_common.h: bin_chunk)
{
  const int BC = bin_chunk(C);
  return BC > 8 ? 8 : BC;
}

int beams_path(int NB)                                       // 0 VALU (NB <= 4), 1 MFMA; DSR_SPH_BEAMS_PATH=valu|mfma forces one (measurements)
{
  const char* e = getenv("DSR_SPH_BEAMS_PATH");
  if (e && *e) {
    if (!strcmp(e, "valu")) return 0;
    if (!strcmp(e, "mfma")) return 1;
    throw Error(DSR_E_PARAMETER, "DSR_SPH_BEAMS_PATH=%s: valu or mfma", e);
  }
  return NB <= 4 ? 0 : 1;
}

constexpr size_t BEAMS_LDS = 48 * 1024;                      // the VALU kernel's staged conj(v): CC channels x NBT beams x F bins

template <int NBT, int E>
void launch_beams_valu(const dsr_sph& s, const float* X, const int* nf, int U, int Tmax, int NB, float* Y, hipStream_t st)
{
  const int F = s.M / 2 + 1;
  int CC = (int) (BEAMS_LDS / ((size_t) NBT * F * sizeof(double2))); if (CC > s.C) CC = s.C;
  if (CC < 1) throw Error(DSR_E_DIMENSION, "%d beams x %d bins do not fit the kernel's %zu bytes of LDS", NBT, F, BEAMS_LDS);
  const size_t lds = (size_t) CC * NBT * F * sizeof(double2);
  launch(k_sph_beams_valu<NBT, E>, dim3(cdiv((long) Tmax * F, 256 * E), U), dim3(256), lds, st, (const float2*) X, nf, s.dV.p, s.C, Tmax, F, CC, NB,
                     (float2*) Y);
}

template <int BCT>
void launch_beams_mfma(const dsr_sph& s, const float* X, const int* nf, int U, int Tmax, int NB, float* Y, hipStream_t st)
{
  const size_t lds = (size_t) s.C * FB * bin_pitch(BCT) * sizeof(float2);
  launch(k_sph_beams_mfma<BCT>, dim3((Tmax + FB - 1) / FB, U), dim3(256), lds, st, (const float2*) X, nf, s.dV.p, s.C, Tmax, s.M / 2 + 1, NB,
                     (s.C + 3) / 4, (float2*) Y);
}

int valu_rows(int NB) { return NB <= 4 ? NB : NB <= 8 ? 8 : 16; }   // the VALU kernel's instantiations: 1..4 exact, above that zero-padded rows

// the kernel of one call: beams_path, but where one channel of the VALU kernel's staged table (rows x F bins) is more than its LDS holds -- rows F
// > 3072: fftLen 2048 with 3 or 4 beams, fftLen >= 6144 with one -- the MFMA kernel, which stages snapshots and has no such limit, takes the call
// (a forced DSR_SPH_BEAMS_PATH=valu is left to fail with DSR_E_DIMENSION: it is for measurements)
int beams_path_for(int NB, int F)
{
  const int path = beams_path(NB);
  if (path == 0 && (size_t) valu_rows(NB) * F * sizeof(double2) > BEAMS_LDS && !getenv("DSR_SPH_BEAMS_PATH")) return 1;
  return path;
}

void upload_beams(dsr_sph& s, int NB, int path, hipStream_t st)   // conj(v): layout 0 [F][KS][64] (MFMA A operand), n > 0 [C][n][F] (VALU, n rows)
{
  const int layout = path == 1 ? 0 : valu_rows(NB);
  if (!s.dVDirty && s.dVLayout == layout) return;
  const int F = s.M / 2 + 1, C = s.C, KS = (C + 3) / 4;
  std::vector<double2> h;
  if (layout == 0) {
    h.assign((size_t) F * KS * 64, make_double2(0.0, 0.0));
    for (int f = 0; f < F; f++)
      for (int ks = 0; ks < KS; ks++)
        for (int l = 0; l < 64; l++) {
          const int b = l & 15, c = ks * 4 + (l >> 4);
          if (b >= NB || c >= C) continue;
          const zc v = s.V[((size_t) b * F + f) * C + c];
          h[((size_t) f * KS + ks) * 64 + l] = make_double2(v.real(), -v.imag());
        }
  } else {
    h.assign((size_t) C * layout * F, make_double2(0.0, 0.0));
    for (int c = 0; c < C; c++)
      for (int b = 0; b < NB; b++)
        for (int f = 0; f < F; f++) {
          const zc v = s.V[((size_t) b * F + f) * C + c];
          h[((size_t) c * layout + b) * F + f] = make_double2(v.real(), -v.imag());
        }
  }
  s.dV.upload(h, st); s.dVLayout = layout; s.dVDirty = false;
}

int pattern_n(double mn, double mx, double w)                // (int)(float)((max - min) / width + 0.5 + 1) (:759-766)
{
  const float n = (float) ((mx - mn) / w + 0.5 + 1);
  return n >= 1.0f && n < 1e6f ? (int) n : 0;
}

const char* forced_path()
{
  const char* e = getenv("DSR_SPH_SRP_PATH");
  return e && *e ? e : nullptr;
}

int pick_path(const dsr_sph& s)                              // 0 fused, 1 folded: folded when dim (C + units) >= C units
{
  if (const char* e = forced_path()) {
    if (!strcmp(e, "fused")) return 0;
    if (!strcmp(e, "folded")) return 1;
    throw Error(DSR_E_PARAMETER, "DSR_SPH_SRP_PATH=%s: fused or folded", e);
  }
  const long nU = units(s);
  return (long) s.dim * (s.C + nU) >= (long) s.C * nU ? 1 : 0;
}

void upload_s(dsr_sph& s, hipStream_t st)                    // S [dim][C] (apply) and Sp [DT][KS][64] (the fused kernel's A operand)
{
  if (!s.dSDirty) return;
  const int D = s.dim, C = s.C; s.DT = D <= 16 ? 1 : D <= 32 ? 2 : 4; s.KS = (C + 3) / 4;   // the kernel's dim tiles: 1, 2 or 4 (rows past dim zero)
  std::vector<double2> h((size_t) D * C), hp((size_t) s.DT * s.KS * 64, make_double2(0.0, 0.0));
  for (int d = 0; d < D; d++)
    for (int c = 0; c < C; c++) h[(size_t) d * C + c] = make_double2(s.SH[(size_t) d * C + c].real(), s.SH[(size_t) d * C + c].imag());
  for (int dt = 0; dt < s.DT; dt++)
    for (int ks = 0; ks < s.KS; ks++)
      for (int l = 0; l < 64; l++) {
        const int d = dt * 16 + (l & 15), c = ks * 4 + (l >> 4);
        if (d < D && c < C) hp[((size_t) dt * s.KS + ks) * 64 + l] = h[(size_t) d * C + c];
      }
  s.dS.upload(h, st); s.dSp.upload(hp, st); s.dSDirty = false;
}

void upload_fused_table(dsr_sph& s, hipStream_t st)
{
  if (!s.dWDirty) return;
  const int F = s.M / 2 + 1, D = s.dim, nU = units(s); s.NT = (nU + 15) / 16;
  const int DT4 = s.DT;
  std::vector<double2> h((size_t) F * s.NT * DT4 * 256, make_double2(0.0, 0.0));
  for (int f = 0; f <= s.tblFbinMax; f++)
    for (int th = 0; th < s.NT; th++)
      for (int dt = 0; dt < DT4; dt++)
        for (int q = 0; q < 4; q++)
          for (int l = 0; l < 64; l++) {
            const int k = th * 16 + (l & 15), d = dt * 16 + (l >> 4) + 4 * q;
            if (k >= nU || d >= D) continue;
            const zc w = s.W[((size_t) f * nU + k) * D + d];
            h[((((size_t) f * s.NT + th) * DT4 + dt) * 4 + q) * 64 + l] = make_double2(w.real(), -w.imag());
          }
  s.dWp.upload(h, st); s.dWDirty = false;
}

void prepare_fold(dsr_sph& s)                                // v[f][unit][c] = sum_d w[f][unit][d] conj(S[d][c]): v^H X = w^H (S X)
{
  dsr_doa& q = s.fold;
  q.C = s.C; q.M = s.M; q.fbinMin = s.fbinMin; q.fbinMax = s.fbinMax; q.threshold = s.threshold; q.nBest = s.nBest;
  if (s.foldGen == s.tableGen) return;
  const int nU = units(s), D = s.dim, C = s.C;
  q.W.assign((size_t) (s.tblFbinMax + 1) * nU * C, zc(0, 0));
  for (int f = 0; f <= s.tblFbinMax; f++)
    for (int k = 0; k < nU; k++) {
      const zc* w = &s.W[((size_t) f * nU + k) * D];
      zc* v = &q.W[((size_t) f * nU + k) * C];
      for (int d = 0; d < D; d++) {
        if (w[d] == zc(0, 0)) continue;
        const zc* sh = &s.SH[(size_t) d * C];
        for (int c = 0; c < C; c++) v[c] += w[d] * std::conj(sh[c]);
      }
    }
  q.nTheta = nU; q.tblFbinMax = s.tblFbinMax; q.tbl = true; q.dDirty = true; s.foldGen = s.tableGen;
}

template <int TG, int DT>
void launch_fused(const dsr_sph& s, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st)
{
  const int BC = bin_chunk(s.C), F = s.M / 2 + 1;
  const size_t lds = (size_t) s.C * FB * bin_pitch(BC) * sizeof(float2);
  dim3 grid((s.NT + TG - 1) / TG, (Tmax + FB - 1) / FB, U);
  launch(k_sph_srp<TG, DT>, grid, dim3(256), lds, st, (const float2*) X, nf, s.dSp.p, s.dWp.p, s.C, Tmax, F, s.M / 2, s.fbinMin, s.fbinMax,
                     units(s), s.NT, s.KS, BC, rp, en, (float2*) Y);
}

template <int DT>
void launch_fused_tg(const dsr_sph& s, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st)
{
  if (s.NT >= 8) launch_fused<8, DT>(s, X, nf, U, Tmax, rp, en, Y, st);
  else if (s.NT >= 4) launch_fused<4, DT>(s, X, nf, U, Tmax, rp, en, Y, st);
  else if (s.NT >= 2) launch_fused<2, DT>(s, X, nf, U, Tmax, rp, en, Y, st);
  else launch_fused<1, DT>(s, X, nf, U, Tmax, rp, en, Y, st);
}

void set_geometry(dsr_sph& s, double a, const double* th, const double* ph, int n)
{
  if (n != s.C) throw Error(DSR_E_DIMENSION, "the array geometry has %d sensors, the beamformer %d channels", n, s.C);
  if (!(a > 0.0)) throw Error(DSR_E_ERROR, "radius %g of the rigid sphere must be positive", a);
  s.a = a; s.thS.assign(th, th + n); s.phS.assign(ph, ph + n);
  s.SH.assign((size_t) s.dim * s.C, zc(0, 0));               // _calcSphericalHarmonicsAtEachPosition: conj Y at every sensor
  for (int n_ = 0, idx = 0; n_ < s.maxOrder; n_++)
    for (int m = -n_; m <= n_; m++, idx++)
      for (int c = 0; c < s.C; c++) s.SH[(size_t) idx * s.C + c] = std::conj(sph_harmonic(m, n_, th[c], ph[c]));
  s.B.clear(); s.lookDirty = true; s.dSDirty = true; s.foldGen = ~0u; s.fixedWValid = false; s.settingsGen++;   // a new radius: new mode amplitudes (the table is not rebuilt)
}

}  // namespace

extern "C" {

dsr_status dsr_sph_create(int kind, int nBest, int sampleRate, int fftLen, int halfBandShift, int NC, int maxOrder, int normalizeWeight, int chanN, dsr_sph** out)
{
  return guard([&] {                                         // NC: beamformerWeights' number of constraints, used by the GSC kinds' blocking matrix only
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < DSR_SPH_EB || kind > DSR_SPH_MOEN) throw Error(DSR_E_PARAMETER, "kind %d (DSR_SPH_EB .. DSR_SPH_MOEN)", kind);
    if (halfBandShift) throw Error(DSR_E_PARAMETER, "_halfBandShift == true is not implemented yet");    // modalBeamformer.cc:391-394
    if (nBest < 1) throw Error(DSR_E_PARAMETER, "nBest %d < 1", nBest);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_PARAMETER, "fftLen %d", fftLen);
    if (sampleRate <= 0) throw Error(DSR_E_PARAMETER, "sampleRate %d", sampleRate);
    if (chanN < 1 || chanN > 128) throw Error(DSR_E_DIMENSION, "%d channels (1..128 supported)", chanN);
    if (maxOrder < 1 || maxOrder > MAX_ORDER) throw Error(DSR_E_DIMENSION, "maxOrder %d: 1..%d supported (dim = maxOrder^2 <= %d)", maxOrder, MAX_ORDER, MAX_ORDER * MAX_ORDER);
    dsr_sph* s = new dsr_sph(); s->kind = kind; s->nBest = nBest; s->sampleRate = (unsigned) sampleRate; s->M = fftLen; s->C = chanN;
    s->maxOrder = maxOrder; s->dim = maxOrder * maxOrder; s->normalize = normalizeWeight != 0; s->fbinMax = fftLen / 2;
    s->NC = NC; s->diag.assign((size_t) fftLen / 2 + 1, 0.0f);
    *out = s;
  });
}
void dsr_sph_destroy(dsr_sph* s) { delete s; }
int dsr_sph_kind(const dsr_sph* s) { return s ? s->kind : -1; }
int dsr_sph_nbest(const dsr_sph* s) { return s ? s->nBest : 0; }
int dsr_sph_chan_n(const dsr_sph* s) { return s ? s->C : 0; }
int dsr_sph_fft_len(const dsr_sph* s) { return s ? s->M : 0; }
int dsr_sph_dim(const dsr_sph* s) { return s ? s->dim : 0; }
int dsr_sph_max_order(const dsr_sph* s) { return s ? s->maxOrder : 0; }
unsigned dsr_sph_table_generation(const dsr_sph* s) { return s ? s->tableGen : 0u; }
int dsr_sph_has_table(const dsr_sph* s) { return s && s->tbl ? 1 : 0; }
unsigned dsr_sph_settings_generation(const dsr_sph* s) { return s ? s->settingsGen : 0u; }

dsr_status dsr_sph_set_array_geometry(dsr_sph* s, double a, const double* theta_s, const double* phi_s, int n)
{
  return guard([&] {
    if (!s || !theta_s || !phi_s) throw Error(DSR_E_PARAMETER, "null argument");
    set_geometry(*s, a, theta_s, phi_s, n);
  });
}
dsr_status dsr_sph_set_eigenmike_geometry(dsr_sph* s)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    double th[32], ph[32];
    for (int i = 0; i < 32; i++) { th[i] = EM_THETA[i] * M_PI / 180; ph[i] = EM_PHI[i] * M_PI / 180; }
    set_geometry(*s, 42, th, ph, 32);
  });
}
dsr_status dsr_sph_array_geometry(const dsr_sph* s, int type, double* out, int n)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    need_geometry(*s);
    if (n < s->C) throw Error(DSR_E_DIMENSION, "room for %d sensors, the geometry has %d", n, s->C);
    const std::vector<double>& v = type == 0 ? s->thS : s->phS;
    std::copy(v.begin(), v.end(), out);
  });
}
double dsr_sph_radius(const dsr_sph* s) { return s ? s->a : 0.0; }
dsr_status dsr_sph_set_look_direction(dsr_sph* s, double theta, double phi)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    s->lookTheta = theta; s->lookPhi = phi; s->lookDirty = true; s->lookSet = true; s->settingsGen++;   // (the reference warns when theta is outside [0, pi] and goes on)
  });
}
dsr_status dsr_sph_set_sigma2(dsr_sph* s, float sigma2)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->sigma2 = sigma2; s->lookDirty = true; s->settingsGen++; }); }
dsr_status dsr_sph_set_weight_gain(dsr_sph* s, float wgain)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->wgain = wgain; s->lookDirty = true; s->settingsGen++; }); }

dsr_status dsr_sph_mode_amplitudes(dsr_sph* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    ensure_modes(*s);
    if (outDoubles < s->B.size() * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, s->B.size() * 2);
    for (size_t i = 0; i < s->B.size(); i++) { out[2 * i] = s->B[i].real(); out[2 * i + 1] = s->B[i].imag(); }
  });
}
dsr_status dsr_sph_harmonics(dsr_sph* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    need_geometry(*s);
    if (outDoubles < s->SH.size() * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, s->SH.size() * 2);
    for (size_t i = 0; i < s->SH.size(); i++) { out[2 * i] = s->SH[i].real(); out[2 * i + 1] = s->SH[i].imag(); }
  });
}
dsr_status dsr_sph_look_weights(dsr_sph* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (sensor_kind(s->kind)) throw Error(DSR_E_ERROR, "this kind's weights are in the sensor domain (dsr_sph_sensor_weights)");
    ensure_look(*s);
    if (outDoubles < s->look.size() * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, s->look.size() * 2);
    for (size_t i = 0; i < s->look.size(); i++) { out[2 * i] = s->look[i].real(); out[2 * i + 1] = s->look[i].imag(); }
  });
}
dsr_status dsr_sph_calc_wng(dsr_sph* s, double* out, int n)
{
  return guard([&] {                                        // SphericalDSBeamformer::calcWNG (:997-1020)
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    ensure_modes(*s);
    const int F = s->M / 2 + 1;
    if (n < F) throw Error(DSR_E_DIMENSION, "room for %d bins, %d needed", n, F);
    const double norm = s->C / (M_PI * M_PI);
    for (int f = 0; f < F; f++) {
      if (hwnc(s->kind)) { out[f] = hwnc_wng(*s, f); continue; }   // SphericalHWNCBeamformer::calcWNG (:1397-1418)
      double val = 0;
      for (int o = 0; o < s->maxOrder; o++) val += (2 * o + 1) * std::norm(s->B[(size_t) f * s->maxOrder + o]);
      out[f] = val * val * norm;
    }
  });
}

dsr_status dsr_sph_set_search_param(dsr_sph* s, double minTheta, double maxTheta, double minPhi, double maxPhi, double widthTheta, double widthPhi)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!(widthTheta > 0.0) || !(widthPhi > 0.0)) throw Error(DSR_E_PARAMETER, "widths %g, %g must be positive", widthTheta, widthPhi);
    s->minTheta = minTheta; s->maxTheta = maxTheta; s->minPhi = minPhi; s->maxPhi = maxPhi; s->widthTheta = widthTheta; s->widthPhi = widthPhi;   // no swap
    s->tbl = false; s->uTheta.clear(); s->uPhi.clear(); s->W.clear(); s->nTheta = s->nPhi = 0;   // clearTable
  });
}
dsr_status dsr_sph_set_frequency_range(dsr_sph* s, int fbinMin, int fbinMax)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (fbinMin < 0 || fbinMin > fbinMax || fbinMax > s->M / 2) throw Error(DSR_E_DIMENSION, "frequency range [%d, %d] outside [0, %d]", fbinMin, fbinMax, s->M / 2);
    s->fbinMin = fbinMin; s->fbinMax = fbinMax;
  });
}
dsr_status dsr_sph_frequency_range(const dsr_sph* s, int* fbinMin, int* fbinMax)
{ return guard([&] { if (!s || !fbinMin || !fbinMax) throw Error(DSR_E_PARAMETER, "null argument"); *fbinMin = s->fbinMin; *fbinMax = s->fbinMax; }); }
dsr_status dsr_sph_set_energy_threshold(dsr_sph* s, float threshold)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->threshold = threshold; }); }
float dsr_sph_energy_threshold(const dsr_sph* s) { return s ? s->threshold : 0.0f; }

dsr_status dsr_sph_grid_n(dsr_sph* s, int* nTheta, int* nPhi)
{
  return guard([&] {
    if (!s || !nTheta || !nPhi) throw Error(DSR_E_PARAMETER, "null argument");
    *nTheta = s->tbl ? s->nTheta : grid_n(s->minTheta, s->maxTheta, s->widthTheta);
    *nPhi = s->tbl ? s->nPhi : grid_n(s->minPhi, s->maxPhi, s->widthPhi);
  });
}
dsr_status dsr_sph_grid(dsr_sph* s, double* theta, double* phi, int n)
{
  return guard([&] {
    if (!s || !theta || !phi) throw Error(DSR_E_PARAMETER, "null argument");
    const int nT = s->tbl ? s->nTheta : grid_n(s->minTheta, s->maxTheta, s->widthTheta), nP = s->tbl ? s->nPhi : grid_n(s->minPhi, s->maxPhi, s->widthPhi);
    if (n < nT * nP) throw Error(DSR_E_DIMENSION, "room for %d units, the grid has %d", n, nT * nP);
    int k = 0; double th = s->minTheta;
    for (int it = 0; it < nT; it++, th += s->widthTheta) {
      double ph = s->minPhi;
      for (int ip = 0; ip < nP; ip++, ph += s->widthPhi, k++) { theta[k] = th; phi[k] = ph; }
    }
  });
}
dsr_status dsr_sph_build_table(dsr_sph* s)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); build_table(*s); }); }
dsr_status dsr_sph_steering(dsr_sph* s, int unit, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    build_table(*s);
    const int nU = units(*s), F = s->M / 2 + 1, D = s->dim;
    if (unit < 0 || unit >= nU) throw Error(DSR_E_INDEX, "unit %d of %d", unit, nU);
    if (outDoubles < (size_t) F * D * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %d needed", outDoubles, F * D * 2);
    for (int f = 0; f < F; f++)
      for (int d = 0; d < D; d++) {
        const zc w = f <= s->tblFbinMax ? s->W[((size_t) f * nU + unit) * D + d] : zc(0, 0);
        out[((size_t) f * D + d) * 2] = w.real(); out[((size_t) f * D + d) * 2 + 1] = w.imag();
      }
  });
}
int dsr_sph_srp_path(dsr_sph* s)
{
  if (!s) return -1;
  if (!s->tbl) { if (dsr_sph_build_table(s)) return -1; }
  try { return pick_path(*s); } catch (const Error& e) { set_last_error(e.msg); return -1; }
}

dsr_status dsr_sph_apply(dsr_sph* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* Y_dev, float* F_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !nframes_dev || !Y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "U %d, Tmax %d", U, Tmax);
    if (sensor_kind(s->kind) && !F_dev) throw Error(DSR_E_ERROR, "this kind has no eigenbeam weights: dsr_sph_beams computes its output");
    ensure_look(*s);
    require_device();
    if (U == 0 || Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    upload_s(*s, st);
    if (s->dLookDirty) {                                     // the GSC kinds: (wq - wl); the sensor-domain kinds: zeros (Y_dev is then only a by-product of F_dev)
      std::vector<zc> eff;
      if (sensor_kind(s->kind)) eff.assign((size_t) (s->M / 2 + 1) * s->dim, zc(0, 0));
      else effective(*s, s->look, gsc_kind(s->kind) ? s->wl.data() : nullptr, eff);
      std::vector<double2> h(eff.size());
      for (size_t i = 0; i < h.size(); i++) h[i] = make_double2(eff[i].real(), eff[i].imag());
      s->dLook.upload(h, st); s->dLookDirty = false;
    }
    const int F = s->M / 2 + 1;
    if ((long) Tmax * F > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "Tmax %d x %d bins", Tmax, F);
    launch(k_sph_apply, dim3(cdiv((long) Tmax * F, 256), U), dim3(256), 0, st, (const float2*) X_dev, nframes_dev, s->dS.p, s->dLook.p,
                       s->C, Tmax, F, s->dim, (float2*) Y_dev, (float2*) F_dev);
  });
}

dsr_status dsr_sph_set_wng(dsr_sph* s, float ratio)
{
  return guard([&] {                                        // setWNG (modalBeamformer.h:329); the weights follow at once, as with set_sigma2
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!hwnc(s->kind)) throw Error(DSR_E_ERROR, "setWNG: not a SphericalHWNC(GSC)Beamformer");
    s->ratio = ratio; s->lookDirty = true; s->settingsGen++;
  });
}
dsr_status dsr_sph_set_active_weights_f(dsr_sph* s, unsigned fbinX, const double* packed, size_t n)
{
  return guard([&] {                                        // setActiveWeights_f (:1586-1594) -> calcSidelobeCancellerP_f (beamformer.cc:761-783)
    if (!s || !packed) throw Error(DSR_E_PARAMETER, "null argument");
    if (!gsc_kind(s->kind)) throw Error(DSR_E_ERROR, "setActiveWeights_f: not a Spherical(HWNC)GSCBeamformer");
    if (!s->lookSet) throw Error(DSR_E_ERROR, "call setLookDirection() once");
    ensure_look(*s);
    const int D = s->dim, bs = D - s->NC;
    if (n != (size_t) 2 * bs) throw Error(DSR_E_DIMENSION, "the size of an active weight vector must be %d but it is %zu", 2 * bs, n);
    if (fbinX > (unsigned) s->M / 2) throw Error(DSR_E_DIMENSION, "Must be a frequency bin %u <= %d", fbinX, s->M / 2);
    std::vector<zc> wa(bs);
    for (int c = 0; c < bs; c++) wa[c] = zc(packed[2 * c], packed[2 * c + 1]);
    sidelobe_wl(&s->Bm[(size_t) fbinX * D * bs], wa.data(), D, bs, &s->wl[(size_t) fbinX * D]);
    s->dLookDirty = true; s->settingsGen++;
  });
}
dsr_status dsr_sph_set_diagonal_loading(dsr_sph* s, unsigned fbinX, float diagonalWeight)
{
  return guard([&] {                                        // setLevelOfDiagonalLoading (:1923-1930); the reference only prints for a bin beyond fftLen/2
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (s->kind != DSR_SPH_MOEN) throw Error(DSR_E_ERROR, "setLevelOfDiagonalLoading: not a SphericalMOENBeamformer");
    if (fbinX > (unsigned) s->M / 2) throw Error(DSR_E_DIMENSION, "Invalid freq. bin %u (0..%d)", fbinX, s->M / 2);
    s->diag[fbinX] = diagonalWeight; s->fixedWValid = false; s->lookDirty = true; s->settingsGen++;
  });
}
dsr_status dsr_sph_fix_terms(dsr_sph* s, int flag)
{
  return guard([&] {                                        // fixTerms (modalBeamformer.h:443)
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (s->kind != DSR_SPH_MOEN) throw Error(DSR_E_ERROR, "fixTerms: not a SphericalMOENBeamformer");
    s->fixedTerms = flag != 0; s->lookDirty = true; s->settingsGen++;
  });
}
dsr_status dsr_sph_wl(dsr_sph* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (!gsc_kind(s->kind)) throw Error(DSR_E_ERROR, "not a Spherical(HWNC)GSCBeamformer");
    ensure_look(*s);
    if (outDoubles < s->wl.size() * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, s->wl.size() * 2);
    for (size_t i = 0; i < s->wl.size(); i++) { out[2 * i] = s->wl[i].real(); out[2 * i + 1] = s->wl[i].imag(); }
  });
}
dsr_status dsr_sph_blocking_matrix(dsr_sph* s, unsigned fbinX, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (!gsc_kind(s->kind)) throw Error(DSR_E_ERROR, "not a Spherical(HWNC)GSCBeamformer");
    ensure_look(*s);
    const size_t n = (size_t) s->dim * (s->dim - s->NC);
    if (fbinX > (unsigned) s->M / 2) throw Error(DSR_E_DIMENSION, "frequency bin %u (0..%d)", fbinX, s->M / 2);
    if (outDoubles < n * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, n * 2);
    const zc* B = &s->Bm[(size_t) fbinX * n];
    for (size_t i = 0; i < n; i++) { out[2 * i] = B[i].real(); out[2 * i + 1] = B[i].imag(); }
  });
}
dsr_status dsr_sph_set_beam(dsr_sph* s, int b, double theta, double phi)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (b < 0 || b >= MAX_BEAMS) throw Error(DSR_E_DIMENSION, "beam %d (0..%d)", b, MAX_BEAMS - 1);
    if (b == 0) { s->lookTheta = theta; s->lookPhi = phi; s->lookDirty = true; s->lookSet = true; s->settingsGen++; return; }
    s->beamTheta[b] = theta; s->beamPhi[b] = phi; s->beamSet[b] = true; s->beamGen++;
  });
}
dsr_status dsr_sph_set_beams_nbest(dsr_sph* s, dsr_sph* doa, const int32_t* nbest_idx, int n)
{
  return guard([&] {
    if (!s || !doa || !nbest_idx) throw Error(DSR_E_PARAMETER, "null argument");
    if (n < 1 || n > MAX_BEAMS) throw Error(DSR_E_DIMENSION, "%d beams (1..%d supported)", n, MAX_BEAMS);
    if (!doa->tbl) throw Error(DSR_E_ERROR, "no steering table: run the estimator after construction / setSearchParam first");
    for (int b = 0; b < n; b++)
      if (nbest_idx[b] < 0 || nbest_idx[b] >= units(*doa)) throw Error(DSR_E_INDEX, "rank %d: unit %d of %d (an empty rank has no direction)", b, nbest_idx[b], units(*doa));
    for (int b = 0; b < n; b++) {
      const double th = doa->uTheta[nbest_idx[b]], ph = doa->uPhi[nbest_idx[b]];
      if (b == 0) { s->lookTheta = th; s->lookPhi = ph; s->lookDirty = true; s->lookSet = true; s->settingsGen++; }
      else { s->beamTheta[b] = th; s->beamPhi[b] = ph; s->beamSet[b] = true; s->beamGen++; }
    }
  });
}
dsr_status dsr_sph_beam_weights(dsr_sph* s, int NB, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    ensure_beams(*s, NB);
    if (outDoubles < s->V.size() * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, s->V.size() * 2);
    for (size_t i = 0; i < s->V.size(); i++) { out[2 * i] = s->V[i].real(); out[2 * i + 1] = s->V[i].imag(); }
  });
}
dsr_status dsr_sph_sensor_weights(dsr_sph* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (!sensor_kind(s->kind)) throw Error(DSR_E_ERROR, "this kind's weights are modal (dsr_sph_look_weights; dsr_sph_beam_weights folds them)");
    ensure_look(*s);
    if (outDoubles < s->look.size() * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, s->look.size() * 2);
    for (size_t i = 0; i < s->look.size(); i++) { out[2 * i] = s->look[i].real(); out[2 * i + 1] = s->look[i].imag(); }
  });
}
int dsr_sph_beams_path(int NB)
{
  try { return beams_path(NB); } catch (const Error& e) { set_last_error(e.msg); return -1; }
}
dsr_status dsr_sph_beam_pattern_n(double minTheta, double maxTheta, double minPhi, double maxPhi, double widthTheta, double widthPhi, int* nTheta, int* nPhi)
{
  return guard([&] {
    if (!nTheta || !nPhi) throw Error(DSR_E_PARAMETER, "null argument");
    if (!(widthTheta > 0.0) || !(widthPhi > 0.0)) throw Error(DSR_E_PARAMETER, "widths %g, %g must be positive", widthTheta, widthPhi);
    *nTheta = pattern_n(minTheta, maxTheta, widthTheta); *nPhi = pattern_n(minPhi, maxPhi, widthPhi);
  });
}
dsr_status dsr_sph_beam_pattern(dsr_sph* s, unsigned fbinX, double theta, double phi, double minTheta, double maxTheta, double minPhi, double maxPhi,
                                double widthTheta, double widthPhi, double* out, size_t outDoubles)
{
  return guard([&] {                                        // getBeamPattern (:756-787; MOEN :2068-2099)
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (!(widthTheta > 0.0) || !(widthPhi > 0.0)) throw Error(DSR_E_PARAMETER, "widths %g, %g must be positive", widthTheta, widthPhi);
    if (fbinX > (unsigned) s->M / 2) throw Error(DSR_E_INDEX, "frequency bin %u (0..%d)", fbinX, s->M / 2);
    need_geometry(*s);
    const int nT = pattern_n(minTheta, maxTheta, widthTheta), nP = pattern_n(minPhi, maxPhi, widthPhi), C = s->C, D = s->dim;
    if (nT < 1 || nP < 1) throw Error(DSR_E_PARAMETER, "beam-pattern grid of %d x %d directions", nT, nP);
    if (outDoubles < (size_t) nT * nP) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %zu needed", outDoubles, (size_t) nT * nP);
    s->lookTheta = theta; s->lookPhi = phi; s->lookDirty = true; s->lookSet = true; s->settingsGen++;   // it calls setLookDirection (:768)
    ensure_look(*s);
    const bool sensor = sensor_kind(s->kind);
    const zc* w = &s->look[(size_t) fbinX * (sensor ? C : D)];   // wq_f(fbinX): the quiescent weights, whatever the active ones
    const double ka = 2.0 * M_PI * fbinX * s->a * s->sampleRate / (s->M * SSPEED);
    std::vector<zc> p(C);
    double th = minTheta;
    for (int it = 0; it < nT; it++, th += widthTheta) {
      double ph = minPhi;
      for (int ip = 0; ip < nP; ip++, ph += widthPhi) {
        for (int c = 0; c < C; c++)                          // planeWaveOnSphericalAperture (:737-747)
          p[c] = std::polar(1.0, ka * (std::sin(s->thS[c]) * std::sin(th) * std::cos(s->phS[c] - ph) + std::cos(s->thS[c]) * std::cos(th)));
        zc val(0, 0);
        if (s->kind == DSR_SPH_MOEN) for (int c = 0; c < C; c++) val += gmul(w[c], p[c]);                  // zdotu (:2091)
        else if (sensor) for (int c = 0; c < C; c++) val += gmul(std::conj(w[c]), p[c]);                   // SpatialDS: w^H p
        else
          for (int d = 0; d < D; d++) {                      // sphericalHarmonicsTransformation (zdotu), then zdotc
            zc Fd(0, 0);
            for (int c = 0; c < C; c++) Fd += gmul(p[c], s->SH[(size_t) d * C + c]);
            val += gmul(std::conj(w[d]), Fd);
          }
        out[(size_t) it * nP + ip] = std::hypot(val.real(), val.imag());
      }
    }
  });
}

dsr_status dsr_sph_beams(dsr_sph* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, int NB, float* Y_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !nframes_dev || !Y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "U %d, Tmax %d", U, Tmax);
    ensure_beams(*s, NB);
    const int F = s->M / 2 + 1, path = beams_path_for(NB, F);
    if ((long) Tmax * F > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "Tmax %d x %d bins", Tmax, F);
    require_device();
    if (U == 0 || Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    upload_beams(*s, NB, path, st);
    if (path == 1) {
      const int BC = beams_bin_chunk(s->C);
      if (BC == 8) launch_beams_mfma<8>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st);
      else if (BC == 4) launch_beams_mfma<4>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st);
      else if (BC == 2) launch_beams_mfma<2>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st);
      else launch_beams_mfma<1>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st);
    } else {
      switch (valu_rows(NB)) {
      case 1: launch_beams_valu<1, 4>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st); break;
      case 2: launch_beams_valu<2, 4>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st); break;
      case 3: launch_beams_valu<3, 4>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st); break;
      case 4: launch_beams_valu<4, 4>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st); break;
      case 8: launch_beams_valu<8, 2>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st); break;
      default: launch_beams_valu<16, 1>(*s, X_dev, nframes_dev, U, Tmax, NB, Y_dev, st); break;
      }
    }
  });
}

dsr_status dsr_sph_srp(dsr_sph* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* energy_dev, double* rp_dev,
                       double* nbest_rp_dev, int32_t* nbest_idx_dev, double* acc_dev, float* Y_dev, int32_t* gated_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !nframes_dev || !energy_dev || !nbest_rp_dev || !nbest_idx_dev || !acc_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "U %d, Tmax %d", U, Tmax);
    build_table(*s);
    check_range(s->fbinMin, s->fbinMax, s->M, s->tblFbinMax);
    const int path = pick_path(*s);
    require_device();
    if (U == 0 || Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    const int nU = units(*s);
    double* rp = rp_dev;
    if (!rp) { DevBuf<double>& w = s->ws.at(st); w.reserve((size_t) U * Tmax * nU); rp = w.p; }
    if (path == 1) {
      prepare_fold(*s);
      doa_launch_rp(s->fold, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
    } else {
      upload_s(*s, st); upload_fused_table(*s, st);
      if (s->DT == 1) launch_fused_tg<1>(*s, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
      else if (s->DT == 2) launch_fused_tg<2>(*s, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
      else launch_fused_tg<4>(*s, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
    }
    const long nfT = (long) U * Tmax;
    launch(k_sph_frame, dim3(cdiv(nfT, 4)), dim3(256), 0, st, rp, energy_dev, nframes_dev, U, Tmax, nU, s->nBest, s->threshold,
                       nbest_rp_dev, nbest_idx_dev, gated_dev);
    doa_launch_acc(rp, energy_dev, nframes_dev, U, Tmax, nU, s->threshold, acc_dev, st);
  });
}

dsr_status dsr_sph_final_nbest(dsr_sph* s, const double* acc, int U, double* nbest_rp, int32_t* nbest_idx)
{
  return guard([&] {
    if (!s || !acc || !nbest_rp || !nbest_idx) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->tbl) throw Error(DSR_E_ERROR, "no steering table: run the estimator after construction / setSearchParam first");
    final_nbest(acc, U, units(*s), s->nBest, nbest_rp, nbest_idx);      // _getNBestHypothesesFromACCRP (beamformer.cc:2986-3025)
  });
}

}  // extern "C"
