// csrc/sph.cpp -- the host side of the spherical-array beamformers and SRP DOA estimators (dsr_sph_*; btk/beamformer/modalBeamformer.{h,cc}):
// set-up work, as in the reference.  The kernels, their operand layouts and launchers: csrc/k_sph.hip, reached through csrc/sph.h.
//
// The rigid-sphere mode amplitudes b_n(ka) (modeAmplitude :37-170, _calcModeAmplitudes), the conjugated spherical harmonics at the sensors
// sh_s [dim][C] (sphericalHarmonic :189-217, _calcSphericalHarmonicsAtEachPosition), the look-direction weights (EigenBeamformer::_calcWeights
// :304-345, SphericalDSBeamformer::_calcWeights :1022-1058, calcDCWeights), the (theta, phi) grid and steering table (_calcSteeringUnitTable
// :793-858, :1190-1246), the folded path's [units][C] table, the beam pattern and the final N-best from the accumulators.
// The spherical Bessel functions are computed here (series below x = l + 1, upward recurrence above; y_l upward): no GSL.
// The further kinds (SphericalHWNCBeamformer :1387-1478, SphericalGSCBeamformer :1483-1594, SphericalHWNCGSCBeamformer :1599-1713,
// SphericalMOENBeamformer :1804-2099, SphericalSpatialDSBeamformer :2106-2270) are weight designs below; all of them run on the beams kernels.
// Built with -ffp-contract=off, as the kernel file: the closed forms keep the reference's order of operations.
#include "sph.h"
#include "sph_math.h"
#include "gsc_weights.h"
#include "svd_linpack.h"
#include <algorithm>
#include <cmath>
#include <complex>

using namespace dsr;

typedef std::complex<double> zc;

// the GSL-shaped complex arithmetic (gmul, gdiv, gdivr, gmulr, gsinc), sph_plm and the EigenMike tables: csrc/sph_math.h

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

int pattern_n(double mn, double mx, double w)                // (int)(float)((max - min) / width + 0.5 + 1) (:759-766)
{
  const float n = (float) ((mx - mn) / w + 0.5 + 1);
  return n >= 1.0f && n < 1e6f ? (int) n : 0;
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
  try { return sph_srp_path(*s); } catch (const Error& e) { set_last_error(e.msg); return -1; }
}
dsr_status dsr_sph_srp_cell(dsr_sph* s, int cell[5], int64_t* ldsBytes)
{
  return guard([&] {
    if (!s || !cell) throw Error(DSR_E_PARAMETER, "null argument");
    build_table(*s);
    SphSrpCell c = sph_fused_cell(*s);
    if (sph_srp_path(*s) == 1) {                             // the folded table [units][C] through doa_launch_rp
      const SrpCell l = doa_srp_cell(units(*s), s->C);
      c = SphSrpCell{1, l.TG, 0, l.BC, l.KS, l.ldsBytes};
    }
    cell[0] = c.path; cell[1] = c.TG; cell[2] = c.DT; cell[3] = c.BC; cell[4] = c.KS;
    if (ldsBytes) *ldsBytes = (int64_t) c.ldsBytes;
  });
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
    if (s->dLookDirty) {                                     // the GSC kinds: (wq - wl); the sensor-domain kinds: zeros (Y_dev is then only a by-product of F_dev)
      std::vector<zc> eff;
      if (sensor_kind(s->kind)) eff.assign((size_t) (s->M / 2 + 1) * s->dim, zc(0, 0));
      else effective(*s, s->look, gsc_kind(s->kind) ? s->wl.data() : nullptr, eff);
      std::vector<double2> h(eff.size());
      for (size_t i = 0; i < h.size(); i++) h[i] = make_double2(eff[i].real(), eff[i].imag());
      s->dLook.upload(h, st); s->dLookDirty = false;
    }
    sph_apply(*s, X_dev, nframes_dev, U, Tmax, Y_dev, F_dev, st);
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
  try { return sph_beams_path(NB); } catch (const Error& e) { set_last_error(e.msg); return -1; }
}
dsr_status dsr_sph_beams_cell(int NB, int chanN, int bins, int cell[3], int64_t* ldsBytes)
{
  return guard([&] {
    if (!cell) throw Error(DSR_E_PARAMETER, "null argument");
    if (NB < 1 || NB > MAX_BEAMS) throw Error(DSR_E_DIMENSION, "%d beams (1..%d supported)", NB, MAX_BEAMS);
    if (chanN < 1 || chanN > 128) throw Error(DSR_E_DIMENSION, "%d channels (1..128 supported)", chanN);
    if (bins < 2) throw Error(DSR_E_DIMENSION, "%d bins", bins);
    const SphBeamsCell c = sph_beams_cell(NB, chanN, bins);
    cell[0] = c.kernel; cell[1] = c.kernel == 1 ? c.BCT : c.rows; cell[2] = c.kernel == 1 ? c.KS : c.CC;
    if (ldsBytes) *ldsBytes = (int64_t) c.ldsBytes;
  });
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
    const int F = s->M / 2 + 1, path = sph_beams_path_for(NB, F);
    if ((long) Tmax * F > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "Tmax %d x %d bins", Tmax, F);
    require_device();
    if (U == 0 || Tmax == 0) return;
    sph_beams(*s, X_dev, nframes_dev, U, Tmax, NB, path, Y_dev, (hipStream_t) stream);
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
    const int path = sph_srp_path(*s);
    require_device();
    if (U == 0 || Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    const int nU = units(*s);
    double* rp = rp_dev;
    if (!rp) { DevBuf<double>& w = s->ws.at(st); w.reserve((size_t) U * Tmax * nU); rp = w.p; }
    if (path == 1) {
      prepare_fold(*s);
      doa_launch_rp(s->fold, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
    } else sph_srp_fused(*s, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
    sph_frame(*s, rp, energy_dev, nframes_dev, U, Tmax, nbest_rp_dev, nbest_idx_dev, gated_dev, st);
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
