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
// The MFMA's lane map: csrc/mfma64.h; the frame tiling (FB, bin_chunk) and the shared kernel parts: csrc/srp_common.h.
#include "srp_common.h"
#include <algorithm>
#include <cmath>
#include <complex>

using namespace dsr;

typedef std::complex<double> zc;

namespace {

constexpr double SSPEED = 343740.0;                          // mm/s (beamformer.h:47)
constexpr int MAX_ORDER = 8;                                 // dim = maxOrder^2 <= 64: four 16-row tiles of the fused kernel
constexpr long MAX_TABLE = 1L << 27;                         // (fbinMax+1) units max(dim, C) complex128 entries: 2 GiB per table copy

// the EigenMike's 32 capsules in degrees (setEigenMikeGeometry :414-535), radius 42 mm
const int EM_THETA[32] = {69, 90, 111, 90, 32, 55, 90, 125, 148, 125, 90, 55, 21, 58, 121, 159, 69, 90, 111, 90, 32, 55, 90, 125, 148, 125, 90, 55, 21, 58, 122, 159};
const int EM_PHI[32] = {0, 32, 0, 328, 0, 45, 69, 45, 0, 315, 291, 315, 91, 90, 90, 89, 180, 212, 180, 148, 180, 225, 249, 225, 180, 135, 111, 135, 269, 270, 270, 271};

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
};

namespace {

// ---- GSL-shaped complex arithmetic (gsl_complex_math.c), so that the closed forms keep the reference's order of operations ----
inline zc gmul(zc a, zc b) { return zc(a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()); }
inline zc gdiv(zc a, zc b)
{
  const double s = 1.0 / std::hypot(b.real(), b.imag()), sbr = s * b.real(), sbi = s * b.imag();
  return zc((a.real() * sbr + a.imag() * sbi) * s, (a.imag() * sbr - a.real() * sbi) * s);
}
inline zc gdivr(zc a, double x) { return zc(a.real() / x, a.imag() / x); }
inline zc gmulr(zc a, double x) { return zc(a.real() * x, a.imag() * x); }
inline double gsinc(double x)                                // gsl_sf_sinc(x) = sin(pi x) / (pi x)
{
  const double y = M_PI * x;
  return std::fabs(x) < 1e-8 ? 1.0 - y * y / 6.0 : std::sin(y) / y;
}

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

// gsl_sf_legendre_sphPlm(l, m, x), m >= 0: sqrt((2l+1)/(4 pi)) sqrt((l-m)!/(l+m)!) P_l^m(x) with the Condon-Shortley phase, by the normalised recurrence
double sph_plm(int l, int m, double x)
{
  double pmm = 1.0 / std::sqrt(4.0 * M_PI);
  const double u = std::sqrt((1.0 - x) * (1.0 + x));
  for (int i = 1; i <= m; i++) pmm *= -u * std::sqrt((2.0 * i + 1.0) / (2.0 * i));
  if (l == m) return pmm;
  double p1 = x * std::sqrt(2.0 * m + 3.0) * pmm;
  if (l == m + 1) return p1;
  double p0 = pmm;
  for (int n = m + 2; n <= l; n++) {
    const double a = std::sqrt((4.0 * n * n - 1.0) / ((double) n * n - (double) m * m));
    const double b = std::sqrt(((n - 1.0) * (n - 1.0) - (double) m * m) / (4.0 * (n - 1.0) * (n - 1.0) - 1.0));
    const double p = a * (x * p1 - b * p0);
    p0 = p1; p1 = p;
  }
  return p1;
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

// _calcWeights of bin f for the direction (theta, phi) into w[dim], with the unit's harmonics Y [dim] at that direction precomputed
void calc_weights(const dsr_sph& s, int f, const zc* Y, zc* w)
{
  static const zc IN[4] = {zc(1, 0), zc(0, 1), zc(-1, 0), zc(0, -1)};
  const unsigned norm = (unsigned) s.dim * (unsigned) s.C;
  for (int n = 0, idx = 0; n < s.maxOrder; n++) {
    const zc bn = s.B[(size_t) f * s.maxOrder + n], in = IN[n % 4];
    if (s.kind == DSR_SPH_EB) {                             // :304-345, the HMDI beamformer
      const double bn2 = std::norm(bn) + (double) s.sigma2, de = norm * bn2;
      const zc inbn = gmul(in, bn);
      for (int m = -n; m <= n; m++, idx++) w[idx] = gdivr(gmul(gmulr(std::conj(Y[idx]), 4 * M_PI), inbn), de);
    } else {                                                 // :1022-1058
      for (int m = -n; m <= n; m++, idx++) w[idx] = std::conj(gmulr(gmul(Y[idx], std::conj(gmul(in, bn))), 4 * M_PI));
    }
  }
  if (s.normalize) {                                         // normalizeWeights (:23-29): wgain / ||w||_2
    double ss = 0.0;
    for (int i = 0; i < s.dim; i++) ss += std::norm(w[i]);
    const double nrm = s.wgain / std::sqrt(ss);
    for (int i = 0; i < s.dim; i++) w[i] = gmulr(w[i], nrm);
  }
}

void harmonics_at(const dsr_sph& s, double theta, double phi, zc* Y)
{
  for (int n = 0, idx = 0; n < s.maxOrder; n++)
    for (int m = -n; m <= n; m++, idx++) Y[idx] = sph_harmonic(m, n, theta, phi);
}

void ensure_look(dsr_sph& s)                                 // _calcSteeringUnit(0): DC weights at bin 0, _calcWeights at 1..M/2
{
  ensure_modes(s);
  if (!s.lookDirty) return;
  const int F = s.M / 2 + 1, D = s.dim;
  s.look.assign((size_t) F * D, zc(0, 0));
  s.look[0] = zc(1, 0);                                      // calcDCWeights: 1 for n = 0
  std::vector<zc> Y(D); harmonics_at(s, s.lookTheta, s.lookPhi, Y.data());
  for (int f = 1; f < F; f++) calc_weights(s, f, Y.data(), &s.look[(size_t) f * D]);
  s.lookDirty = false; s.dLookDirty = true;
}

int grid_n(double mn, double mx, double w)                   // (unsigned)((max - min) / width + 0.5) (:803-804)
{
  const double v = (mx - mn) / w + 0.5;
  return v >= 1.0 && v < 1e9 ? (int) (unsigned) v : 0;
}

void build_table(dsr_sph& s)                                 // _calcSteeringUnitTable (:793-858 / :1190-1246)
{
  if (s.tbl) return;
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
  hipLaunchKernelGGL((k_sph_srp<TG, DT>), grid, dim3(256), lds, st, (const float2*) X, nf, s.dSp.p, s.dWp.p, s.C, Tmax, F, s.M / 2, s.fbinMin, s.fbinMax,
                     units(s), s.NT, s.KS, BC, rp, en, (float2*) Y);
  DSR_HIP(hipGetLastError());
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
  s.B.clear(); s.lookDirty = true; s.dSDirty = true; s.foldGen = ~0u; s.settingsGen++;   // a new radius: new mode amplitudes (the table is not rebuilt)
}

}  // namespace

extern "C" {

dsr_status dsr_sph_create(int kind, int nBest, int sampleRate, int fftLen, int halfBandShift, int NC, int maxOrder, int normalizeWeight, int chanN, dsr_sph** out)
{
  (void) NC;                                                 // only passed on by the reference (beamformerWeights' NC), never used here
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind != DSR_SPH_EB && kind != DSR_SPH_DS) throw Error(DSR_E_PARAMETER, "kind %d (DSR_SPH_EB or DSR_SPH_DS)", kind);
    if (halfBandShift) throw Error(DSR_E_PARAMETER, "_halfBandShift == true is not implemented yet");    // modalBeamformer.cc:391-394
    if (nBest < 1) throw Error(DSR_E_PARAMETER, "nBest %d < 1", nBest);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_PARAMETER, "fftLen %d", fftLen);
    if (sampleRate <= 0) throw Error(DSR_E_PARAMETER, "sampleRate %d", sampleRate);
    if (chanN < 1 || chanN > 128) throw Error(DSR_E_DIMENSION, "%d channels (1..128 supported)", chanN);
    if (maxOrder < 1 || maxOrder > MAX_ORDER) throw Error(DSR_E_DIMENSION, "maxOrder %d: 1..%d supported (dim = maxOrder^2 <= %d)", maxOrder, MAX_ORDER, MAX_ORDER * MAX_ORDER);
    dsr_sph* s = new dsr_sph(); s->kind = kind; s->nBest = nBest; s->sampleRate = (unsigned) sampleRate; s->M = fftLen; s->C = chanN;
    s->maxOrder = maxOrder; s->dim = maxOrder * maxOrder; s->normalize = normalizeWeight != 0; s->fbinMax = fftLen / 2;
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
    s->lookTheta = theta; s->lookPhi = phi; s->lookDirty = true; s->settingsGen++;   // (the reference warns when theta is outside [0, pi] and goes on)
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
    ensure_look(*s);
    require_device();
    if (U == 0 || Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    upload_s(*s, st);
    if (s->dLookDirty) {
      std::vector<double2> h(s->look.size());
      for (size_t i = 0; i < h.size(); i++) h[i] = make_double2(s->look[i].real(), s->look[i].imag());
      s->dLook.upload(h, st); s->dLookDirty = false;
    }
    const int F = s->M / 2 + 1;
    if ((long) Tmax * F > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "Tmax %d x %d bins", Tmax, F);
    hipLaunchKernelGGL(k_sph_apply, dim3(cdiv((long) Tmax * F, 256), U), dim3(256), 0, st, (const float2*) X_dev, nframes_dev, s->dS.p, s->dLook.p,
                       s->C, Tmax, F, s->dim, (float2*) Y_dev, (float2*) F_dev);
    DSR_HIP(hipGetLastError());
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
    hipLaunchKernelGGL(k_sph_frame, dim3(cdiv(nfT, 4)), dim3(256), 0, st, rp, energy_dev, nframes_dev, U, Tmax, nU, s->nBest, s->threshold,
                       nbest_rp_dev, nbest_idx_dev, gated_dev);
    DSR_HIP(hipGetLastError());
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
