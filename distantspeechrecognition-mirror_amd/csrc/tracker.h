// csrc/tracker.h -- what the spherical-array speaker trackers' files share: the handle dsr_trk, the harmonics that the host set-up and the kernel both
// evaluate, and the functions through which the host side (tracker.cpp: the geometry, the modal coefficients, the observation-noise blocks, the
// dsr_trk_* / dsr_pws_* entries) reaches the kernels (k_tracker.hip).  Line numbers are tracker.cc's.
#pragma once
#include "sph_math.h"

struct dsr_trk {
  int spatial = 0, orderN = 0, modesN = 1, M = 0, F = 0, K = 0, L = 0, N = 0, maxLocalN = 1;
  double a = 0, fs = 0, s2u = 10, s2v = 10, s2init = 10, th0 = 0.5, ph0 = 0.0;
  std::vector<dsr::zcplx> bn, sc;                            // _bn [F][orderN+1]; _sphericalComponent [modesN][32] = conj(Y) at the sensors
  std::vector<double> norm, absbn;                           // [modesN]; |_bn| [F][orderN+1]
  std::vector<double> V; bool vDirty = true;                 // setV's blocks [F][2L][2L] (empty until the first setV: sqrt(sigma2_v) I)
  dsr::DevBuf<double2> dBn, dSc; dsr::DevBuf<double> dNorm, dAbs, dVt; bool tablesUp = false;
  dsr::PerStream<dsr::DevBuf<double>> ws;
  size_t lds = 0;
};

namespace dsr {

constexpr int CHAN = 32;                                     // _ChannelsN (:85)
constexpr int MAX_ORDER_N = 8;                               // 81 modes: the per-mode tables of the kernel
constexpr int STATE_DOUBLES = 8;                             // theta, phi, K (row major), frames seen, error flag

// _calculatePnm (:421-437): the unnormalised Legendre function with the negative-degree scaling loop; x = cos(theta)
DSR_HD inline double trk_pnm(int order, int degree, double x)
{
  double result = legendre_plm(order, degree < 0 ? -degree : degree, x);
  if (degree < 0) {
    int m = -degree; double factor = 1.0;
    while (m > degree) { factor *= (order + m); m--; }
    result /= factor;
    if (((-degree) % 2) == 1) result *= -1;
  }
  return result;
}
// _calculate_dPnm_dtheta (:440-449): dP/dx in fact; the (degree - order - 1) factor is kept for negative degree, as written
DSR_HD inline double trk_dpnm(int order, int degree, double x)
{
  const double x2 = x * x;
  return ((degree - order - 1) * trk_pnm(order + 1, degree, x) + (order + 1) * x * trk_pnm(order, degree, x)) / (1.0 - x2);
}
// harmonic (:319-339) and the two derivatives (:452-472) from cos / sin of theta and the mode's normalisation: host and device
struct Harm { double yr, yi, tr, ti, pr, pi, P, dP; };
DSR_HD inline Harm trk_harm(int n, int m, double ct, double st, double phi, double norm)
{
  Harm h;
  double p = sph_plm(n, m >= 0 ? m : -m, ct);
  if (m < 0 && ((-m) % 2) == 1) p = -p;
  const double ang = -m * phi, er = cos(ang), ei = sin(ang);
  h.yr = er * p; h.yi = ei * p;
  h.P = trk_pnm(n, m, ct); h.dP = trk_dpnm(n, m, ct);
  const double factor = -norm * h.dP * st;
  h.tr = er * factor; h.ti = ei * factor;
  const double qr = h.yr * 0.0 - h.yi * -1.0, qi = h.yr * -1.0 + h.yi * 0.0;    // gsl_complex_mul(Ynm, (0, -1))
  h.pr = qr * m; h.pi = qi * m;
  return h;
}

// ---- k_tracker.hip ----
// the largest 2N (rows of the realified observation) the workgroup's LDS admits, and the dynamic LDS of k_trk_run for s
long trk_max_rows(int modesN, int orderN, int spatial, int K);
size_t trk_lds_bytes(const dsr_trk& s);
// k_trk_init: state [U][STATE_DOUBLES] at (th, ph); the covariance factor k0 I unless keepK
void trk_launch_init(double* state, int U, double th, double ph, double k0, int keepK, hipStream_t st);
// k_trk_run over s's tables (uploaded when new, the V blocks when dirty): one workgroup per utterance, the frames in order
void trk_launch_run(dsr_trk& s, const float* X, const int32_t* nframes, int U, int Tmax, double* state, float* pos, double* pos64, int32_t* info, hipStream_t st);
// k_pws_apply: out = coefficient x source spectrum, optionally with the conjugate mirror
void pws_launch_apply(const double* coef, int C, const float* src, const int32_t* nframes, int U, int Tmax, int M, int full, float* out, hipStream_t st);

}  // namespace dsr
