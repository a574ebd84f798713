// csrc/sph_math.h -- what the spherical-array files share (sph.cpp, k_tracker.hip): the EigenMike's capsule table, the GSL-shaped complex
// arithmetic that keeps the reference's order of operations, the normalised Legendre recurrence (host and device) and the spherical Bessel
// functions of sph.cpp.
#pragma once
#include "common.h"
#include <cmath>
#include <complex>

#ifdef __HIPCC__
#define DSR_HD __host__ __device__
#else
#define DSR_HD
#endif

namespace dsr {

typedef std::complex<double> zcplx;

// the EigenMike's 32 capsules in degrees (modalBeamformer.cc setEigenMikeGeometry :414-535, tracker.cc :195-297: the same table), radius 42 mm
constexpr int EM_THETA[32] = {69, 90, 111, 90, 32, 55, 90, 125, 148, 125, 90, 55, 21, 58, 121, 159, 69, 90, 111, 90, 32, 55, 90, 125, 148, 125, 90, 55, 21, 58, 122, 159};
constexpr int EM_PHI[32] = {0, 32, 0, 328, 0, 45, 69, 45, 0, 315, 291, 315, 91, 90, 90, 89, 180, 212, 180, 148, 180, 225, 249, 225, 180, 135, 111, 135, 269, 270, 270, 271};

// ---- GSL-shaped complex arithmetic (gsl_complex_math.c), so that the closed forms keep the reference's order of operations ----
inline zcplx gmul(zcplx a, zcplx b) { return zcplx(a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()); }
inline zcplx gdiv(zcplx a, zcplx b)
{
  const double s = 1.0 / std::hypot(b.real(), b.imag()), sbr = s * b.real(), sbi = s * b.imag();
  return zcplx((a.real() * sbr + a.imag() * sbi) * s, (a.imag() * sbr - a.real() * sbi) * s);
}
inline zcplx gdivr(zcplx a, double x) { return zcplx(a.real() / x, a.imag() / x); }
inline zcplx gmulr(zcplx a, double x) { return zcplx(a.real() * x, a.imag() * x); }
inline double gsinc(double x)                                // gsl_sf_sinc(x) = sin(pi x) / (pi x)
{
  const double y = M_PI * x;
  return std::fabs(x) < 1e-8 ? 1.0 - y * y / 6.0 : std::sin(y) / y;
}

// gsl_sf_legendre_sphPlm(l, m, x), m >= 0: sqrt((2l+1)/(4 pi)) sqrt((l-m)!/(l+m)!) P_l^m(x) with the Condon-Shortley phase, by the normalised recurrence
DSR_HD inline double sph_plm(int l, int m, double x)
{
  double pmm = 1.0 / sqrt(4.0 * M_PI);
  const double u = sqrt((1.0 - x) * (1.0 + x));
  for (int i = 1; i <= m; i++) pmm *= -u * sqrt((2.0 * i + 1.0) / (2.0 * i));
  if (l == m) return pmm;
  double p1 = x * sqrt(2.0 * m + 3.0) * pmm;
  if (l == m + 1) return p1;
  double p0 = pmm;
  for (int n = m + 2; n <= l; n++) {
    const double a = sqrt((4.0 * n * n - 1.0) / ((double) n * n - (double) m * m));
    const double b = sqrt(((n - 1.0) * (n - 1.0) - (double) m * m) / (4.0 * (n - 1.0) * (n - 1.0) - 1.0));
    const double p = a * (x * p1 - b * p0);
    p0 = p1; p1 = p;
  }
  return p1;
}

// gsl_sf_legendre_Plm(l, m, x), m >= 0: the unnormalised P_l^m with the Condon-Shortley phase, upward in l from P_m^m
DSR_HD inline double legendre_plm(int l, int m, double x)
{
  double pmm = 1.0;
  if (m > 0) {
    const double root = sqrt(1.0 - x) * sqrt(1.0 + x);
    double fact = 1.0;
    for (int i = 0; i < m; i++) { pmm *= -fact * root; fact += 2.0; }
  }
  if (l == m) return pmm;
  double pmmp1 = x * (2 * m + 1) * pmm;
  if (l == m + 1) return pmmp1;
  double p = 0.0;
  for (int ell = m + 2; ell <= l; ell++) {
    p = (x * (2 * ell - 1) * pmmp1 - (ell + m - 1) * pmm) / (ell - m);
    pmm = pmmp1; pmmp1 = p;
  }
  return p;
}

double sph_jl(int l, double x);                              // sph.cpp
double sph_yl(int l, double x);

}  // namespace dsr
