// csrc/det_math.h -- fp64 log, exp and pow that give the same bits on the device, on the host and in numpy (tests/mn_np.py restates them
// operation for operation).  A minimiser branches on comparisons of nearly equal costs, so the transcendental functions under those costs are
// part of the interface: they are written from additions, multiplications, one division, floor and exponent-field moves only, and every unit
// that includes this header is built with -ffp-contract=off.  Coefficients are the exact series values rounded to double (1/(2j+1), 1/j!).
//
//   det_log(x)   x = 2^e m, m in [sqrt(1/2), sqrt(2));  s = (m - 1)/(m + 1), z = s s, p = sum_{j=1..11} z^(j-1) / (2j+1) (Horner),
//                r = 2s + (2s)(z p);  (e LN2_HI + r) + e LN2_LO.  LN2_HI holds the leading 33 bits of ln 2, so e LN2_HI is exact.
//                x = 0: -inf, x = +inf: +inf, x < 0 or NaN: NaN.  Measured: at most 2.6 2^-53 relative.
//   det_exp(x)   k = floor(x / ln 2 + 0.5), r = (x - k LN2_HI) - k LN2_LO, p = sum_{j=2..14} r^(j-2) / j! (Horner), y = 1 + (r + (r r) p), y 2^k.
//                x < -708: 0, x > 709: +inf, NaN: NaN.
//   det_pow(x,f) det_exp(f det_log(x)) for x > 0, 0 for x == 0, NaN otherwise.  Measured: at most 2.3 (|f ln x| + 2) 2^-53 relative.
//   det_psi(x)   digamma, host only (the GG model update): psi(x) = psi(x + 1) - 1/x up to x >= 6, then the asymptotic series to x^-22.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define DET_HD __host__ __device__
#else
#define DET_HD
#endif

namespace dsr {

constexpr double DET_LN2_HI = 0x1.62e42fefp-1;             // the leading 33 bits of ln 2
constexpr double DET_LN2_LO = 0x1.473de6af278edp-34;       // ln 2 - DET_LN2_HI
constexpr double DET_INV_LN2 = 0x1.71547652b82fep+0;
constexpr double DET_SQRT_HALF = 0.70710678118654757;

DET_HD inline uint64_t det_bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
DET_HD inline double det_from_bits(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

DET_HD inline double det_log(double x)
{
  if (!(x > 0.0)) return x == 0.0 ? -__builtin_inf() : __builtin_nan("");
  if (x > 1.7976931348623157e308) return x;
  int e = 0;
  if (x < 2.2250738585072014e-308) { x *= 18014398509481984.0; e = -54; }        // subnormal: times 2^54, exact
  const uint64_t u = det_bits(x);
  e += (int) ((u >> 52) & 0x7ff) - 1022;                                          // x = 2^e m, m in [1/2, 1)
  double m = det_from_bits((u & 0x800fffffffffffffull) | 0x3fe0000000000000ull);
  if (m < DET_SQRT_HALF) { m *= 2.0; e -= 1; }
  const double s = (m - 1.0) / (m + 1.0), z = s * s;
  double p = 1.0 / 23.0;
  p = 1.0 / 21.0 + z * p; p = 1.0 / 19.0 + z * p; p = 1.0 / 17.0 + z * p; p = 1.0 / 15.0 + z * p; p = 1.0 / 13.0 + z * p;
  p = 1.0 / 11.0 + z * p; p = 1.0 / 9.0 + z * p; p = 1.0 / 7.0 + z * p; p = 1.0 / 5.0 + z * p; p = 1.0 / 3.0 + z * p;
  const double s2 = 2.0 * s, r = s2 + s2 * (z * p), de = (double) e;
  return (de * DET_LN2_HI + r) + de * DET_LN2_LO;
}

DET_HD inline double det_exp(double x)
{
  if (x != x) return x;
  if (x < -708.0) return 0.0;
  if (x > 709.0) return __builtin_inf();
  const double k = floor(x * DET_INV_LN2 + 0.5);
  const double r = (x - k * DET_LN2_HI) - k * DET_LN2_LO;
  double p = 1.0 / 87178291200.0;
  p = 1.0 / 6227020800.0 + r * p; p = 1.0 / 479001600.0 + r * p; p = 1.0 / 39916800.0 + r * p; p = 1.0 / 3628800.0 + r * p;
  p = 1.0 / 362880.0 + r * p; p = 1.0 / 40320.0 + r * p; p = 1.0 / 5040.0 + r * p; p = 1.0 / 720.0 + r * p; p = 1.0 / 120.0 + r * p;
  p = 1.0 / 24.0 + r * p; p = 1.0 / 6.0 + r * p; p = 1.0 / 2.0 + r * p;
  const double y = 1.0 + (r + (r * r) * p);
  return y * det_from_bits((uint64_t) ((int64_t) k + 1023) << 52);                // |k| <= 1023 here: 2^k is a normal number
}

DET_HD inline double det_pow(double x, double f)
{
  if (x > 0.0) return det_exp(f * det_log(x));
  return x == 0.0 ? 0.0 : __builtin_nan("");
}

inline double det_psi(double x)
{
  double r = 0.0;
  while (x < 6.0) { r -= 1.0 / x; x += 1.0; }
  const double v = 1.0 / x, w = v * v;
  double t = 854513.0 / 3036.0;                                                   // |B_2k| / (2k), k = 11 .. 1
  t = 174611.0 / 6600.0 - w * t; t = 43867.0 / 14364.0 - w * t; t = 3617.0 / 8160.0 - w * t;
  t = 1.0 / 12.0 - w * t; t = 691.0 / 32760.0 - w * t; t = 1.0 / 132.0 - w * t; t = 1.0 / 240.0 - w * t;
  t = 1.0 / 252.0 - w * t; t = 1.0 / 120.0 - w * t; t = 1.0 / 12.0 - w * t;
  return r + ((det_log(x) - 0.5 * v) - w * t);
}

}  // namespace dsr
