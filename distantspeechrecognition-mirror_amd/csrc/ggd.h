// csrc/ggd.h -- the constants of the generalised Gaussian model of a complex subband sample (btk/lib/GGDcEst.py: CGGaussianD.fixConst :45-61).
// Host code: lgamma is the C library's, log and exp are those of det_math.h.
#pragma once
#include "det_math.h"
#include <cmath>

namespace dsr {

struct GgdConst { double Bc, lNF, NgConst, LlConst, logBc; };

inline GgdConst ggd_constants(double p)
{
  GgdConst c;
  const double lg1 = std::lgamma(1.0 / p), lg2 = std::lgamma(2.0 / p), lB = lg1 - lg2;
  c.Bc = det_exp(lB);                                                // Gamma(1/p) / Gamma(2/p)
  c.lNF = (1.1447298858494002 + lg1) + lB;                           // log(pi) + log Gamma(1/p) + log B
  c.NgConst = (c.lNF - det_log(p)) + 1.0 / p;
  c.LlConst = det_log(p) - c.lNF;
  c.logBc = det_log(c.Bc);
  return c;
}

}  // namespace dsr
