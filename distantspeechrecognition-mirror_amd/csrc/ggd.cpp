// csrc/ggd.cpp -- the host part of the generalised Gaussian model of complex subband samples (btk/lib/GGDcEst.py): the constants of a shape
// parameter (fixConst :45-61), the maximum-likelihood update from accumulated statistics (MLE4CGGaussianD.update :246-293), the parameter and
// accumulator files (:118-152, :176-216), and the host hooks of det_math.h.  Nothing here needs a device.  Built with -ffp-contract=off:
// tests/mn_np.py restates update() operation for operation.
#include "common.h"
#include "ggd.h"
#include <cstdio>

using namespace dsr;

namespace {

struct File {
  FILE* fp;
  File(const char* path, const char* mode) : fp(path ? fopen(path, mode) : nullptr)
  { if (!fp) throw Error(DSR_E_IO, "Could not %s file %s", mode[0] == 'r' ? "find" : "write", path ? path : "(null)"); }
  ~File() { if (fp) fclose(fp); }
};

void read_doubles(File& f, const char* path, double* v, int n)
{
  for (int i = 0; i < n; i++)
    if (fscanf(f.fp, "%lf", &v[i]) != 1) throw Error(DSR_E_IO, "%s: value %d of %d is missing", path, i + 1, n);
}

}  // namespace

extern "C" {

dsr_status dsr_det_log(const double* x, double* y, int n)
{ return guard([&] { if (!x || !y) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < n; i++) y[i] = det_log(x[i]); }); }
dsr_status dsr_det_exp(const double* x, double* y, int n)
{ return guard([&] { if (!x || !y) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < n; i++) y[i] = det_exp(x[i]); }); }
dsr_status dsr_det_psi(const double* x, double* y, int n)
{
  return guard([&] {
    if (!x || !y) throw Error(DSR_E_PARAMETER, "null argument");
    for (int i = 0; i < n; i++) {
      if (!(x[i] > 0.0) || !std::isfinite(x[i])) throw Error(DSR_E_PARAMETER, "det_psi of %g", x[i]);
      y[i] = det_psi(x[i]);
    }
  });
}

dsr_status dsr_ggd_constants(const double* p, int F, double* Bc, double* lNF, double* NgConst, double* LlConst)
{
  return guard([&] {
    if (!p) throw Error(DSR_E_PARAMETER, "null argument");
    for (int f = 0; f < F; f++) {
      if (!(p[f] > 0.0) || !std::isfinite(p[f])) throw Error(DSR_E_PARAMETER, "the shape parameter of bin %d is %g", f, p[f]);
      const GgdConst c = ggd_constants(p[f]);
      if (Bc) Bc[f] = c.Bc;
      if (lNF) lNF[f] = c.lNF;
      if (NgConst) NgConst[f] = c.NgConst;
      if (LlConst) LlConst[f] = c.LlConst;
    }
  });
}

dsr_status dsr_ggd_update(const double* acc, int F, const double* p, const double* sa, int nItr, double alpha, double thresh, double floorV, double floorP,
                          int sigmaOnly, double* newSa, double* newP, int32_t* converged)
{
  return guard([&] {
    if (!acc || !p || !sa || !newSa || !newP || !converged) throw Error(DSR_E_PARAMETER, "null argument");
    if (nItr < 0) throw Error(DSR_E_PARAMETER, "nItr %d", nItr);
    for (int f = 0; f < F; f++) {
      const double acc1S = acc[f], acc1P = acc[F + f], acc2P = acc[2 * F + f], nS = acc[3 * F + f], pf = p[f];
      newSa[f] = sa[f]; newP[f] = pf; converged[f] = 0;
      if (!(pf > 0.0) || !std::isfinite(pf)) throw Error(DSR_E_PARAMETER, "the shape parameter of bin %d is %g", f, pf);
      if (!(nS > 0.0)) continue;                                     // no sample: the bin keeps its parameters
      const double B = ggd_constants(pf).Bc;
      const double val = det_pow((pf * acc1S) / nS, 1.0 / pf);       // :255-256
      const double sigma = (1.0 / B) * val;
      double np_ = pf;
      if (!sigmaOnly) {                                              // :259-265
        const double dg1 = det_psi(1.0 / pf), dg2 = det_psi(2.0 / pf);
        const double dLp1 = (nS / (pf * pf)) * ((pf + 2.0 * dg1) - 2.0 * dg2);
        const double dLp2 = acc1P + (acc2P * (dg1 - 2.0 * dg2)) / pf;
        const double dLp = dLp1 - dLp2;
        np_ = pf + dLp * (alpha / (double) (1 + nItr));
        if (fabs(np_ - pf) < thresh) converged[f] = 1;
      }
      newSa[f] = sigma < floorV ? floorV : sigma;                    // :275-285 (a sigma that is not a number stays one)
      if (!sigmaOnly) newP[f] = np_ < floorP ? floorP : np_;
    }
  });
}

dsr_status dsr_ggd_write_param(const char* path, double sa, double p, double mean)
{
  return guard([&] {
    if (mean != 0.0) throw Error(DSR_E_PARAMETER, "zero-mean models only (mean = %g)", mean);
    if (!(p > 0.0) || !std::isfinite(p)) throw Error(DSR_E_PARAMETER, "the shape parameter is %g", p);
    const GgdConst c = ggd_constants(p);
    File f(path, "w");
    fprintf(f.fp, "%e %e %e\n", sa, p, mean);
    fprintf(f.fp, "%e %e\n", c.Bc, c.lNF);
  });
}

dsr_status dsr_ggd_read_param(const char* path, double out[5])
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    File f(path, "r");
    read_doubles(f, path, out, 5);                                   // sa p mean / B lNF
  });
}

dsr_status dsr_ggd_write_accs(const char* path, const double acc[5], double alpha, int nItr, double thresh, double floorV, double floorP)
{
  return guard([&] {
    if (!acc) throw Error(DSR_E_PARAMETER, "null argument");
    File f(path, "w");
    fprintf(f.fp, "%e\n%e\n%e\n%lld\n%e\n", acc[0], acc[1], acc[2], (long long) acc[3], acc[4]);
    fprintf(f.fp, "%e\n%d\n%e\n%e\n%e\n", alpha, nItr, thresh, floorV, floorP);
  });
}

dsr_status dsr_ggd_read_accs(const char* path, double acc[5], int* used)
{
  return guard([&] {
    if (!acc || !used) throw Error(DSR_E_PARAMETER, "null argument");
    File f(path, "r");
    double v[10];
    read_doubles(f, path, v, 10);
    *used = (int) v[6] == 1 ? 1 : 0;                                 // statistics of another iteration are ignored (:206-209)
    if (*used) for (int i = 0; i < 5; i++) acc[i] += v[i];
  });
}

}  // extern "C"
