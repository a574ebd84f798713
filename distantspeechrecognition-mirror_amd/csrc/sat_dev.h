// csrc/sat_dev.h -- the device code sat_kernels.hip and fsat_kernels.hip share: transform(origMean) in the transform's own types, the
// variance statistic of one speaker, the auxiliary function and the Jacobi loop of the mean solve.  Every operation is an explicit
// round-to-nearest intrinsic in the reference's order, so that both units restate asr/sat/sat.cc ("sat") and asr/adapt/transform.cc ("tr")
// with the same bits.
#pragma once
#include "sat.h"
#include "mllr_jacobi.h"

namespace dsr {

// component of transform(origMean) whose matrix row is a [bl] and whose block of the mean is mu [bl]; bias: the offset the transform adds
// to this component, or none.  MLLR (tr:1777-1784): float comp = offset, rounded to float after every term.  APT (tr:1300-1336): the double
// sum stored to float, then the float bias
__device__ inline float sat_transform_comp(int kind, bool hasBias, double bias, const double* a, const float* mu, int bl)
{
  float comp;
  if (kind == kSatMLLR) {
    comp = hasBias ? (float) bias : 0.0f;
    for (int j = 0; j < bl; j++) comp = (float) __dadd_rn((double) comp, __dmul_rn(a[j], (double) mu[j]));
  } else {
    double sum = 0.0;
    for (int j = 0; j < bl; j++) sum = __dadd_rn(sum, __dmul_rn(a[j], (double) mu[j]));
    comp = (float) sum;
    if (hasBias) comp = __fadd_rn(comp, (float) bias);
  }
  return comp;
}

// vec + sumOsq - 2 trn sumO + c trn^2 as sat:723-724 and codebookFastSAT.cc:410-414 write it
__device__ inline double sat_var_term(double vec, double sumOsq, double sumO, double trn, double c)
{
  const double sqr = __dmul_rn(trn, trn);
  return __dadd_rn(__dsub_rn(__dadd_rn(vec, sumOsq), __dmul_rn(__dmul_rn(2.0, trn), sumO)), __dmul_rn(c, sqr));
}

// t = M x, a row a thread; M has row stride n
__device__ inline void sat_rows_times(const double* M, const double* x, double* t, int n, int tid, int nt)
{
  for (int e = tid; e < n; e += nt) { double s = 0.0; for (int j = 0; j < n; j++) s = __dadd_rn(s, __dmul_rn(M[e * n + j], x[j])); t[e] = s; }
}

// _auxFunc (sat:276-286) given t = M x: 0.5 (x^T t + scalar) - x^T vec; one thread
__device__ inline double sat_aux_value(const double* t, const double* x, const double* vec, double scalar, int n)
{
  double ip1 = 0.0, ip2 = 0.0;
  for (int e = 0; e < n; e++) { ip1 = __dadd_rn(ip1, __dmul_rn(t[e], x[e])); ip2 = __dadd_rn(ip2, __dmul_rn(x[e], vec[e])); }
  return __dsub_rn(__dmul_rn(0.5, __dadd_rn(ip1, scalar)), ip2);
}

// the cyclic Jacobi of mllr_jacobi.h by the whole workgroup: a -> diag, v (the identity on entry) accumulates the rotations; cs [m], sq [2 nt].
// false: not converged within the sweep cap, or a norm that is NaN or infinite.  The same value in every thread
__device__ inline bool sat_jacobi(double* a, double* v, int n, int m, double* cs, double* sq, int tid, int nt)
{
  for (int sweep = 0; sweep <= kJacobiSweeps; sweep++) {
    mj_norms(a, n, sq, tid, nt);
    __syncthreads();
    double off, all; mj_norms_done(sq, nt, off, all);
    __syncthreads();
    if (!(all <= 1.7E308)) return false;                  // NaN or infinite
    if (mj_converged(off, all, n)) return true;
    if (sweep == kJacobiSweeps) return false;
    for (int r = 0; r < m - 1; r++) {
      mj_angles(a, n, m, r, cs, tid, nt);
      __syncthreads();
      mj_rows(a, n, m, r, cs, tid, nt);
      __syncthreads();
      mj_cols(a, v, n, m, r, cs, tid, nt);
      __syncthreads();
    }
  }
  return false;
}

}  // namespace dsr
