// csrc/mllr_jacobi.h -- the phases of the cyclic two-sided Jacobi eigen-solver of k_mllr_solve, written per (thread, thread count) so that the
// kernel runs them between barriers and a host program can run the same code thread by thread.
//
// A symmetric n x n matrix a (row stride n) becomes diagonal under rotations applied in rounds of n/2 disjoint (p, q) pairs (the round-robin
// order of a tournament, so a sweep of m - 1 rounds meets every pair once); v accumulates the rotations: a_in = v diag(a) v^T.  Inside a round
// all rotations commute: J^T a is formed for every pair (each row belongs to one pair), then (J^T a) J and v J (each column belongs to one pair).
#pragma once
#include <cmath>
#ifdef __HIPCC__
#define MJ_FN __host__ __device__ inline
#else
#define MJ_FN inline
#endif

namespace dsr {

static constexpr int kJacobiSweeps = 30;                  // sweep cap; a symmetric matrix of order <= 129 needs about ten

// pair k of round r among m (even) players; p < q; a pair with q >= n (the phantom of an odd n) is idle
MJ_FN void mj_pair(int m, int r, int k, int& p, int& q)
{
  int a, b;
  if (k == 0) { a = m - 1; b = r; } else { a = (r + k) % (m - 1); b = (r - k + (m - 1)) % (m - 1); }
  p = a < b ? a : b; q = a < b ? b : a;
}

// the rotation that zeroes a_pq: cs[2 k] = c, cs[2 k + 1] = s (c = 1, s = 0: nothing to do)
MJ_FN void mj_angles(const double* a, int n, int m, int r, double* cs, int tid, int nt)
{
  for (int k = tid; k < m / 2; k += nt) {
    int p, q; mj_pair(m, r, k, p, q);
    double c = 1.0, s = 0.0;
    if (q < n) {
      const double apq = a[p * n + q];
      if (apq != 0.0) {
        const double tau = (a[q * n + q] - a[p * n + p]) / (2.0 * apq);
        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        c = 1.0 / sqrt(1.0 + t * t); s = t * c;
      }
    }
    cs[2 * k] = c; cs[2 * k + 1] = s;
  }
}

// rows: a <- J^T a
MJ_FN void mj_rows(double* a, int n, int m, int r, const double* cs, int tid, int nt)
{
  for (int e = tid; e < (m / 2) * n; e += nt) {
    const int k = e / n, j = e - k * n;
    int p, q; mj_pair(m, r, k, p, q);
    const double c = cs[2 * k], s = cs[2 * k + 1];
    if (q >= n || s == 0.0) continue;
    const double x = a[p * n + j], y = a[q * n + j];
    a[p * n + j] = c * x - s * y; a[q * n + j] = s * x + c * y;
  }
}

// columns: a <- a J, v <- v J; the rotated off-diagonal pair is set to zero exactly
MJ_FN void mj_cols(double* a, double* v, int n, int m, int r, const double* cs, int tid, int nt)
{
  for (int e = tid; e < (m / 2) * n; e += nt) {
    const int k = e / n, j = e - k * n;
    int p, q; mj_pair(m, r, k, p, q);
    const double c = cs[2 * k], s = cs[2 * k + 1];
    if (q >= n || s == 0.0) continue;
    double x = a[j * n + p], y = a[j * n + q];
    double xp = c * x - s * y, yq = s * x + c * y;
    if (j == p) yq = 0.0;
    if (j == q) xp = 0.0;
    a[j * n + p] = xp; a[j * n + q] = yq;
    x = v[j * n + p]; y = v[j * n + q];
    v[j * n + p] = c * x - s * y; v[j * n + q] = s * x + c * y;
  }
}

// partial sums of squares of row `tid`-strided rows: sq[2 t] off-diagonal, sq[2 t + 1] all (t < nt); summed by mj_norms_done in a fixed order
MJ_FN void mj_norms(const double* a, int n, double* sq, int tid, int nt)
{
  double off = 0.0, all = 0.0;
  for (int i = tid; i < n; i += nt)
    for (int j = 0; j < n; j++) { const double x = a[i * n + j]; all += x * x; if (j != i) off += x * x; }
  sq[2 * tid] = off; sq[2 * tid + 1] = all;
}
MJ_FN void mj_norms_done(const double* sq, int nt, double& off, double& all)
{
  off = 0.0; all = 0.0;
  for (int t = 0; t < nt; t++) { off += sq[2 * t]; all += sq[2 * t + 1]; }
}
// converged: the off-diagonal Frobenius norm is below n 2^-53 times the whole norm (what the roundings of one sweep leave behind)
MJ_FN bool mj_converged(double off, double all, int n) { const double tol = n * 0x1p-53; return off <= tol * tol * all; }

}  // namespace dsr
