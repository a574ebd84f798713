// csrc/stc_rows.h -- the estimation of a semi-tied covariance transform (STCEstimator::_update, Accu::makePosDef, asr/train/estimateAdapt.cc:
// 2387-2464, 2689-2711, "eA") and of an LDA matrix (LDAEstimator::_update, eA:2793-2836), written per (thread, thread count) with the barrier
// passed in, as fsa_rows.h is: k_stc_eig / k_stc_rows / k_lda_solve run it between __syncthreads() and a host program runs the same code with
// one thread and an empty barrier.  Every branch around a barrier depends on values all threads read alike.
//
//   stc_jacobi     a symmetric matrix to its eigenvalues (the diagonal left in a) and eigenvectors v by the phases of mllr_jacobi.h.
//   stc_eig_run    G_d = sumOsq[d] + E regSq[d] -> its smallest and largest eigenvalue and, where stc_posdef, G_d^-1 = V diag(1 / lambda) V^T
//                  (symmetric bit for bit).  The reference asks gsl_eigen_symm for lambda <= 0 (eA:2702-2704) and inverts by LU (eA:2407-2409).
//                  stc_posdef also refuses a smallest eigenvalue below 16 n 2^-53 of the largest: the decomposition knows an eigenvalue only
//                  to about n 2^-53 lambda_max, so such a value is not known to be positive (statistics of fewer items than dimN land there).
//   stc_invert     A -> A^-1 in place by Gauss-Jordan elimination with row pivoting, and the SIGN of det A.  Only the sign survives in a row
//                  update: with c = det A . A^-1[:, d], row_d = sqrt(gamma / (c^T Gi c)) Gi^T c is unchanged when c is scaled by a positive
//                  number.  The magnitude of det A, which leaves the range of a double at dimN = 40, is never formed.
//   stc_rows_run   itns sweeps over the rows d (eA:2416-2448).  A^-1 and the sign follow a changed row by the rank-one update
//                  A'^-1 = A^-1 - (A^-1 e_d)(delta^T A^-1) / (1 + delta^T A^-1 e_d) and are formed afresh at the start of every sweep (the
//                  reference decomposes A afresh for every row).  c^T Gi c <= 0 is the reference's jnumeric_error (eA:2434-2435); before every
//                  row and for the result ||A||_F ||A^-1||_F must lie below 1e7, the bound of fsa_rows.h.  Otherwise, and for any value that
//                  is not finite, the run ends with `false` and the caller keeps the old matrix.  On success w.Ai holds the result's inverse.
//   lda_run        within = V diag(l) V^T, whitening Wh = V diag(1 / sqrt(l)) with zero columns for l <= 0, S = Wh^T between Wh = U diag(m) U^T,
//                  m sorted descending, ldaMatrix = (Wh U_sorted)^T.
#pragma once
#include "mllr_jacobi.h"

namespace dsr {

static constexpr double kStcMaxCond = 1.0e7;              // as kFsaMaxCond
static constexpr int kStcMaxItns = 10;                    // MaxItns, eA:2389

MJ_FN bool stc_finite(double x) { return fabs(x) <= 1.7E308; }
MJ_FN bool stc_posdef(double lmin, double lmax, int n) { return lmin > 0.0 && lmin > 16.0 * n * 0x1p-53 * lmax; }

// a [n][n] symmetric -> diagonal, v [n][n] its eigenvectors (columns), cs [m], sq [2 nt], m = n rounded up to even
template <class Sync> MJ_FN bool stc_jacobi(double* a, double* v, double* cs, double* sq, int n, int tid, int nt, Sync sync)
{
  const int m = (n + 1) & ~1;
  for (int e = tid; e < n * n; e += nt) v[e] = (e / n == e % n) ? 1.0 : 0.0;
  sync();
  for (int sweep = 0; sweep <= kJacobiSweeps; sweep++) {
    mj_norms(a, n, sq, tid, nt);
    sync();
    double off, all; mj_norms_done(sq, nt, off, all);
    sync();
    if (!(all <= 1.7E308)) return false;
    if (mj_converged(off, all, n)) return true;
    if (sweep == kJacobiSweeps) break;
    for (int r = 0; r < m - 1; r++) {
      mj_angles(a, n, m, r, cs, tid, nt);
      sync();
      mj_rows(a, n, m, r, cs, tid, nt);
      sync();
      mj_cols(a, v, n, m, r, cs, tid, nt);
      sync();
    }
  }
  return false;
}

// a [n][n] (destroyed), v [n][n], t [n], cs [m], sq [2 nt] in fast memory; out [n][n] (zero unless positive definite), ev[0] = min, ev[1] = max
template <class Sync> MJ_FN bool stc_eig_run(double* a, double* v, double* t, double* cs, double* sq, int n, double* out, double* ev, int tid, int nt, Sync sync)
{
  if (!stc_jacobi(a, v, cs, sq, n, tid, nt, sync)) return false;
  double lmin = a[0], lmax = a[0];
  for (int e = 1; e < n; e++) { const double l = a[e * n + e]; if (l < lmin) lmin = l; if (l > lmax) lmax = l; }
  if (tid == 0) { ev[0] = lmin; ev[1] = lmax; }
  const bool pd = stc_posdef(lmin, lmax, n);
  for (int e = tid; e < n; e += nt) t[e] = pd ? 1.0 / a[e * n + e] : 0.0;
  sync();
  for (int e = tid; e < n * n; e += nt) {
    const int r = e / n, c = e - r * n;
    double sum = 0.0;
    for (int k = 0; k < n; k++) sum += t[k] * (v[r * n + k] * v[c * n + k]);
    out[e] = sum;
  }
  return true;
}

// the fast memory of stc_rows_run: doubles, then D ints
struct StcWork {
  double *A, *Ai, *c, *v, *dl, *u, *w, *red, *sc; int* piv;
  MJ_FN static size_t doubles(int D, int nt) { return 2 * (size_t) D * D + 5 * (size_t) D + 2 * (size_t) nt + 8; }
  MJ_FN void carve(double* base, int D, int nt)
  {
    A = base; Ai = A + (size_t) D * D; c = Ai + (size_t) D * D; v = c + D; dl = v + D; u = dl + D; w = u + D; red = w + D; sc = red + 2 * nt;
    piv = reinterpret_cast<int*>(sc + 8);
  }
};
// sc: 0 sign of det, 1 pivot, 2 refusal, 3 scale

template <class Sync> MJ_FN bool stc_invert(const StcWork& w, int D, int tid, int nt, Sync sync)
{
  double* Ai = w.Ai;
  for (int e = tid; e < D * D; e += nt) Ai[e] = w.A[e];
  if (tid == 0) { w.sc[0] = 1.0; w.sc[2] = 0.0; }
  sync();
  for (int k = 0; k < D; k++) {
    if (tid == 0) {
      int pr = k; double best = fabs(Ai[k * D + k]);
      for (int r = k + 1; r < D; r++) { const double x = fabs(Ai[r * D + k]); if (x > best || !(x == x)) { best = x; pr = r; } }
      const double pv = Ai[pr * D + k];
      w.piv[k] = pr; w.sc[1] = pv;
      if (!(best > 0.0) || !stc_finite(best)) w.sc[2] = 1.0;
      if ((pr != k) != (pv < 0.0)) w.sc[0] = -w.sc[0];
    }
    sync();
    if (w.sc[2] != 0.0) return false;
    const int pr = w.piv[k]; const double pv = w.sc[1];
    if (pr != k) for (int c = tid; c < D; c += nt) { const double x = Ai[k * D + c]; Ai[k * D + c] = Ai[pr * D + c]; Ai[pr * D + c] = x; }
    sync();
    for (int c = tid; c < D; c += nt) { w.dl[c] = (c == k ? 1.0 : Ai[k * D + c]) / pv; w.u[c] = Ai[c * D + k]; }
    sync();
    for (int e = tid; e < D * D; e += nt) {
      const int r = e / D, c = e - r * D;
      Ai[e] = r == k ? w.dl[c] : (c == k ? 0.0 : Ai[e]) - w.u[r] * w.dl[c];
    }
    sync();
  }
  for (int k = D - 1; k >= 0; k--) {                      // the row exchanges, undone as column exchanges in reverse order
    const int pr = w.piv[k];
    if (pr == k) continue;
    for (int r = tid; r < D; r += nt) { const double x = Ai[r * D + k]; Ai[r * D + k] = Ai[r * D + pr]; Ai[r * D + pr] = x; }
    sync();
  }
  return true;
}

// ||A||_F ||A^-1||_F < kStcMaxCond, and finite
template <class Sync> MJ_FN bool stc_cond_ok(const StcWork& w, int D, int tid, int nt, Sync sync)
{
  double sa = 0.0, si = 0.0;
  for (int e = tid; e < D * D; e += nt) { const double x = w.A[e], y = w.Ai[e]; sa += x * x; si += y * y; }
  w.red[2 * tid] = sa; w.red[2 * tid + 1] = si;
  sync();
  sa = 0.0; si = 0.0;
  for (int k = 0; k < nt; k++) { sa += w.red[2 * k]; si += w.red[2 * k + 1]; }
  sync();
  return sa * si < kStcMaxCond * kStcMaxCond;             // false for NaN
}

// w.A holds the matrix [D][D] on entry and the result on exit; GiInv [D][D][D] may be slow memory
template <class Sync> MJ_FN bool stc_rows_run(const StcWork& w, int D, int itns, const double* GiInv, double gamma, int tid, int nt, Sync sync)
{
  for (int it = 0; it < itns; it++) {
    if (!stc_invert(w, D, tid, nt, sync)) return false;
    for (int d = 0; d < D; d++) {
      if (!stc_cond_ok(w, D, tid, nt, sync)) return false;
      const double* Gi = GiInv + (size_t) d * D * D;
      const double sgn = w.sc[0];
      for (int j = tid; j < D; j += nt) w.c[j] = sgn * w.Ai[j * D + d];                   // the cofactors of row d over |det A|, eA:2425-2426
      sync();
      for (int j = tid; j < D; j += nt) { double s = 0.0; for (int k = 0; k < D; k++) s += Gi[(size_t) k * D + j] * w.c[k]; w.v[j] = s; }      // Gi^T c, eA:2429
      sync();
      if (tid == 0) {
        double f = 0.0;
        for (int j = 0; j < D; j++) f += w.v[j] * w.c[j];
        const double s = (f > 0.0) ? sqrt(gamma / f) : 0.0;                               // eA:2433-2438
        w.sc[3] = s;
        if (!(f > 0.0) || !stc_finite(f) || !(s > 0.0) || !stc_finite(s)) w.sc[2] = 1.0;
      }
      sync();
      if (w.sc[2] != 0.0) return false;
      const double s = w.sc[3];
      for (int j = tid; j < D; j += nt) { w.dl[j] = s * w.v[j] - w.A[d * D + j]; w.u[j] = w.Ai[j * D + d]; }
      sync();
      for (int c = tid; c < D; c += nt) { double t = 0.0; for (int r = 0; r < D; r++) t += w.dl[r] * w.Ai[r * D + c]; w.w[c] = t; }
      sync();
      const double denom = 1.0 + w.w[d];
      if (!(fabs(denom) > 0.0) || !stc_finite(denom)) return false;
      for (int e = tid; e < D * D; e += nt) { const int r = e / D, c = e - r * D; w.Ai[e] -= w.u[r] * (w.w[c] / denom); }
      for (int j = tid; j < D; j += nt) w.A[d * D + j] = s * w.v[j];                      // eA:2441-2442
      sync();
      if (tid == 0 && denom < 0.0) w.sc[0] = -sgn;
      sync();
    }
  }
  // the result itself: finite, and inside the bound (a later estimate and the W(2) statistics start from it); w.Ai is its inverse
  if (!stc_invert(w, D, tid, nt, sync) || !stc_cond_ok(w, D, tid, nt, sync)) return false;
  double bad = 0.0;
  for (int e = tid; e < D * D; e += nt) if (!stc_finite(w.A[e]) || !stc_finite(w.Ai[e])) bad = 1.0;
  w.red[2 * tid] = bad;
  sync();
  bad = 0.0;
  for (int k = 0; k < nt; k++) bad += w.red[2 * k];
  sync();
  return bad == 0.0;
}

// within, between [n][n] symmetric (may be slow memory); a, v, u [n][n], lam [2 n], cs [m], sq [2 nt], ord [n] in fast memory.
// L [n][n] the LDA matrix, ev [2 n]: the eigenvalues of `within` as found, then those of the whitened `between`, descending
template <class Sync> MJ_FN bool lda_run(const double* within, const double* between, double* a, double* v, double* u, double* lam, double* cs, double* sq, int* ord,
                                         int n, double* L, double* ev, int tid, int nt, Sync sync)
{
  for (int e = tid; e < n * n; e += nt) a[e] = within[e];
  sync();
  if (!stc_jacobi(a, v, cs, sq, n, tid, nt, sync)) return false;
  for (int e = tid; e < n; e += nt) { const double l = a[e * n + e]; ev[e] = l; lam[e] = (l <= 0.0) ? 0.0 : 1.0 / sqrt(l); }      // eA:2800-2810
  sync();
  for (int e = tid; e < n * n; e += nt) v[e] = lam[e % n] * v[e];
  sync();
  for (int e = tid; e < n * n; e += nt) {                  // between Wh
    const int r = e / n, c = e - r * n;
    double s = 0.0;
    for (int k = 0; k < n; k++) s += between[(size_t) r * n + k] * v[k * n + c];
    u[e] = s;
  }
  sync();
  for (int e = tid; e < n * n; e += nt) {                  // Wh^T (between Wh); element (r, c) takes the value computed for (max, min): symmetric bit for bit
    const int r0 = e / n, c0 = e - r0 * n, r = r0 > c0 ? r0 : c0, c = r0 > c0 ? c0 : r0;
    double s = 0.0;
    for (int k = 0; k < n; k++) s += v[k * n + r] * u[k * n + c];
    a[e] = s;
  }
  sync();
  if (!stc_jacobi(a, u, cs, sq, n, tid, nt, sync)) return false;
  for (int e = tid; e < n; e += nt) lam[n + e] = a[e * n + e];
  sync();
  if (tid == 0) {                                         // descending, eA:2822-2827 (std::sort there: the order of equal values is not pinned)
    for (int i = 0; i < n; i++) ord[i] = i;
    for (int i = 1; i < n; i++) { const int o = ord[i]; int j = i; while (j > 0 && lam[n + ord[j - 1]] < lam[n + o]) { ord[j] = ord[j - 1]; j--; } ord[j] = o; }
  }
  sync();
  for (int e = tid; e < n; e += nt) ev[n + e] = lam[n + ord[e]];
  for (int e = tid; e < n * n; e += nt) {                  // (Wh U_sorted)^T, eA:2829-2835
    const int i = e / n, j = e - i * n;
    double s = 0.0;
    for (int k = 0; k < n; k++) s += v[j * n + k] * u[k * n + ord[i]];
    L[e] = s;
  }
  sync();
  bool okAll = true;
  for (int e = 0; e < 2 * n; e++) if (!stc_finite(ev[e])) okAll = false;
  return okAll;
}

}  // namespace dsr
