// csrc/fsa_rows.h -- the estimation of a feature-space transform (FeatureSpaceAdaptationFeature::estimate, asr/train/fsa.cc:332-433, "fsa"),
// written per (thread, thread count) with the barrier passed in, so that k_fsa_eig / k_fsa_rows run it between __syncthreads() and a host
// program can run the same code with one thread and an empty barrier.  Every branch around a barrier depends on values all threads read alike.
//
//   fsa_eig_run    G_i (symmetric, n = dimN + 1) -> G_i^+ = V diag(1 / lambda_k if |lambda_k| / max |lambda| >= 1e-7 else 0) V^T by the cyclic
//                  Jacobi method of mllr_jacobi.h: what gsl_linalg_SV_decomp and MaxSingularValueRatio give for a symmetric matrix
//                  (fsa:367-372, 379-387, 419-426).  Element (r, c) is sum_k inv_k (v_rk v_ck), so the result is symmetric bit for bit.
//   fsa_invert     A -> A^-1 and det A in place by Gauss-Jordan elimination with row pivoting.
//   fsa_rows_run   iterN sweeps over the rows i (fsa:374-432): p = (0, det A . A^-1[:, i]) -- the cofactors of row i; the reference takes them
//                  from an SVD of A per row and uses |det|, whose sign cancels in w_i --, d = G_i^+ p, the quadratic in alpha, the root with the
//                  larger auxiliary value, w_i = G_i^+ (alpha p + z_i).  A^-1 and det follow a changed row by the rank-one update
//                  A'^-1 = A^-1 - (A^-1 e_i)(delta^T A^-1) / (1 + delta^T A^-1 e_i), det' = det (1 + delta^T A^-1 e_i), and are formed afresh at
//                  the start of every sweep.  Before every row, and for the result, ||A||_F ||A^-1||_F must lie below 1e7: then every singular
//                  value of A is above 1e-7 of the largest and the reference's rule in _calcCofactor (fsa:345-350) drops none.  Otherwise, and
//                  for any value that is not finite, the run ends with `false` and the caller keeps the old transform.
#pragma once
#include "mllr_jacobi.h"

namespace dsr {

static constexpr double kFsaMaxCond = 1.0e7;              // 1 / MaxSingularValueRatio (fsa:330)

MJ_FN bool fsa_finite(double x) { return fabs(x) <= 1.7E308; }

// a [n][n] (destroyed), v [n][n], t [n], cs [m], sq [2 nt] in fast memory; out [n][n]
template <class Sync> MJ_FN bool fsa_eig_run(double* a, double* v, double* t, double* cs, double* sq, int n, double* out, int tid, int nt, Sync sync)
{
  const int m = (n + 1) & ~1;
  for (int e = tid; e < n * n; e += nt) v[e] = (e / n == e % n) ? 1.0 : 0.0;
  sync();
  bool ok = false;
  for (int sweep = 0; sweep <= kJacobiSweeps; sweep++) {
    mj_norms(a, n, sq, tid, nt);
    sync();
    double off, all; mj_norms_done(sq, nt, off, all);
    sync();
    if (!(all <= 1.7E308)) break;
    if (mj_converged(off, all, n)) { ok = true; break; }
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
  if (!ok) return false;
  double lmax = 0.0;
  for (int e = 0; e < n; e++) { const double l = fabs(a[e * n + e]); if (l > lmax) lmax = l; }
  for (int e = tid; e < n; e += nt) { const double l = a[e * n + e]; t[e] = (fabs(l) / lmax >= 1.0e-07) ? 1.0 / l : 0.0; }      // fsa:382-385; 0 / 0 is dropped
  sync();
  for (int e = tid; e < n * n; e += nt) {
    const int r = e / n, c = e - r * n;
    double sum = 0.0;
    for (int k = 0; k < n; k++) sum += t[k] * (v[r * n + k] * v[c * n + k]);
    out[e] = sum;
  }
  return true;
}

// the fast memory of fsa_rows_run: doubles, then D ints
struct FsaWork {
  double *W, *Ai, *p, *d, *zr, *t, *wn, *dl, *u, *v, *red, *sc; int* piv;
  MJ_FN static size_t doubles(int D, int nt) { return (size_t) D * (D + 1) + (size_t) D * D + 5 * (size_t) (D + 1) + 3 * (size_t) D + 2 * (size_t) nt + 8; }
  MJ_FN void carve(double* base, int D, int nt)
  {
    const int n = D + 1;
    W = base; Ai = W + (size_t) D * n; p = Ai + (size_t) D * D; d = p + n; zr = d + n; t = zr + n; wn = t + n; dl = wn + n; u = dl + D; v = u + D;
    red = v + D; sc = red + 2 * nt; piv = reinterpret_cast<int*>(sc + 8);
  }
};
// sc: 0 det, 1 pivot, 2 refusal, 3 alpha

template <class Sync> MJ_FN bool fsa_invert(const FsaWork& w, int D, int tid, int nt, Sync sync)
{
  const int n = D + 1; double* Ai = w.Ai;
  for (int e = tid; e < D * D; e += nt) { const int r = e / D, c = e - r * D; Ai[e] = w.W[r * n + 1 + c]; }
  if (tid == 0) { w.sc[0] = 1.0; w.sc[2] = 0.0; }
  sync();
  for (int k = 0; k < D; k++) {
    if (tid == 0) {
      int pr = k; double best = fabs(Ai[k * D + k]);
      for (int r = k + 1; r < D; r++) { const double x = fabs(Ai[r * D + k]); if (x > best || !(x == x)) { best = x; pr = r; } }
      const double pv = Ai[pr * D + k];
      w.piv[k] = pr; w.sc[1] = pv;
      if (!(best > 0.0) || !fsa_finite(best)) w.sc[2] = 1.0;
      w.sc[0] = (pr != k ? -w.sc[0] : w.sc[0]) * pv;
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

// ||A||_F ||A^-1||_F < kFsaMaxCond, and finite
template <class Sync> MJ_FN bool fsa_cond_ok(const FsaWork& w, int D, int tid, int nt, Sync sync)
{
  const int n = D + 1;
  double sa = 0.0, si = 0.0;
  for (int e = tid; e < D * D; e += nt) { const int r = e / D, c = e - r * D; const double x = w.W[r * n + 1 + c], y = w.Ai[e]; sa += x * x; si += y * y; }
  w.red[2 * tid] = sa; w.red[2 * tid + 1] = si;
  sync();
  sa = 0.0; si = 0.0;
  for (int k = 0; k < nt; k++) { sa += w.red[2 * k]; si += w.red[2 * k + 1]; }
  sync();
  const double c2 = sa * si;
  return c2 < kFsaMaxCond * kFsaMaxCond && fsa_finite(w.sc[0]);
}

// w.W holds the transform [D][D + 1] on entry and the result on exit; Ginv [D][n][n] and z [D][n] may be slow memory
template <class Sync> MJ_FN bool fsa_rows_run(const FsaWork& w, int D, int iterN, const double* Ginv, const double* z, double beta, int tid, int nt, Sync sync)
{
  const int n = D + 1;
  for (int it = 0; it < iterN; it++) {
    if (!fsa_invert(w, D, tid, nt, sync)) return false;
    for (int i = 0; i < D; i++) {
      if (!fsa_cond_ok(w, D, tid, nt, sync)) return false;
      const double* Gi = Ginv + (size_t) i * n * n;
      const double det = w.sc[0];
      for (int j = tid; j < n; j += nt) { w.p[j] = j == 0 ? 0.0 : det * w.Ai[(j - 1) * D + i]; w.zr[j] = z[(size_t) i * n + j]; }
      sync();
      for (int j = tid; j < n; j += nt) { double s = 0.0; for (int k = 0; k < n; k++) s += Gi[(size_t) k * n + j] * w.p[k]; w.d[j] = s; }      // G_i^+ is symmetric
      sync();
      if (tid == 0) {
        double term1 = 0.0, term2 = 0.0;
        for (int j = 0; j < n; j++) { term1 += w.d[j] * w.p[j]; term2 += w.d[j] * w.zr[j]; }
        const double term3 = term2 / (2 * term1), term4 = sqrt(term3 * term3 + beta / term1);
        const double alpha1 = -1.0 * term3 + term4, alpha2 = -1.0 * term3 - term4;
        const double kullback1 = beta * log(fabs(alpha1 * term1 + term2)) - 0.5 * alpha1 * alpha1 * term1;
        const double kullback2 = beta * log(fabs(alpha2 * term1 + term2)) - 0.5 * alpha2 * alpha2 * term1;
        const double alpha = (kullback2 > kullback1) ? alpha2 : alpha1;
        w.sc[3] = alpha;
        if (!fsa_finite(alpha)) w.sc[2] = 1.0;
      }
      sync();
      if (w.sc[2] != 0.0) return false;
      const double alpha = w.sc[3];
      for (int j = tid; j < n; j += nt) w.t[j] = alpha * w.p[j] + w.zr[j];
      sync();
      for (int j = tid; j < n; j += nt) { double s = 0.0; for (int k = 0; k < n; k++) s += Gi[(size_t) k * n + j] * w.t[k]; w.wn[j] = s; }
      sync();
      for (int c = tid; c < D; c += nt) { w.dl[c] = w.wn[c + 1] - w.W[i * n + 1 + c]; w.u[c] = w.Ai[c * D + i]; }
      sync();
      for (int c = tid; c < D; c += nt) { double s = 0.0; for (int r = 0; r < D; r++) s += w.dl[r] * w.Ai[r * D + c]; w.v[c] = s; }
      sync();
      const double denom = 1.0 + w.v[i];
      if (!(fabs(denom) > 0.0) || !fsa_finite(denom)) return false;
      for (int e = tid; e < D * D; e += nt) { const int r = e / D, c = e - r * D; w.Ai[e] -= w.u[r] * (w.v[c] / denom); }
      for (int j = tid; j < n; j += nt) w.W[i * n + j] = w.wn[j];
      sync();
      if (tid == 0) w.sc[0] = det * denom;
      sync();
    }
  }
  // the result itself: finite, and A inside the bound (a later estimate starts from it)
  if (!fsa_invert(w, D, tid, nt, sync) || !fsa_cond_ok(w, D, tid, nt, sync)) return false;
  double bad = 0.0;
  for (int e = tid; e < D * n; e += nt) if (!fsa_finite(w.W[e])) bad = 1.0;
  w.red[2 * tid] = bad;
  sync();
  bad = 0.0;
  for (int k = 0; k < nt; k++) bad += w.red[2 * k];
  sync();
  return bad == 0.0;
}

}  // namespace dsr
