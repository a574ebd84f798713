// csrc/k_mk.hip -- maximum empirical kurtosis beamforming (btk/lib/mkBeamforming.py: MEKSubbandBeamformer_pr / _nrm): the active weights of a GSC
// for a whole utterance, every (utterance, bin) an optimisation problem of its own, minimised inside one kernel launch.
//
//   Y_t = (wq - B wa)^H X_t = y0_t - sum_j conj(wa_j) Z_t,j      y0_t = wq^H X_t,  Z_t = B^H X_t   (k_mk_prepare, once per call)
//   cost  fun_MK  = -(exY4 - beta exY2^2) + alpha |wa|^2          (mkBeamforming.py:302-336, 436-456)
//   grad  dfun_MK = -(dexY4 - 2 beta exY2 dexY2) + alpha wa       (:338-383, 458-484): the derivative w.r.t. conj(wa) = HALF the real gradient
//   _pr : conjugate_pr as btk/minimizer/conjugate_pr.c + directional_minimize.c state the algorithm, driver loop :486-534
//   _nrm: steepest descent (trial x - step g / |g|, step x tol on a rejected trial, x 2 after a clean step), driver loop :579-658, weights
//         clipped to length |gamma| in cost, gradient and regulariser (the gradient ignores the clipping's Jacobian, as there)
//
// Reduction order (an interface: tests/mk_np.py restates it): 64 partial sums, partial p adds frames p, p + 64, ... in increasing order, then
// a butterfly over the wave (lane ^ 1, ^ 2, ... ^ 32) = a fixed binary tree; sums are divided by N after the reduction.  Built with
// -ffp-contract=off, so a run repeats bit for bit and the LDS-resident and the streamed path agree bit for bit.  |v| of a packed vector
// is the square root of the sequential sum of squares.
//
// One wave (64 lanes) owns a problem.  Every lane carries the same scalars (the butterfly leaves the same sum in every lane), so control flow
// is uniform; the minimiser's vectors (x, g, trial points, direction) live in LDS and are updated lane-parallel.
#include "launch.h"
#include "gsc_weights.h"
#include <complex>
#include <cmath>

// k_beamform.hip defines it inside its extern "C" block, so it has C linkage
extern "C" { namespace dsr { bool bf_gsc_fixed_weights(const dsr_bf* s, int* M, int* C, int* halfBandShift, const std::complex<double>** wq, const std::complex<double>** B); } }

namespace dsr {
typedef std::complex<double> zc;
static const int MK_FRAME_LDS = 128 * 1024;        // LDS a workgroup gives its frames (of the 160 KiB of a CU; the rest: minimiser vectors)
static const int MK_NVEC = 7;                      // x, g, x1, x2, p, g0, wn

struct MkParams { int kind, maxItns, evalCap; double alpha, beta, tol, stopTol, diffStop, stepSize; };

struct MkState {
  int M = 0, C = 0; bool haveFixed = false, forceStreamed = false;
  std::vector<zc> wq, B;                           // [F][C], [F][C][C-1]
  MkParams p;
  double gamma = -1.0;
  DevBuf<double2> d_wq, d_B, d_scr; DevBuf<double> d_gam; DevBuf<float2> d_w; bool dirty = true;
  MkState() { p.kind = DSR_MK_PR; p.maxItns = 40; p.evalCap = DSR_MK_EVAL_CAP; p.alpha = 1.0e-2; p.beta = 3.0; p.tol = 1.0e-3; p.stopTol = 1.0e-2; p.diffStop = 1.0e-5; p.stepSize = 0.01; }
};

// frames accumObservations(sFrame, eFrame, R) keeps (:97-143): s = first + k R, first the smallest multiple of R >= sFrame, s < lim
__host__ __device__ static inline int mk_first(int sFrame, int R) { const int s = sFrame < 0 ? 0 : sFrame; return ((s + R - 1) / R) * R; }
__host__ __device__ static inline int mk_count(int first, int R, int lim) { return lim > first ? (lim - first + R - 1) / R : 0; }

// ---- 1. prepare: y0 and Z of every selected frame.  Lanes run over bins (X is contiguous in f); a tile of 64 bins x TK frames x C values
// goes through LDS so that the scratch [U][F][Tsel][C] is written in runs of TK C values.
template <int CT>
__global__ __launch_bounds__(64) void k_mk_prepare(const float2* __restrict__ X, const double2* __restrict__ wq, const double2* __restrict__ B,
                                                   const int* __restrict__ nframes, double2* __restrict__ scr, int Crt, int Tmax, int F, int Tsel,
                                                   int first, int R, int eLim, int TK)
{
  const int C = CT ? CT : Crt, n = C - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2* tile = reinterpret_cast<double2*>(smem);                  // [64][TK * C + 1]
  const int u = blockIdx.z, f0 = blockIdx.x * 64, k0 = blockIdx.y * TK, lane = threadIdx.x, f = f0 + lane, pitch = TK * C + 1;
  int lim = eLim; if (nframes) { const int nf = nframes[u]; if (nf < lim) lim = nf; }
  int kn = mk_count(first, R, lim) - k0; if (kn > TK) kn = TK;
  if (kn <= 0) return;                                               // the same for every lane
  if (f < F) {
    const float2* Xu = X + (long) u * C * Tmax * F;
    const double2* wqf = wq + (long) f * C; const double2* Bf = B + (long) f * C * n;
    for (int kk = 0; kk < kn; kk++) {
      const long t = first + (long) (k0 + kk) * R;
      double2 xr[CT ? CT : 1];
      if (CT) for (int c = 0; c < C; c++) { const float2 v = Xu[((long) c * Tmax + t) * F + f]; xr[CT ? c : 0] = make_double2((double) v.x, (double) v.y); }
      double2* o = tile + (long) lane * pitch + kk * C;
      for (int e = 0; e < C; e++) {                                  // e = 0: conj(wq) . x; e = 1 + j: conj(B[:, j]) . x; channels in increasing order
        double ar = 0.0, ai = 0.0;
        for (int c = 0; c < C; c++) {
          double2 x;
          if (CT) x = xr[CT ? c : 0]; else { const float2 v = Xu[((long) c * Tmax + t) * F + f]; x = make_double2((double) v.x, (double) v.y); }
          const double2 w = e == 0 ? wqf[c] : Bf[c * n + (e - 1)];
          ar += w.x * x.x + w.y * x.y; ai += w.x * x.y - w.y * x.x;
        }
        o[e] = make_double2(ar, ai);
      }
    }
  }
  __syncthreads();
  const int nb = F - f0 < 64 ? F - f0 : 64, seg = kn * C;
  for (int i = lane; i < nb * seg; i += 64) {
    const int b = i / seg, r = i - b * seg;
    scr[((long) ((long) u * F + f0 + b) * Tsel + k0) * C + r] = tile[(long) b * pitch + r];
  }
}

// ---- 2. minimise
struct MkCtx {
  const double2* scr; const double2* zs; double* wn;
  int resident, T, Tn, C, n, kind, lane;
  double alpha, beta, ag, prevY2, prevY4, prevN, N;
  double S2, S4;                                                     // sums of |Y|^2, |Y|^4 of the last evaluation
};

// (not wave_sum of dev_math.h: this butterfly runs from distance 1 up, the other from 32 down, and the two round differently)
__device__ __forceinline__ double mk_wsum(double v) { for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m); return v; }
__device__ __forceinline__ double2 mk_ld(const MkCtx& c, int t, int e) { return c.resident ? c.zs[(long) e * c.Tn + t] : c.scr[(long) t * c.C + e]; }

// cost (returned) and, with gout, the packed gradient at the packed weights xv; xv, gout and c.wn are LDS vectors of 2n doubles
template <int CT>
__device__ double mk_eval(MkCtx& c, const double* xv, double* gout)
{
  const int n = c.n, n2 = 2 * n, lane = c.lane;
  __syncthreads();
  double s = 0.0;
  for (int k = 0; k < n; k++) s += xv[2 * k] * xv[2 * k] + xv[2 * k + 1] * xv[2 * k + 1];
  double nr = 0.0; bool clip = false;
  if (c.kind == DSR_MK_NRM) { nr = sqrt(s); clip = nr > c.ag; }      // normalizeWeight (:549-559)
  for (int i = lane; i < n2; i += 64) c.wn[i] = clip ? (c.ag * xv[i]) / nr : xv[i];
  __syncthreads();
  const double* wn = c.wn;
  double s2 = 0.0;
  for (int k = 0; k < n; k++) s2 += wn[2 * k] * wn[2 * k] + wn[2 * k + 1] * wn[2 * k + 1];
  const double rterm = c.alpha * s2;
  constexpr int JB = CT ? CT - 1 : 8;                                // gradient entries accumulated per pass over the frames
  double S2 = 0.0, S4 = 0.0, exY2 = 0.0;
  for (int j0 = 0; j0 < n; j0 += JB) {
    double a2r[JB], a2i[JB], a4r[JB], a4i[JB];
    for (int jj = 0; jj < JB; jj++) { a2r[jj] = 0.0; a2i[jj] = 0.0; a4r[jj] = 0.0; a4i[jj] = 0.0; }
    for (int t = lane; t < c.T; t += 64) {
      const double2 y0 = mk_ld(c, t, 0);
      double sr = 0.0, si = 0.0;
      for (int j = 0; j < n; j++) { const double2 z = mk_ld(c, t, 1 + j); const double wr = wn[2 * j], wi = wn[2 * j + 1]; sr += wr * z.x + wi * z.y; si += wr * z.y - wi * z.x; }
      const double Yr = y0.x - sr, Yi = y0.y - si, y2 = Yr * Yr + Yi * Yi;
      if (j0 == 0) { S2 += y2; S4 += y2 * y2; }
      if (gout)
        for (int jj = 0; jj < JB; jj++) {
          const int j = j0 + jj;
          if (j < n) {
            const double2 z = mk_ld(c, t, 1 + j);
            const double qr = z.x * Yr + z.y * Yi, qi = z.y * Yr - z.x * Yi;      // Z conj(Y)
            a2r[jj] += qr; a2i[jj] += qi; a4r[jj] += y2 * qr; a4i[jj] += y2 * qi;
          }
        }
    }
    if (j0 == 0) { S2 = mk_wsum(S2); S4 = mk_wsum(S4); exY2 = (c.prevY2 / c.N) * c.prevN + S2 / c.N; }
    if (!gout) break;
    for (int jj = 0; jj < JB; jj++) {
      const int j = j0 + jj;
      if (j < n) {
        const double A2r = mk_wsum(a2r[jj]), A2i = mk_wsum(a2i[jj]), A4r = mk_wsum(a4r[jj]), A4i = mk_wsum(a4i[jj]);
        const double d4r = (-2.0 * A4r) / c.N, d4i = (-2.0 * A4i) / c.N, d2r = (-A2r) / c.N, d2i = (-A2i) / c.N;   // BHX = -Z (:474-477)
        const double cc = (2.0 * c.beta) * exY2;
        const double dkr = d4r - cc * d2r, dki = d4i - cc * d2i;
        if (lane == 0) { gout[2 * j] = (-dkr) + c.alpha * wn[2 * j]; gout[2 * j + 1] = (-dki) + c.alpha * wn[2 * j + 1]; }
      }
    }
  }
  c.S2 = S2; c.S4 = S4;
  const double exY4 = (c.prevY4 / c.N) * c.prevN + S4 / c.N;
  const double kurt = exY4 - (c.beta * exY2) * exY2;
  __syncthreads();
  return (0.0 - kurt) + rterm;
}

// lane-parallel vector pieces; every one starts with a barrier, so a value written by the piece before is seen and nobody still reads what is overwritten
__device__ __forceinline__ void mk_copy(double* d, const double* s, int n2, int lane) { __syncthreads(); for (int i = lane; i < n2; i += 64) d[i] = s[i]; }
// take_step: dx = a p, x1 = x + dx
__device__ __forceinline__ void mk_step(double* x1, const double* x, const double* p, double a, int n2, int lane)
{ __syncthreads(); for (int i = lane; i < n2; i += 64) { const double dx = a * p[i]; x1[i] = x[i] + dx; } }
__device__ __forceinline__ double mk_dot(const double* a, const double* b, int n2) { __syncthreads(); double r = 0.0; for (int i = 0; i < n2; i++) r += a[i] * b[i]; return r; }
__device__ __forceinline__ double mk_nrm(const double* a, int n2) { return sqrt(mk_dot(a, a, n2)); }

template <int CT>
__global__ __launch_bounds__(64) void k_mk_minimize(const double2* __restrict__ scrAll, const double* __restrict__ gam, const int* __restrict__ nframes,
                                                    double* __restrict__ wa, double* __restrict__ stats, int* __restrict__ info, double* __restrict__ fout,
                                                    double* __restrict__ gradOut, MkParams P, int Crt, int U, int F, int fbin, int Tsel, int first, int R,
                                                    int eLim, int resident, int evalOnly)
{
  const int C = CT ? CT : Crt, n = C - 1, n2 = 2 * n, lane = threadIdx.x;
  const int u = fbin < 0 ? blockIdx.x / F : blockIdx.x, f = fbin < 0 ? blockIdx.x - u * F : fbin;
  const long pix = (long) u * F + f, UF = (long) U * F;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* vec = reinterpret_cast<double*>(smem);
  double *X = vec, *G = vec + n2, *X1 = vec + 2 * n2, *X2 = vec + 3 * n2, *Pd = vec + 4 * n2, *G0 = vec + 5 * n2;
  MkCtx c;
  c.wn = vec + 6 * n2;
  double2* zs = reinterpret_cast<double2*>(smem + (((size_t) MK_NVEC * n2 * sizeof(double) + 15) & ~(size_t) 15));
  int lim = eLim; if (nframes) { const int nf = nframes[u]; if (nf < lim) lim = nf; }
  c.T = mk_count(first, R, lim); c.Tn = Tsel; c.C = C; c.n = n; c.kind = P.kind; c.lane = lane; c.resident = resident;
  c.scr = scrAll + pix * Tsel * C; c.zs = zs;
  c.alpha = P.alpha; c.beta = P.beta; c.ag = fabs(gam[f]);
  c.prevY2 = stats ? stats[pix] : 0.0; c.prevY4 = stats ? stats[UF + pix] : 0.0; c.prevN = stats ? stats[2 * UF + pix] : 0.0;
  c.N = c.prevN + (double) c.T; c.S2 = 0.0; c.S4 = 0.0;
  double* wap = wa + pix * n2;
  for (int i = lane; i < n2; i += 64) X[i] = wap[i];
  if (resident) for (int i = lane; i < c.T * C; i += 64) { const int t = i / C, e = i - t * C; zs[(long) e * Tsel + t] = c.scr[i]; }
  __syncthreads();

  if (evalOnly) {
    if (c.T == 0) {                                                  // no frame: nothing to average
      if (lane == 0) { fout[pix] = nan(""); for (int i = 0; i < n2; i++) gradOut[pix * n2 + i] = nan(""); }
      return;
    }
    const double fv = mk_eval<CT>(c, X, G);
    if (lane == 0) fout[pix] = fv;
    for (int i = lane; i < n2; i += 64) gradOut[pix * n2 + i] = G[i];
    return;
  }

  int iters = 0, evals = 0, failed = 0, reason = DSR_MK_EXIT_MAX_ITERATIONS;
  double fcur = 0.0;
  bool skipped = c.T == 0;
  if (!skipped) { fcur = mk_eval<CT>(c, X, G); evals = 1; skipped = !isfinite(fcur); }
  if (skipped) {
    if (lane == 0) { info[pix * 4] = 0; info[pix * 4 + 1] = evals; info[pix * 4 + 2] = 0; info[pix * 4 + 3] = DSR_MK_EXIT_SKIPPED; fout[pix] = c.T == 0 ? nan("") : fcur; }
    return;
  }
  double preMi = 10000.0;

  if (P.kind == DSR_MK_PR) {
    // conjugate_pr: set
    mk_copy(Pd, G, n2, lane); mk_copy(G0, G, n2, lane);
    double pnorm = mk_nrm(G, n2), g0norm = pnorm, step = P.stepSize; int cgIter = 0;
    for (int itera = 0; itera < P.maxItns; itera++) {
      int itEvals = 0;
      // iterate
      if (pnorm == 0.0 || g0norm == 0.0) { reason = DSR_MK_EXIT_NO_PROGRESS; break; }
      double fa = fcur, stepa = 0.0, stepc = step;
      double pg = mk_dot(Pd, G, n2);
      const double dir = pg >= 0.0 ? 1.0 : -1.0, lam = dir / pnorm;
      mk_step(X1, X, Pd, -stepc * lam, n2, lane);
      double fc = mk_eval<CT>(c, X1, nullptr); evals++; itEvals++;
      // intermediate_point: a point b between a and c with f(b) < f(a), from the parabola through f(a), f'(a), f(c)
      double stepb = 0.0, fb = 0.0; bool capped = false;
      { double ic = stepc, ifc = fc;
        for (;;) {
          const double uu = fabs(pg * lam * ic);
          stepb = 0.5 * ic * uu / ((ifc - fa) + uu);
          if (itEvals >= P.evalCap) { capped = true; break; }
          mk_step(X1, X, Pd, -stepb * lam, n2, lane);
          fb = mk_eval<CT>(c, X1, nullptr); evals++; itEvals++;
          if (fb >= fa && stepb > 0.0) { ifc = fb; ic = stepb; failed++; continue; }
          break;
        } }
      if (capped) { reason = DSR_MK_EXIT_EVAL_CAP; break; }
      (void) mk_eval<CT>(c, X1, G); evals++; itEvals++;
      if (stepb == 0.0) { reason = DSR_MK_EXIT_NO_PROGRESS; break; }
      // minimize: at most 10 parabolic / golden-section trials along the direction
      double uS = stepb, vS = stepa, wS = stepc, fu = fb, fv = fa, fw = fc;
      double old2 = fabs(wS - vS), old1 = fabs(vS - uS);
      mk_copy(X2, X1, n2, lane);
      double fnew = fb, stepNew = stepb, g1norm = mk_nrm(G, n2);
      for (int li = 1; li <= 10; li++) {
        const double dw = wS - uS, dv = vS - uS; double du = 0.0;
        const double e1 = ((fv - fu) * dw * dw + (fu - fw) * dv * dv);
        const double e2 = 2.0 * ((fv - fu) * dw + (fu - fw) * dv);
        if (e2 != 0.0) du = e1 / e2;
        double stepm;
        if (du > 0.0 && du < (stepc - stepb) && fabs(du) < 0.5 * old2) stepm = uS + du;
        else if (du < 0.0 && du > (stepa - stepb) && fabs(du) < 0.5 * old2) stepm = uS + du;
        else if ((stepc - stepb) > (stepb - stepa)) stepm = 0.38 * (stepc - stepb) + stepb;
        else stepm = stepb - 0.38 * (stepb - stepa);
        mk_step(X1, X, Pd, -stepm * lam, n2, lane);
        const double fm = mk_eval<CT>(c, X1, nullptr); evals++; itEvals++;
        if (fm > fb) {
          if (fm < fv) { wS = vS; vS = stepm; fw = fv; fv = fm; }
          else if (fm < fw) { wS = stepm; fw = fm; }
          if (stepm < stepb) { stepa = stepm; fa = fm; } else { stepc = stepm; fc = fm; }
        } else if (fm <= fb) {
          old2 = old1; old1 = fabs(uS - stepm);
          wS = vS; vS = uS; uS = stepm; fw = fv; fv = fu; fu = fm;
          mk_copy(X2, X1, n2, lane);
          (void) mk_eval<CT>(c, X1, G); evals++; itEvals++;
          pg = mk_dot(Pd, G, n2);
          const double gnorm1 = mk_nrm(G, n2);
          fnew = fm; stepNew = stepm; g1norm = gnorm1;
          if (fabs(pg * lam / gnorm1) < P.tol) break;
          if (stepm < stepb) { stepc = stepb; fc = fb; stepb = stepm; fb = fm; }
          else { stepa = stepb; fa = fb; stepb = stepm; fb = fm; }
        } else break;                                                // fm is not a number
      }
      fcur = fnew; step = stepNew;
      mk_copy(X, X2, n2, lane);
      // the next direction: restart every 2(C-1) iterations, else Polak-Ribiere
      cgIter = (cgIter + 1) % n2;
      if (cgIter == 0) { mk_copy(Pd, G, n2, lane); pnorm = g1norm; }
      else {
        __syncthreads();
        for (int i = lane; i < n2; i += 64) G0[i] = G0[i] + (-1.0) * G[i];
        const double g0g1 = mk_dot(G0, G, n2), beta = g0g1 / (g0norm * g0norm);
        __syncthreads();
        for (int i = lane; i < n2; i += 64) { const double q = (-beta) * Pd[i]; Pd[i] = q + G[i]; }
        pnorm = mk_nrm(Pd, n2);
      }
      g0norm = g1norm; mk_copy(G0, G, n2, lane);
      iters++;
      // driver (:517-531)
      const double gn = mk_nrm(G, n2);
      if (gn < P.stopTol) { reason = DSR_MK_EXIT_GRADIENT; break; }
      if (fabs(preMi - fcur) < P.diffStop) { reason = DSR_MK_EXIT_DIFFERENCE; break; }
      preMi = fcur;
    }
  } else {
    // steepest descent
    double step = P.stepSize;
    for (int itera = 0; itera < P.maxItns; itera++) {
      int itEvals = 0;
      const double f0 = fcur; bool fail = false, noprog = false, capped = false;
      const double gnorm = mk_nrm(G, n2);
      if (gnorm == 0.0) { reason = DSR_MK_EXIT_NO_PROGRESS; break; }
      double f1 = 0.0;
      for (;;) {
        mk_step(X1, X, G, (-step) / gnorm, n2, lane);
        __syncthreads();
        bool same = true; for (int i = 0; i < n2; i++) same = same && (X1[i] == X[i]);
        if (same) { noprog = true; break; }
        if (itEvals >= P.evalCap) { capped = true; break; }
        f1 = mk_eval<CT>(c, X1, G0); evals++; itEvals++;            // G0 holds the trial's gradient
        if (f1 > f0) { fail = true; failed++; step *= P.tol; continue; }
        break;
      }
      if (noprog) { reason = DSR_MK_EXIT_NO_PROGRESS; break; }
      if (capped) { reason = DSR_MK_EXIT_EVAL_CAP; break; }
      step *= fail ? P.tol : 2.0;
      mk_copy(X, X1, n2, lane); mk_copy(G, G0, n2, lane); fcur = f1;
      iters++;
      // driver (:612-643): both stop tests only after the third iteration
      const double gn = mk_nrm(G, n2);
      if (gn < P.stopTol && itera > 2) { reason = DSR_MK_EXIT_GRADIENT; break; }
      if (fabs(preMi - fcur) < P.diffStop && itera > 2) { reason = DSR_MK_EXIT_DIFFERENCE; break; }
      preMi = fcur;
    }
    // :646-654: the weights are normalised, storeStatistics (:410-420) with N already advanced
    __syncthreads();
    double s = 0.0; for (int k = 0; k < n; k++) s += X[2 * k] * X[2 * k] + X[2 * k + 1] * X[2 * k + 1];
    const double nr = sqrt(s);
    __syncthreads();
    if (nr > c.ag) for (int i = lane; i < n2; i += 64) X[i] = (c.ag * X[i]) / nr;
    if (stats) {
      (void) mk_eval<CT>(c, X, nullptr);                             // not counted: the reference's storeStatistics pass
      if (lane == 0) { stats[pix] = c.prevY2 + c.S2 / c.N; stats[UF + pix] = c.prevY4 + c.S4 / c.N; stats[2 * UF + pix] = c.N; }
    }
  }
  __syncthreads();
  for (int i = lane; i < n2; i += 64) wap[i] = X[i];
  if (lane == 0) { info[pix * 4] = iters; info[pix * 4 + 1] = evals; info[pix * 4 + 2] = failed; info[pix * 4 + 3] = reason; fout[pix] = fcur; }
}

// ---- 3. apply with per-utterance weights: W[u][f][c] = wq - B wa (fp64, rounded to fp32 as dsr_bf's effective weights are), then w^H X
__global__ void k_mk_weff(const double2* __restrict__ wq, const double2* __restrict__ B, const double* __restrict__ wa, float2* __restrict__ W, int U, int C, int F)
{
  const long i = (long) blockIdx.x * blockDim.x + threadIdx.x; const int n = C - 1;
  if (i >= (long) U * F * C) return;
  const int c = (int) (i % C); const long uf = i / C; const int f = (int) (uf % F);
  double lr = 0.0, li = 0.0;
  for (int j = 0; j < n; j++) {
    const double2 b = B[((long) f * C + c) * n + j]; const double wr = wa[(uf * n + j) * 2], wi = wa[(uf * n + j) * 2 + 1];
    lr += b.x * wr - b.y * wi; li += b.x * wi + b.y * wr;
  }
  const double2 q = wq[(long) f * C + c];
  W[i] = make_float2((float) (q.x - lr), (float) (q.y - li));
}
__global__ __launch_bounds__(256) void k_mk_apply(const float2* __restrict__ X, const float2* __restrict__ W, float2* __restrict__ Y, int C, int F, long perUtt)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* w = reinterpret_cast<float2*>(smem);
  const int u = blockIdx.y;
  for (int i = threadIdx.x; i < F * C; i += blockDim.x) w[i] = W[(long) u * F * C + i];
  __syncthreads();
  const float2* Xu = X + (long) u * C * perUtt; float2* Yu = Y + (long) u * perUtt;
  for (long idx = (long) blockIdx.x * blockDim.x + threadIdx.x; idx < perUtt; idx += (long) gridDim.x * blockDim.x) {
    const int f = (int) (idx % F);
    float2 acc = make_float2(0.f, 0.f);
    for (int c = 0; c < C; c++) {
      const float2 x = Xu[(long) c * perUtt + idx]; const float2 wc = w[f * C + c];
      acc.x += wc.x * x.x + wc.y * x.y; acc.y += wc.x * x.y - wc.y * x.x;
    }
    Yu[idx] = acc;
  }
}

// ---- dispatch, in one place: the launches below and dsr_mk_path read it
using MkCt = ints<4, 6, 8>;                                          // the channel counts k_mk_* are instantiated for besides the run-time 0
using MkCtAll = ints<4, 6, 8, 0>;
struct MkPath { int ct, residence, tcap; size_t ldsBytes; };
static MkPath mk_path(int C, int Tsel, bool forceStreamed)
{
  MkPath r; r.ct = has_value(MkCt{}, C) ? C : 0;
  r.tcap = MK_FRAME_LDS / (16 * C);
  r.residence = (Tsel <= r.tcap && !forceStreamed) ? DSR_MK_FRAMES_LDS : DSR_MK_FRAMES_STREAMED;
  const size_t vb = ((size_t) MK_NVEC * 2 * (C - 1) * sizeof(double) + 15) & ~(size_t) 15;
  r.ldsBytes = vb + (r.residence == DSR_MK_FRAMES_LDS ? (size_t) (Tsel > 0 ? Tsel : 0) * C * 16 : 0);
  return r;
}

static void mk_upload(MkState& s)
{
  if (!s.dirty) return;
  const int C = s.C, F = s.M / 2 + 1, n = C - 1;
  std::vector<double2> a((size_t) F * C), b((size_t) F * C * n); std::vector<double> g(F);
  for (size_t i = 0; i < a.size(); i++) a[i] = make_double2(s.wq[i].real(), s.wq[i].imag());
  for (size_t i = 0; i < b.size(); i++) b[i] = make_double2(s.B[i].real(), s.B[i].imag());
  for (int f = 0; f < F; f++) {                                      // gamma < 0: |wq| (:552-555)
    double q = 0.0; for (int c = 0; c < C; c++) q += gsc::abs2(s.wq[(size_t) f * C + c]);
    g[f] = s.gamma < 0 ? std::sqrt(q) : s.gamma;
  }
  s.d_wq.upload(a); s.d_B.upload(b); s.d_gam.upload(g); s.dirty = false;
}

static void mk_run(MkState& s, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, int fbin, double* wa, double* stats,
                   int32_t* info, double* cost, double* grad, bool evalOnly, hipStream_t st)
{
  if (!s.haveFixed) throw Error(DSR_E_ERROR, "call calcFixedWeights() or setFixedWeights() once");
  const int C = s.C, F = s.M / 2 + 1;
  if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "bad batch U=%d Tmax=%d", U, Tmax);
  if (fbin >= F) throw Error(DSR_E_INDEX, "frequency bin %d > fftLen/2 %d", fbin, F - 1);
  if (U > 65535) throw Error(DSR_E_DIMENSION, "at most 65535 utterances a call (%d)", U);
  if (R < 1) R = 1;                                                  // :106-107
  if (R > Tmax) R = Tmax > 0 ? Tmax : 1;                             // the same frames (only s = 0 is a multiple), no overflow in mk_first
  if (sFrame > Tmax) sFrame = Tmax;
  if (U == 0) return;
  require_device();
  mk_upload(s);
  const int first = mk_first(sFrame, R), eLim = eFrame < Tmax ? eFrame : Tmax, Tsel = mk_count(first, R, eLim);
  const MkPath pa = mk_path(C, Tsel, s.forceStreamed);
  s.d_scr.reserve((size_t) U * F * (Tsel > 0 ? Tsel : 1) * C);
  if (Tsel > 0) {
    int TK = 32768 / (64 * C * 16); if (TK < 1) TK = 1; if (TK > 8) TK = 8;
    const size_t lds = (size_t) 64 * (TK * C + 1) * 16;
    const dim3 grid((unsigned) cdiv(F, 64), (unsigned) cdiv(Tsel, TK), (unsigned) U);
    if (grid.y > 65535) throw Error(DSR_E_DIMENSION, "too many frames (%d)", Tsel);
    if (!for_value(MkCtAll{}, pa.ct, [&](auto ct) {
          launch(k_mk_prepare<ct()>, grid, dim3(64), lds, st, (const float2*) X, s.d_wq.p, s.d_B.p, nframes, s.d_scr.p, C, Tmax, F, Tsel, first, R, eLim, TK); }))
      throw Error(DSR_E_ERROR, "MKSubbandBeamformer: no kernel k_mk_prepare<%d>", pa.ct);
  }
  const unsigned blocks = fbin < 0 ? (unsigned) ((long) U * F) : (unsigned) U;
  const int resident = pa.residence == DSR_MK_FRAMES_LDS ? 1 : 0;
  if (!for_value(MkCtAll{}, pa.ct, [&](auto ct) {
        launch(k_mk_minimize<ct()>, dim3(blocks), dim3(64), pa.ldsBytes, st, s.d_scr.p, s.d_gam.p, nframes, wa, stats, info, cost, grad, s.p, C, U, F, fbin, Tsel, first, R,
               eLim, resident, evalOnly ? 1 : 0); }))
    throw Error(DSR_E_ERROR, "MKSubbandBeamformer: no kernel k_mk_minimize<%d>", pa.ct);
}

}  // namespace dsr

using namespace dsr;
struct dsr_mk : MkState {};

extern "C" {

dsr_status dsr_mk_create(int fftLen, int chanN, int NC, int nSource, int halfBandShift, dsr_mk** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (halfBandShift) throw Error(DSR_E_ERROR, "not support halfBandShift==True yet");                  // mkBeamforming.py:41-43
    if (NC != 1) throw Error(DSR_E_ERROR, "not yet implemented in the case of NC > 2 (NC = %d)", NC);   // :38-40, :233-235
    if (nSource != 1) throw Error(DSR_E_PARAMETER, "one source only (nSource = %d)", nSource);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_DIMENSION, "bad fftLen=%d", fftLen);
    if (chanN < 2 || chanN > DSR_MK_MAX_CHAN) throw Error(DSR_E_DIMENSION, "MKSubbandBeamformer: 2 to %d channels (%d)", DSR_MK_MAX_CHAN, chanN);
    dsr_mk* s = new dsr_mk(); s->M = fftLen; s->C = chanN; *out = s;
  });
}
void dsr_mk_destroy(dsr_mk* s) { delete s; }

dsr_status dsr_mk_set_fixed_weights(dsr_mk* s, const double* wq, const double* B)
{
  return guard([&] {
    if (!s || !wq) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = s->C, F = s->M / 2 + 1, n = C - 1;
    s->wq.resize((size_t) F * C); s->B.resize((size_t) F * C * n);
    for (size_t i = 0; i < s->wq.size(); i++) s->wq[i] = zc(wq[2 * i], wq[2 * i + 1]);
    if (B) for (size_t i = 0; i < s->B.size(); i++) s->B[i] = zc(B[2 * i], B[2 * i + 1]);
    else for (int f = 0; f < F; f++) blocking_matrix_nc(&s->wq[(size_t) f * C], C, 1, &s->B[(size_t) f * C * n]);
    s->haveFixed = true; s->dirty = true;
  });
}
dsr_status dsr_mk_set_fixed_weights_from_bf(dsr_mk* s, const dsr_bf* bf)
{
  return guard([&] {
    if (!s || !bf) throw Error(DSR_E_PARAMETER, "null argument");
    int M = 0, C = 0, hbs = 0; const zc* wq = nullptr; const zc* B = nullptr;
    if (!bf_gsc_fixed_weights(bf, &M, &C, &hbs, &wq, &B)) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
    if (hbs) throw Error(DSR_E_ERROR, "not support halfBandShift==True yet");
    if (M != s->M || C != s->C) throw Error(DSR_E_DIMENSION, "the beamformer has fftLen %d and %d channels, this object %d and %d", M, C, s->M, s->C);
    const int F = M / 2 + 1, n = C - 1;
    s->wq.assign(wq, wq + (size_t) F * C); s->B.assign(B, B + (size_t) F * C * n);
    s->haveFixed = true; s->dirty = true;
  });
}
dsr_status dsr_mk_get_fixed_weights(const dsr_mk* s, double* wq, double* B)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveFixed) throw Error(DSR_E_ERROR, "call calcFixedWeights() or setFixedWeights() once");
    if (wq) for (size_t i = 0; i < s->wq.size(); i++) { wq[2 * i] = s->wq[i].real(); wq[2 * i + 1] = s->wq[i].imag(); }
    if (B) for (size_t i = 0; i < s->B.size(); i++) { B[2 * i] = s->B[i].real(); B[2 * i + 1] = s->B[i].imag(); }
  });
}
dsr_status dsr_mk_config(dsr_mk* s, int kind, double alpha, double beta, double gamma)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind != DSR_MK_PR && kind != DSR_MK_NRM) throw Error(DSR_E_PARAMETER, "bad kind %d", kind);
    s->p.kind = kind; s->p.alpha = alpha; s->p.beta = beta; s->gamma = gamma; s->dirty = true;
  });
}
dsr_status dsr_mk_minimizer(dsr_mk* s, int maxItns, double tolerance, double stopTolerance, double diffStopTolerance, double stepSize)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (maxItns < 0) throw Error(DSR_E_PARAMETER, "MAXITNS %d", maxItns);
    s->p.maxItns = maxItns; s->p.tol = tolerance; s->p.stopTol = stopTolerance; s->p.diffStop = diffStopTolerance; s->p.stepSize = stepSize;
  });
}
dsr_status dsr_mk_force_streamed(dsr_mk* s, int on)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->forceStreamed = on != 0; }); }

dsr_status dsr_mk_path(int chanN, int Tsel, int path[2], int64_t lds[2])
{
  return guard([&] {
    if (!path) throw Error(DSR_E_PARAMETER, "null argument");
    if (chanN < 2 || chanN > DSR_MK_MAX_CHAN) throw Error(DSR_E_DIMENSION, "MKSubbandBeamformer: 2 to %d channels (%d)", DSR_MK_MAX_CHAN, chanN);
    if (Tsel < 0) throw Error(DSR_E_DIMENSION, "Tsel %d", Tsel);
    const MkPath r = mk_path(chanN, Tsel, false);
    path[0] = r.ct; path[1] = r.residence;
    if (lds) { lds[0] = r.tcap; lds[1] = (int64_t) r.ldsBytes; }
  });
}

dsr_status dsr_mk_eval(dsr_mk* s, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                       const double* wa, const double* stats, double* cost, double* grad, void* stream)
{
  return guard([&] {
    if (!s || !X || !wa || !cost || !grad) throw Error(DSR_E_PARAMETER, "null argument");
    mk_run(*s, X, nframes, U, Tmax, sFrame, eFrame, R, fbinX, const_cast<double*>(wa), const_cast<double*>(stats), nullptr, cost, grad, true, (hipStream_t) stream);
  });
}
dsr_status dsr_mk_estimate(dsr_mk* s, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                           double* wa, double* stats, int32_t* info, double* cost, void* stream)
{
  return guard([&] {
    if (!s || !X || !wa || !info || !cost) throw Error(DSR_E_PARAMETER, "null argument");
    mk_run(*s, X, nframes, U, Tmax, sFrame, eFrame, R, fbinX, wa, stats, info, cost, nullptr, false, (hipStream_t) stream);
  });
}
dsr_status dsr_mk_apply(dsr_mk* s, const float* X, int U, int Tmax, const double* wa, float* Y, void* stream)
{
  return guard([&] {
    if (!s || !X || !wa || !Y) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveFixed) throw Error(DSR_E_ERROR, "call calcFixedWeights() or setFixedWeights() once");
    if (U <= 0 || Tmax <= 0) return;
    if (U > 65535) throw Error(DSR_E_DIMENSION, "at most 65535 utterances a call (%d)", U);
    require_device();
    mk_upload(*s);
    const int C = s->C, F = s->M / 2 + 1; const long perUtt = (long) Tmax * F, nw = (long) U * F * C;
    const size_t lds = sizeof(float2) * (size_t) F * C;
    if (lds > 160 * 1024) throw Error(DSR_E_DIMENSION, "beamformer weights need %zu bytes of LDS", lds);
    s->d_w.reserve((size_t) nw);
    launch(k_mk_weff, dim3((unsigned) cdiv(nw, 256)), dim3(256), 0, (hipStream_t) stream, s->d_wq.p, s->d_B.p, wa, s->d_w.p, U, C, F);
    int gx = cdiv(perUtt, 256 * 4); if (gx < 1) gx = 1; if (gx > 4096) gx = 4096;
    launch(k_mk_apply, dim3(gx, U), dim3(256), lds, (hipStream_t) stream, (const float2*) X, s->d_w.p, (float2*) Y, C, F, perUtt);
  });
}

}  // extern "C"
