// csrc/mk_minimize.h -- what the maximum-kurtosis (k_mk.hip) and the maximum-negentropy (k_mn.hip) beamformers share: the GSC's fixed weights
// on host and device, the prepare kernel (y0 = wq^H X, Z = B^H X), the minimisers (conjugate_pr with its line search; steepest descent) as one
// kernel template over an evaluator, the LDS-resident / streamed choice and the per-utterance apply.  The kernels that are no templates of the
// evaluator (prepare, apply) and the host pieces are defined once, in k_mk.hip.
//
// An evaluator Ev supplies
//   Ev::kNrm                      whether the steepest-descent (_nrm) minimiser and its epilogue exist for it
//   Ev::Args                      its kernel arguments (a trivially copyable struct)
//   void init(frames, wn, P, args, u, f, pix, UF)
//   template <int CT> double eval(xv, gout)      cost (returned) and, with gout, the packed gradient at the packed weights xv; LDS vectors
//   template <int CT> void finish_nrm(X, n2)     the _nrm epilogue (only read when kNrm)
// A starting cost that is not finite makes the problem DSR_MK_EXIT_SKIPPED.
//
// Reduction order (an interface: tests/mk_np.py restates it): 64 partial sums, partial p adds frames p, p + 64, ... in increasing order, then
// a butterfly over the wave (lane ^ 1, ^ 2, ... ^ 32) = a fixed binary tree; sums are divided by N after the reduction.  Built with
// -ffp-contract=off, so a run repeats bit for bit and the LDS-resident and the streamed path agree bit for bit.  |v| of a packed vector
// is the square root of the sequential sum of squares.
//
// One wave (64 lanes) owns a problem.  Every lane carries the same scalars (the butterfly leaves the same sum in every lane), so control flow
// is uniform; the minimiser's vectors (x, g, trial points, direction) live in LDS and are updated lane-parallel.
#pragma once
#include "launch.h"
#include "gsc_weights.h"
#include "beamformer.h"
#include <complex>
#include <cmath>
#include <vector>

namespace dsr {
typedef std::complex<double> zc;
static const int MK_FRAME_LDS = 128 * 1024;        // LDS a workgroup gives its frames (of the 160 KiB of a CU; the rest: minimiser vectors)
static const int MK_NVEC = 7;                      // x, g, x1, x2, p, g0, wn

struct MkParams { int kind, maxItns, evalCap; double alpha, beta, tol, stopTol, diffStop, stepSize; };

// the fixed part of a GSC and the device buffers of a call
struct MkFixed {
  int M = 0, C = 0; bool haveFixed = false, forceStreamed = false;
  std::vector<zc> wq, B;                           // [F][C], [F][C][C-1]
  DevBuf<double2> d_wq, d_B, d_scr; DevBuf<float2> d_w; bool dirty = true;
};

// frames accumObservations(sFrame, eFrame, R) keeps (:97-143): s = first + k R, first the smallest multiple of R >= sFrame, s < lim
__host__ __device__ static inline int mk_first(int sFrame, int R) { const int s = sFrame < 0 ? 0 : sFrame; return ((s + R - 1) / R) * R; }
__host__ __device__ static inline int mk_count(int first, int R, int lim) { return lim > first ? (lim - first + R - 1) / R : 0; }

using MkCt = ints<4, 6, 8>;                                          // the channel counts k_mk_* are instantiated for besides the run-time 0
using MkCtAll = ints<4, 6, 8, 0>;
struct MkPath { int ct, residence, tcap; size_t ldsBytes; };
struct MkCall { int first, R, eLim, Tsel; MkPath pa; };             // the frame selection and the dispatch of one call

// ---- defined in k_mk.hip
MkPath mk_path(int C, int Tsel, bool forceStreamed);
void mk_create_checks(const char* what, int fftLen, int chanN, int NC, int nSource, int halfBandShift);
void mk_fixed_set(MkFixed& s, const double* wq, const double* B);
void mk_fixed_from_bf(MkFixed& s, const dsr_bf* bf);
void mk_fixed_get(const MkFixed& s, double* wq, double* B);
void mk_fixed_upload(MkFixed& s);                                   // wq and B to the device, dirty cleared
// checks the batch, clamps R and sFrame as accumObservations does; false: nothing to do (U == 0)
bool mk_batch_checks(const MkFixed& s, int U, int Tmax, int fbin, int& R, int& sFrame);
// launches k_mk_prepare<CT> into s.d_scr (after mk_fixed_upload)
MkCall mk_prepare(MkFixed& s, const char* what, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, hipStream_t st);
void mk_apply(MkFixed& s, const float* X, int U, int Tmax, const double* wa, float* Y, hipStream_t st);

// ---- device pieces
struct MkFrames { const double2* scr; const double2* zs; int resident, T, Tn, C, n, lane; };

// (not wave_sum of dev_math.h: this butterfly runs from distance 1 up, the other from 32 down, and the two round differently)
__device__ __forceinline__ double mk_wsum(double v) { for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m); return v; }
__device__ __forceinline__ double2 mk_ld(const MkFrames& c, int t, int e) { return c.resident ? c.zs[(long) e * c.Tn + t] : c.scr[(long) t * c.C + e]; }

// lane-parallel vector pieces; every one starts with a barrier, so a value written by the piece before is seen and nobody still reads what is overwritten
__device__ __forceinline__ void mk_copy(double* d, const double* s, int n2, int lane) { __syncthreads(); for (int i = lane; i < n2; i += 64) d[i] = s[i]; }
// take_step: dx = a p, x1 = x + dx
__device__ __forceinline__ void mk_step(double* x1, const double* x, const double* p, double a, int n2, int lane)
{ __syncthreads(); for (int i = lane; i < n2; i += 64) { const double dx = a * p[i]; x1[i] = x[i] + dx; } }
__device__ __forceinline__ double mk_dot(const double* a, const double* b, int n2) { __syncthreads(); double r = 0.0; for (int i = 0; i < n2; i++) r += a[i] * b[i]; return r; }
__device__ __forceinline__ double mk_nrm(const double* a, int n2) { return sqrt(mk_dot(a, a, n2)); }

template <int CT, class Ev>
__global__ __launch_bounds__(64) void k_mk_minimize(const double2* __restrict__ scrAll, typename Ev::Args ea, const int* __restrict__ nframes,
                                                    double* __restrict__ wa, int* __restrict__ info, double* __restrict__ fout,
                                                    double* __restrict__ gradOut, MkParams P, int Crt, int U, int F, int fbin, int Tsel, int first, int R,
                                                    int eLim, int resident, int evalOnly)
{
  const int C = CT ? CT : Crt, n = C - 1, n2 = 2 * n, lane = threadIdx.x;
  const int u = fbin < 0 ? blockIdx.x / F : blockIdx.x, f = fbin < 0 ? blockIdx.x - u * F : fbin;
  const long pix = (long) u * F + f, UF = (long) U * F;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double* vec = reinterpret_cast<double*>(smem);
  double *X = vec, *G = vec + n2, *X1 = vec + 2 * n2, *X2 = vec + 3 * n2, *Pd = vec + 4 * n2, *G0 = vec + 5 * n2;
  double2* zs = reinterpret_cast<double2*>(smem + (((size_t) MK_NVEC * n2 * sizeof(double) + 15) & ~(size_t) 15));
  int lim = eLim; if (nframes) { const int nf = nframes[u]; if (nf < lim) lim = nf; }
  MkFrames fr;
  fr.T = mk_count(first, R, lim); fr.Tn = Tsel; fr.C = C; fr.n = n; fr.lane = lane; fr.resident = resident;
  fr.scr = scrAll + pix * Tsel * C; fr.zs = zs;
  Ev c;
  c.init(fr, vec + 6 * n2, P, ea, u, f, pix, UF);
  double* wap = wa + pix * n2;
  for (int i = lane; i < n2; i += 64) X[i] = wap[i];
  if (resident) for (int i = lane; i < fr.T * C; i += 64) { const int t = i / C, e = i - t * C; zs[(long) e * Tsel + t] = fr.scr[i]; }
  __syncthreads();

  if (evalOnly) {
    if (fr.T == 0) {                                                 // no frame: nothing to average
      if (lane == 0) { fout[pix] = nan(""); for (int i = 0; i < n2; i++) gradOut[pix * n2 + i] = nan(""); }
      return;
    }
    const double fv = c.template eval<CT>(X, G);
    if (lane == 0) fout[pix] = fv;
    for (int i = lane; i < n2; i += 64) gradOut[pix * n2 + i] = G[i];
    return;
  }

  int iters = 0, evals = 0, failed = 0, reason = DSR_MK_EXIT_MAX_ITERATIONS;
  double fcur = 0.0;
  bool skipped = fr.T == 0;
  if (!skipped) { fcur = c.template eval<CT>(X, G); evals = 1; skipped = !isfinite(fcur); }
  if (skipped) {
    if (lane == 0) { info[pix * 4] = 0; info[pix * 4 + 1] = evals; info[pix * 4 + 2] = 0; info[pix * 4 + 3] = DSR_MK_EXIT_SKIPPED; fout[pix] = fr.T == 0 ? nan("") : fcur; }
    return;
  }
  double preMi = 10000.0;

  if (!Ev::kNrm || P.kind == DSR_MK_PR) {
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
      double fc = c.template eval<CT>(X1, nullptr); evals++; itEvals++;
      // intermediate_point: a point b between a and c with f(b) < f(a), from the parabola through f(a), f'(a), f(c)
      double stepb = 0.0, fb = 0.0; bool capped = false;
      { double ic = stepc, ifc = fc;
        for (;;) {
          const double uu = fabs(pg * lam * ic);
          stepb = 0.5 * ic * uu / ((ifc - fa) + uu);
          if (itEvals >= P.evalCap) { capped = true; break; }
          mk_step(X1, X, Pd, -stepb * lam, n2, lane);
          fb = c.template eval<CT>(X1, nullptr); evals++; itEvals++;
          if (fb >= fa && stepb > 0.0) { ifc = fb; ic = stepb; failed++; continue; }
          break;
        } }
      if (capped) { reason = DSR_MK_EXIT_EVAL_CAP; break; }
      (void) c.template eval<CT>(X1, G); evals++; itEvals++;
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
        const double fm = c.template eval<CT>(X1, nullptr); evals++; itEvals++;
        if (fm > fb) {
          if (fm < fv) { wS = vS; vS = stepm; fw = fv; fv = fm; }
          else if (fm < fw) { wS = stepm; fw = fm; }
          if (stepm < stepb) { stepa = stepm; fa = fm; } else { stepc = stepm; fc = fm; }
        } else if (fm <= fb) {
          old2 = old1; old1 = fabs(uS - stepm);
          wS = vS; vS = uS; uS = stepm; fw = fv; fv = fu; fu = fm;
          mk_copy(X2, X1, n2, lane);
          (void) c.template eval<CT>(X1, G); evals++; itEvals++;
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
  } else if constexpr (Ev::kNrm) {
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
        f1 = c.template eval<CT>(X1, G0); evals++; itEvals++;       // G0 holds the trial's gradient
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
    c.template finish_nrm<CT>(X, n2);
  }
  __syncthreads();
  for (int i = lane; i < n2; i += 64) wap[i] = X[i];
  if (lane == 0) { info[pix * 4] = iters; info[pix * 4 + 1] = evals; info[pix * 4 + 2] = failed; info[pix * 4 + 3] = reason; fout[pix] = fcur; }
}

// dispatch, in one place: the instantiation of k_mk_minimize<CT, Ev> that mk_path names, through launch()
template <class Ev>
void mk_minimize_launch(const char* what, MkFixed& s, const MkCall& c, typename Ev::Args ea, const int32_t* nframes, double* wa, int32_t* info, double* cost,
                        double* grad, const MkParams& P, int U, int fbin, bool evalOnly, hipStream_t st)
{
  const int C = s.C, F = s.M / 2 + 1;
  const unsigned blocks = fbin < 0 ? (unsigned) ((long) U * F) : (unsigned) U;
  const int resident = c.pa.residence == DSR_MK_FRAMES_LDS ? 1 : 0;
  if (!for_value(MkCtAll{}, c.pa.ct, [&](auto ct) {
        launch(k_mk_minimize<ct(), Ev>, dim3(blocks), dim3(64), c.pa.ldsBytes, st, s.d_scr.p, ea, nframes, wa, info, cost, grad, P, C, U, F, fbin, c.Tsel, c.first, c.R,
               c.eLim, resident, evalOnly ? 1 : 0); }))
    throw Error(DSR_E_ERROR, "%s: no kernel k_mk_minimize<%d>", what, c.pa.ct);
}

}  // namespace dsr
