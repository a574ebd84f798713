// csrc/mn_kernels.hip -- maximum negentropy beamforming under a generalised Gaussian (GG) speech model (btk/lib/mnBeamforming.py:
// MNSubbandBeamformerGGDc_pr / _nrm) and the accumulation of the GG model's training statistics (btk/lib/GGDcEst.py: MLE4CGGaussianD.acc).
//
// The beamformer is the negentropy evaluator of k_mk_minimize (mk_minimize.h): fixed weights, prepare kernel, conjugate_pr with its line search,
// frame residence and apply are the maximum-kurtosis beamformer's.  With the per-bin shape f, Bc = Gamma(1/f) / Gamma(2/f) and NgConst (ggd.h):
//   Y_t = y0_t - sum_j conj(wa_j) Z_t,j      y2_t = |Y_t|^2      p_t = det_pow(y2_t, f)
//   sigma2 = (sum y2_t) / T                  Sf = (sum p_t) / T
//   cost = -[ (det_log(sigma2) + (1 + log pi)) - beta ((NgConst + det_log(f Sf) / f) - log Bc) ] + alpha |wa|^2       (:446-485, 331-370)
//   dJ_j = [ (-(sum' q_t,j)) / sigma2 + (beta sum' (p_t / y2_t) q_t,j) / Sf ] / T'        q_t,j = Z_t,j conj(Y_t)       (:487-513)
//   grad_j = -dJ_j + alpha wa_j               (packed re/im: the derivative w.r.t. conj(wa) = half the real gradient, as in k_mk.hip)
// sum' and T' run over the frames with y2_t > 0 (:506-513: the divisor is the count of the frames that are not zero).  normalizeWeight is the
// identity in both reference classes (its clipping is commented out, :515-528, :693-706), so _pr and _nrm differ in the default beta only (0.5
// and 1.0), both run conjugate_pr, and gamma is accepted without effect.  A cost whose sum of y2 is zero is NaN, which makes the problem
// DSR_MK_EXIT_SKIPPED at the start.  log, exp and pow are det_math.h's, so tests/mn_np.py restates an evaluation bit for bit.
// One pass over the frames per evaluation; a cost-only evaluation does one det_log and one det_exp a frame.
#include "mk_minimize.h"
#include "ggd.h"

namespace dsr {

struct MnState : MkFixed {
  MkParams p;
  double gamma = -1.0;
  bool haveGgd = false;
  std::vector<double> shape, cst;                                    // [F]; [F][3]: shape, NgConst, log Bc
  std::vector<double> Bc;
  DevBuf<double> d_cst;
  MnState() { p.kind = DSR_MK_PR; p.maxItns = 40; p.evalCap = DSR_MK_EVAL_CAP; p.alpha = 1.0e-2; p.beta = 0.5; p.tol = 1.0e-3; p.stopTol = 1.0e-2; p.diffStop = 1.0e-5; p.stepSize = 0.2; }
};

struct MnNeg {
  static constexpr bool kNrm = false;
  struct Args { const double* cst; };                                // [F][3]: shape, NgConst, log Bc
  MkFrames fr;
  double alpha, beta, shape, ngConst, logBc;

  __device__ void init(const MkFrames& frames, double*, const MkParams& P, const Args& a, int, int f, long, long)
  { fr = frames; alpha = P.alpha; beta = P.beta; shape = a.cst[3 * f]; ngConst = a.cst[3 * f + 1]; logBc = a.cst[3 * f + 2]; }

  template <int CT>
  __device__ double eval(const double* xv, double* gout)
  {
    const int n = fr.n, lane = fr.lane;
    __syncthreads();
    double s2 = 0.0;
    for (int k = 0; k < n; k++) s2 += xv[2 * k] * xv[2 * k] + xv[2 * k + 1] * xv[2 * k + 1];
    const double rterm = alpha * s2;
    constexpr int JB = CT ? CT - 1 : 8;                              // gradient entries accumulated per pass over the frames
    const double Tn = (double) fr.T;
    double S2 = 0.0, Sp = 0.0, Tp = 0.0, sig2 = 0.0, Sf = 0.0;
    for (int j0 = 0; j0 < n; j0 += JB) {
      double a1r[JB], a1i[JB], apr[JB], api[JB];
      for (int jj = 0; jj < JB; jj++) { a1r[jj] = 0.0; a1i[jj] = 0.0; apr[jj] = 0.0; api[jj] = 0.0; }
      for (int t = lane; t < fr.T; t += 64) {
        const double2 y0 = mk_ld(fr, t, 0);
        double sr = 0.0, si = 0.0;
        for (int j = 0; j < n; j++) { const double2 z = mk_ld(fr, t, 1 + j); const double wr = xv[2 * j], wi = xv[2 * j + 1]; sr += wr * z.x + wi * z.y; si += wr * z.y - wi * z.x; }
        const double Yr = y0.x - sr, Yi = y0.y - si, y2 = Yr * Yr + Yi * Yi;
        const double pt = det_pow(y2, shape);
        if (j0 == 0) { S2 += y2; Sp += pt; if (y2 > 0.0) Tp += 1.0; }
        if (gout && y2 > 0.0) {
          const double ratio = pt / y2;
          for (int jj = 0; jj < JB; jj++) {
            const int j = j0 + jj;
            if (j < n) {
              const double2 z = mk_ld(fr, t, 1 + j);
              const double qr = z.x * Yr + z.y * Yi, qi = z.y * Yr - z.x * Yi;      // Z conj(Y)
              a1r[jj] += qr; a1i[jj] += qi; apr[jj] += ratio * qr; api[jj] += ratio * qi;
            }
          }
        }
      }
      if (j0 == 0) { S2 = mk_wsum(S2); Sp = mk_wsum(Sp); Tp = mk_wsum(Tp); sig2 = S2 / Tn; Sf = Sp / Tn; }
      if (!gout) break;
      for (int jj = 0; jj < JB; jj++) {
        const int j = j0 + jj;
        if (j < n) {
          const double A1r = mk_wsum(a1r[jj]), A1i = mk_wsum(a1i[jj]), Apr = mk_wsum(apr[jj]), Api = mk_wsum(api[jj]);
          const double dJr = ((-A1r) / sig2 + (beta * Apr) / Sf) / Tp, dJi = ((-A1i) / sig2 + (beta * Api) / Sf) / Tp;
          if (lane == 0) {
            if (S2 > 0.0) { gout[2 * j] = (-dJr) + alpha * xv[2 * j]; gout[2 * j + 1] = (-dJi) + alpha * xv[2 * j + 1]; }
            else { gout[2 * j] = nan(""); gout[2 * j + 1] = nan(""); }
          }
        }
      }
    }
    double cost = nan("");
    if (S2 > 0.0) {
      const double hg = det_log(sig2) + (1.0 + 1.1447298858494002);                 // H_gaussian (:202-204)
      const double hgg = (ngConst + det_log(shape * Sf) / shape) - logBc;           // entropy(ScalingPar): NgConst + log(ScalingPar)
      cost = (0.0 - (hg - beta * hgg)) + rterm;
    }
    __syncthreads();
    return cost;
  }

  template <int CT> __device__ void finish_nrm(double*, int) {}
};

static void mn_upload(MnState& s)
{
  if (!s.dirty) return;
  s.d_cst.upload(s.cst); mk_fixed_upload(s);
}

static void mn_run(MnState& s, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, int fbin, double* wa,
                   int32_t* info, double* cost, double* grad, bool evalOnly, hipStream_t st)
{
  if (!s.haveGgd) throw Error(DSR_E_ERROR, "MNSubbandBeamformer: set the GG model (dsr_mn_set_ggd) once");
  if (!mk_batch_checks(s, U, Tmax, fbin, R, sFrame)) return;
  require_device();
  mn_upload(s);
  const MkCall c = mk_prepare(s, "MNSubbandBeamformer", X, nframes, U, Tmax, sFrame, eFrame, R, st);
  mk_minimize_launch<MnNeg>("MNSubbandBeamformer", s, c, MnNeg::Args{s.d_cst.p}, nframes, wa, info, cost, grad, s.p, U, fbin, evalOnly, st);
}

// ---- GG model training statistics.  X [U][Tmax][F] complex64; lanes run over bins, so a row of F is read coalesced.  Per (utterance, bin): 64
// partial sums (partial q adds frames q, q + 64, ... in increasing order) and a fixed binary tree over them: a thread row holds partials
// 4 row .. 4 row + 3 and adds them as (a0 + a1) + (a2 + a3), the 16 rows are combined pairwise through LDS.  k_ggd_total then adds acc_in and
// the utterances in increasing order.  Nothing depends on the grid: a call repeats bit for bit.
static const int GGD_ROWS = 16;

__global__ __launch_bounds__(64 * GGD_ROWS) void k_ggd_partial(const float2* __restrict__ X, const int* __restrict__ nframes, const double* __restrict__ par,
                                                               double* __restrict__ uacc, int Tmax, int F)
{
  __shared__ double sh[GGD_ROWS][4][64];
  const int tx = threadIdx.x, ty = threadIdx.y, f = blockIdx.x * 64 + tx, u = blockIdx.y;
  int nf = Tmax; if (nframes) { const int v = nframes[u]; if (v < nf) nf = v; }
  double a[4][4];
  for (int i = 0; i < 4; i++) for (int k = 0; k < 4; k++) a[i][k] = 0.0;
  if (f < F) {
    const double p = par[4 * f], sa = par[4 * f + 1], Bc = par[4 * f + 2], LlConst = par[4 * f + 3];
    const double la0 = det_log(Bc * sa), ll0 = LlConst - det_log(sa);
    const float2* Xu = X + (long) u * Tmax * F + f;
    for (int t0 = 4 * ty; t0 < nf; t0 += 64)
      for (int i = 0; i < 4; i++) {
        const int t = t0 + i;
        if (t < nf) {
          const float2 v = Xu[(long) t * F];
          const double re = (double) v.x, im = (double) v.y, v2 = re * re + im * im;
          double tmp = 0.0;
          if (v2 > 0.0) {
            const double l = det_log(v2), la = l - la0;
            a[i][0] += det_exp(p * l);                               // accSigma (:218-220)
            tmp = det_exp(p * la);                                   // accP (:222-228)
            if (v2 > 1.0e-22) a[i][1] += tmp * la;                   // |X| > 10e-12
            a[i][2] += tmp;
          }
          a[i][3] += ll0 - tmp;                                      // prob (:90-104)
        }
      }
  }
  for (int k = 0; k < 4; k++) sh[ty][k][tx] = (a[0][k] + a[1][k]) + (a[2][k] + a[3][k]);
  __syncthreads();
  for (int m = 1; m < GGD_ROWS; m <<= 1) {
    if (ty % (2 * m) == 0) for (int k = 0; k < 4; k++) sh[ty][k][tx] += sh[ty + m][k][tx];
    __syncthreads();
  }
  if (ty == 0 && f < F) for (int k = 0; k < 4; k++) uacc[((long) u * 4 + k) * F + f] = sh[0][k][tx];
}

// acc [5][F] = acc_in + the utterances in increasing order; rows: acc1S, acc1P, acc2P, nSample, totalL
__global__ void k_ggd_total(const double* __restrict__ uacc, const int* __restrict__ nframes, const double* __restrict__ accIn, double* __restrict__ acc,
                            int U, int Tmax, int F)
{
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 5 * F) return;
  const int row = i / F, f = i - row * F;
  double r = accIn ? accIn[i] : 0.0;
  for (int u = 0; u < U; u++) {
    if (row == 3) { int nf = Tmax; if (nframes) { const int v = nframes[u]; if (v < nf) nf = v; } r += (double) (nf > 0 ? nf : 0); }
    else r += uacc[((long) u * 4 + (row < 3 ? row : 3)) * F + f];
  }
  acc[i] = r;
}

}  // namespace dsr

using namespace dsr;
struct dsr_mn : MnState {};

extern "C" {

dsr_status dsr_mn_create(int fftLen, int chanN, int NC, int nSource, int halfBandShift, dsr_mn** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    mk_create_checks("MNSubbandBeamformer", fftLen, chanN, NC, nSource, halfBandShift);
    dsr_mn* s = new dsr_mn(); s->M = fftLen; s->C = chanN; *out = s;
  });
}
void dsr_mn_destroy(dsr_mn* s) { delete s; }

dsr_status dsr_mn_set_fixed_weights(dsr_mn* s, const double* wq, const double* B)
{ return guard([&] { if (!s || !wq) throw Error(DSR_E_PARAMETER, "null argument"); mk_fixed_set(*s, wq, B); }); }
dsr_status dsr_mn_set_fixed_weights_from_bf(dsr_mn* s, const dsr_bf* bf)
{ return guard([&] { if (!s || !bf) throw Error(DSR_E_PARAMETER, "null argument"); mk_fixed_from_bf(*s, bf); }); }
dsr_status dsr_mn_get_fixed_weights(const dsr_mn* s, double* wq, double* B)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); mk_fixed_get(*s, wq, B); }); }

dsr_status dsr_mn_set_ggd(dsr_mn* s, const double* shape)
{
  return guard([&] {
    if (!s || !shape) throw Error(DSR_E_PARAMETER, "null argument");
    const int F = s->M / 2 + 1;
    for (int f = 0; f < F; f++)
      if (!(shape[f] > 0.0) || !std::isfinite(shape[f])) throw Error(DSR_E_PARAMETER, "the shape parameter of bin %d is %g", f, shape[f]);
    s->shape.assign(shape, shape + F); s->cst.resize((size_t) 3 * F); s->Bc.resize(F);
    for (int f = 0; f < F; f++) {
      const GgdConst c = ggd_constants(shape[f]);
      s->cst[3 * f] = shape[f]; s->cst[3 * f + 1] = c.NgConst; s->cst[3 * f + 2] = c.logBc; s->Bc[f] = c.Bc;
    }
    s->haveGgd = true; s->dirty = true;
  });
}
dsr_status dsr_mn_get_constants(const dsr_mn* s, double* Bc, double* NgConst, double* logBc)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveGgd) throw Error(DSR_E_ERROR, "MNSubbandBeamformer: set the GG model (dsr_mn_set_ggd) once");
    const int F = s->M / 2 + 1;
    for (int f = 0; f < F; f++) { if (Bc) Bc[f] = s->Bc[f]; if (NgConst) NgConst[f] = s->cst[3 * f + 1]; if (logBc) logBc[f] = s->cst[3 * f + 2]; }
  });
}
dsr_status dsr_mn_config(dsr_mn* s, double alpha, double beta, double gamma)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    s->p.alpha = alpha; s->p.beta = beta; s->gamma = gamma;
  });
}
dsr_status dsr_mn_minimizer(dsr_mn* s, int maxItns, double tolerance, double stopTolerance, double diffStopTolerance, double stepSize)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (maxItns < 0) throw Error(DSR_E_PARAMETER, "MAXITNS %d", maxItns);
    s->p.maxItns = maxItns; s->p.tol = tolerance; s->p.stopTol = stopTolerance; s->p.diffStop = diffStopTolerance; s->p.stepSize = stepSize;
  });
}
dsr_status dsr_mn_force_streamed(dsr_mn* s, int on)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->forceStreamed = on != 0; }); }

dsr_status dsr_mn_eval(dsr_mn* s, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                       const double* wa, double* cost, double* grad, void* stream)
{
  return guard([&] {
    if (!s || !X || !wa || !cost || !grad) throw Error(DSR_E_PARAMETER, "null argument");
    mn_run(*s, X, nframes, U, Tmax, sFrame, eFrame, R, fbinX, const_cast<double*>(wa), nullptr, cost, grad, true, (hipStream_t) stream);
  });
}
dsr_status dsr_mn_estimate(dsr_mn* s, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, int fbinX,
                           double* wa, int32_t* info, double* cost, void* stream)
{
  return guard([&] {
    if (!s || !X || !wa || !info || !cost) throw Error(DSR_E_PARAMETER, "null argument");
    mn_run(*s, X, nframes, U, Tmax, sFrame, eFrame, R, fbinX, wa, info, cost, nullptr, false, (hipStream_t) stream);
  });
}
dsr_status dsr_mn_apply(dsr_mn* s, const float* X, int U, int Tmax, const double* wa, float* Y, void* stream)
{
  return guard([&] {
    if (!s || !X || !wa || !Y) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->haveFixed) throw Error(DSR_E_ERROR, "call calcFixedWeights() or setFixedWeights() once");
    if (U <= 0 || Tmax <= 0) return;
    if (U > 65535) throw Error(DSR_E_DIMENSION, "at most 65535 utterances a call (%d)", U);
    require_device();
    if (s->dirty) { if (s->haveGgd) s->d_cst.upload(s->cst); mk_fixed_upload(*s); }
    mk_apply(*s, X, U, Tmax, wa, Y, (hipStream_t) stream);
  });
}

dsr_status dsr_ggd_accumulate(const float* X, const int32_t* nframes, int U, int Tmax, int F, const double* p, const double* sa, const double* accIn,
                              double* acc, void* stream)
{
  return guard([&] {
    if (!X || !p || !sa || !acc) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0 || F < 1) throw Error(DSR_E_DIMENSION, "bad batch U=%d Tmax=%d F=%d", U, Tmax, F);
    if (U > 65535) throw Error(DSR_E_DIMENSION, "at most 65535 utterances a call (%d)", U);
    std::vector<double> par((size_t) 4 * F);
    for (int f = 0; f < F; f++) {
      if (!(p[f] > 0.0) || !std::isfinite(p[f])) throw Error(DSR_E_PARAMETER, "the shape parameter of bin %d is %g", f, p[f]);
      if (!(sa[f] > 0.0) || !std::isfinite(sa[f])) throw Error(DSR_E_PARAMETER, "the scaling parameter of bin %d is %g", f, sa[f]);
      const GgdConst c = ggd_constants(p[f]);
      par[4 * f] = p[f]; par[4 * f + 1] = sa[f]; par[4 * f + 2] = c.Bc; par[4 * f + 3] = c.LlConst;
    }
    if (U == 0 || Tmax == 0) {                                       // no sample: acc_in alone (nframes is not read)
      for (int i = 0; i < 5 * F; i++) acc[i] = accIn ? accIn[i] : 0.0;
      return;
    }
    require_device();
    hipStream_t st = (hipStream_t) stream;
    DevBuf<double> d_par, d_uacc, d_in, d_out;
    d_par.upload(par, st); d_uacc.reserve((size_t) U * 4 * F); d_out.reserve((size_t) 5 * F);
    if (accIn) d_in.upload(accIn, (size_t) 5 * F, st);
    launch(k_ggd_partial, dim3((unsigned) cdiv(F, 64), (unsigned) U), dim3(64, GGD_ROWS), 0, st, (const float2*) X, nframes, d_par.p, d_uacc.p, Tmax, F);
    launch(k_ggd_total, dim3((unsigned) cdiv(5L * F, 256)), dim3(256), 0, st, d_uacc.p, nframes, accIn ? d_in.p : nullptr, d_out.p, U, Tmax, F);
    DSR_HIP(hipMemcpyAsync(acc, d_out.p, sizeof(double) * 5 * F, hipMemcpyDeviceToHost, st));
    DSR_HIP(hipStreamSynchronize(st));
  });
}

}  // extern "C"
