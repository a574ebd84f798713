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
// The minimisers, their reduction order and every piece the maximum-negentropy beamformer (mn_kernels.hip) uses as well are in mk_minimize.h; this
// unit has the kurtosis evaluator, the prepare and apply kernels, and the host pieces that header declares.
#include "mk_minimize.h"

namespace dsr {

struct MkState : MkFixed {
  MkParams p;
  double gamma = -1.0;
  DevBuf<double> d_gam;
  MkState() { p.kind = DSR_MK_PR; p.maxItns = 40; p.evalCap = DSR_MK_EVAL_CAP; p.alpha = 1.0e-2; p.beta = 3.0; p.tol = 1.0e-3; p.stopTol = 1.0e-2; p.diffStop = 1.0e-5; p.stepSize = 0.01; }
};

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

// ---- 2. the kurtosis evaluator of k_mk_minimize (mk_minimize.h)
struct MkKurt {
  static constexpr bool kNrm = true;
  struct Args { const double* gam; double* stats; };                // |gamma| per bin; the carried statistics [3][U][F] (optional)
  MkFrames fr; double* wn; double* stats; long pix, UF;
  int kind;
  double alpha, beta, ag, prevY2, prevY4, prevN, N;
  double S2, S4;                                                     // sums of |Y|^2, |Y|^4 of the last evaluation

  __device__ void init(const MkFrames& frames, double* wnv, const MkParams& P, const Args& a, int u, int f, long pix_, long UF_)
  {
    fr = frames; wn = wnv; stats = a.stats; pix = pix_; UF = UF_; kind = P.kind;
    alpha = P.alpha; beta = P.beta; ag = fabs(a.gam[f]);
    prevY2 = stats ? stats[pix] : 0.0; prevY4 = stats ? stats[UF + pix] : 0.0; prevN = stats ? stats[2 * UF + pix] : 0.0;
    N = prevN + (double) fr.T; S2 = 0.0; S4 = 0.0;
  }

  // cost (returned) and, with gout, the packed gradient at the packed weights xv; xv, gout and wn are LDS vectors of 2n doubles
  template <int CT>
  __device__ double eval(const double* xv, double* gout)
  {
    MkKurt& c = *this;
    const int n = c.fr.n, n2 = 2 * n, lane = c.fr.lane;
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
      for (int t = lane; t < c.fr.T; t += 64) {
        const double2 y0 = mk_ld(c.fr, t, 0);
        double sr = 0.0, si = 0.0;
        for (int j = 0; j < n; j++) { const double2 z = mk_ld(c.fr, t, 1 + j); const double wr = wn[2 * j], wi = wn[2 * j + 1]; sr += wr * z.x + wi * z.y; si += wr * z.y - wi * z.x; }
        const double Yr = y0.x - sr, Yi = y0.y - si, y2 = Yr * Yr + Yi * Yi;
        if (j0 == 0) { S2 += y2; S4 += y2 * y2; }
        if (gout)
          for (int jj = 0; jj < JB; jj++) {
            const int j = j0 + jj;
            if (j < n) {
              const double2 z = mk_ld(c.fr, t, 1 + j);
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

  // :646-654: the weights are normalised, storeStatistics (:410-420) with N already advanced
  template <int CT>
  __device__ void finish_nrm(double* X, int n2)
  {
    MkKurt& c = *this;
    const int n = c.fr.n, lane = c.fr.lane;
    __syncthreads();
    double s = 0.0; for (int k = 0; k < n; k++) s += X[2 * k] * X[2 * k] + X[2 * k + 1] * X[2 * k + 1];
    const double nr = sqrt(s);
    __syncthreads();
    if (nr > c.ag) for (int i = lane; i < n2; i += 64) X[i] = (c.ag * X[i]) / nr;
    if (stats) {
      (void) eval<CT>(X, nullptr);                                   // not counted: the reference's storeStatistics pass
      if (lane == 0) { stats[pix] = c.prevY2 + c.S2 / c.N; stats[UF + pix] = c.prevY4 + c.S4 / c.N; stats[2 * UF + pix] = c.N; }
    }
  }
};

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

// ---- the host pieces mk_minimize.h declares
MkPath mk_path(int C, int Tsel, bool forceStreamed)
{
  MkPath r; r.ct = has_value(MkCt{}, C) ? C : 0;
  r.tcap = MK_FRAME_LDS / (16 * C);
  r.residence = (Tsel <= r.tcap && !forceStreamed) ? DSR_MK_FRAMES_LDS : DSR_MK_FRAMES_STREAMED;
  const size_t vb = ((size_t) MK_NVEC * 2 * (C - 1) * sizeof(double) + 15) & ~(size_t) 15;
  r.ldsBytes = vb + (r.residence == DSR_MK_FRAMES_LDS ? (size_t) (Tsel > 0 ? Tsel : 0) * C * 16 : 0);
  return r;
}

void mk_create_checks(const char* what, int fftLen, int chanN, int NC, int nSource, int halfBandShift)
{
  if (halfBandShift) throw Error(DSR_E_ERROR, "not support halfBandShift==True yet");                  // mkBeamforming.py:41-43
  if (NC != 1) throw Error(DSR_E_ERROR, "not yet implemented in the case of NC > 2 (NC = %d)", NC);   // :38-40, :233-235
  if (nSource != 1) throw Error(DSR_E_PARAMETER, "one source only (nSource = %d)", nSource);
  if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_DIMENSION, "bad fftLen=%d", fftLen);
  if (chanN < 2 || chanN > DSR_MK_MAX_CHAN) throw Error(DSR_E_DIMENSION, "%s: 2 to %d channels (%d)", what, DSR_MK_MAX_CHAN, chanN);
}

void mk_fixed_set(MkFixed& s, const double* wq, const double* B)
{
  const int C = s.C, F = s.M / 2 + 1, n = C - 1;
  s.wq.resize((size_t) F * C); s.B.resize((size_t) F * C * n);
  for (size_t i = 0; i < s.wq.size(); i++) s.wq[i] = zc(wq[2 * i], wq[2 * i + 1]);
  if (B) for (size_t i = 0; i < s.B.size(); i++) s.B[i] = zc(B[2 * i], B[2 * i + 1]);
  else for (int f = 0; f < F; f++) blocking_matrix_nc(&s.wq[(size_t) f * C], C, 1, &s.B[(size_t) f * C * n]);
  s.haveFixed = true; s.dirty = true;
}

void mk_fixed_from_bf(MkFixed& s, const dsr_bf* bf)
{
  int M = 0, C = 0, hbs = 0; const zc* wq = nullptr; const zc* B = nullptr;
  if (!bf_gsc_fixed_weights(bf, &M, &C, &hbs, &wq, &B)) throw Error(DSR_E_ERROR, "call calcGSCWeightsX() once");
  if (hbs) throw Error(DSR_E_ERROR, "not support halfBandShift==True yet");
  if (M != s.M || C != s.C) throw Error(DSR_E_DIMENSION, "the beamformer has fftLen %d and %d channels, this object %d and %d", M, C, s.M, s.C);
  const int F = M / 2 + 1, n = C - 1;
  s.wq.assign(wq, wq + (size_t) F * C); s.B.assign(B, B + (size_t) F * C * n);
  s.haveFixed = true; s.dirty = true;
}

void mk_fixed_get(const MkFixed& s, double* wq, double* B)
{
  if (!s.haveFixed) throw Error(DSR_E_ERROR, "call calcFixedWeights() or setFixedWeights() once");
  if (wq) for (size_t i = 0; i < s.wq.size(); i++) { wq[2 * i] = s.wq[i].real(); wq[2 * i + 1] = s.wq[i].imag(); }
  if (B) for (size_t i = 0; i < s.B.size(); i++) { B[2 * i] = s.B[i].real(); B[2 * i + 1] = s.B[i].imag(); }
}

void mk_fixed_upload(MkFixed& s)
{
  std::vector<double2> a(s.wq.size()), b(s.B.size());
  for (size_t i = 0; i < a.size(); i++) a[i] = make_double2(s.wq[i].real(), s.wq[i].imag());
  for (size_t i = 0; i < b.size(); i++) b[i] = make_double2(s.B[i].real(), s.B[i].imag());
  s.d_wq.upload(a); s.d_B.upload(b); s.dirty = false;
}

bool mk_batch_checks(const MkFixed& s, int U, int Tmax, int fbin, int& R, int& sFrame)
{
  if (!s.haveFixed) throw Error(DSR_E_ERROR, "call calcFixedWeights() or setFixedWeights() once");
  const int F = s.M / 2 + 1;
  if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "bad batch U=%d Tmax=%d", U, Tmax);
  if (fbin >= F) throw Error(DSR_E_INDEX, "frequency bin %d > fftLen/2 %d", fbin, F - 1);
  if (U > 65535) throw Error(DSR_E_DIMENSION, "at most 65535 utterances a call (%d)", U);
  if (R < 1) R = 1;                                                  // :106-107
  if (R > Tmax) R = Tmax > 0 ? Tmax : 1;                             // the same frames (only s = 0 is a multiple), no overflow in mk_first
  if (sFrame > Tmax) sFrame = Tmax;
  return U != 0;
}

MkCall mk_prepare(MkFixed& s, const char* what, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, hipStream_t st)
{
  const int C = s.C, F = s.M / 2 + 1;
  MkCall c; c.R = R;
  c.first = mk_first(sFrame, R); c.eLim = eFrame < Tmax ? eFrame : Tmax; c.Tsel = mk_count(c.first, R, c.eLim);
  c.pa = mk_path(C, c.Tsel, s.forceStreamed);
  const int Tsel = c.Tsel;
  s.d_scr.reserve((size_t) U * F * (Tsel > 0 ? Tsel : 1) * C);
  if (Tsel > 0) {
    int TK = 32768 / (64 * C * 16); if (TK < 1) TK = 1; if (TK > 8) TK = 8;
    const size_t lds = (size_t) 64 * (TK * C + 1) * 16;
    const dim3 grid((unsigned) cdiv(F, 64), (unsigned) cdiv(Tsel, TK), (unsigned) U);
    if (grid.y > 65535) throw Error(DSR_E_DIMENSION, "too many frames (%d)", Tsel);
    if (!for_value(MkCtAll{}, c.pa.ct, [&](auto ct) {
          launch(k_mk_prepare<ct()>, grid, dim3(64), lds, st, (const float2*) X, s.d_wq.p, s.d_B.p, nframes, s.d_scr.p, C, Tmax, F, Tsel, c.first, R, c.eLim, TK); }))
      throw Error(DSR_E_ERROR, "%s: no kernel k_mk_prepare<%d>", what, c.pa.ct);
  }
  return c;
}

void mk_apply(MkFixed& s, const float* X, int U, int Tmax, const double* wa, float* Y, hipStream_t st)
{
  const int C = s.C, F = s.M / 2 + 1; const long perUtt = (long) Tmax * F, nw = (long) U * F * C;
  const size_t lds = sizeof(float2) * (size_t) F * C;
  if (lds > 160 * 1024) throw Error(DSR_E_DIMENSION, "beamformer weights need %zu bytes of LDS", lds);
  s.d_w.reserve((size_t) nw);
  launch(k_mk_weff, dim3((unsigned) cdiv(nw, 256)), dim3(256), 0, st, s.d_wq.p, s.d_B.p, wa, s.d_w.p, U, C, F);
  int gx = cdiv(perUtt, 256 * 4); if (gx < 1) gx = 1; if (gx > 4096) gx = 4096;
  launch(k_mk_apply, dim3(gx, U), dim3(256), lds, st, (const float2*) X, s.d_w.p, (float2*) Y, C, F, perUtt);
}

static void mk_upload(MkState& s)
{
  if (!s.dirty) return;
  const int C = s.C, F = s.M / 2 + 1;
  std::vector<double> g(F);
  for (int f = 0; f < F; f++) {                                      // gamma < 0: |wq| (:552-555)
    double q = 0.0; for (int c = 0; c < C; c++) q += gsc::abs2(s.wq[(size_t) f * C + c]);
    g[f] = s.gamma < 0 ? std::sqrt(q) : s.gamma;
  }
  s.d_gam.upload(g); mk_fixed_upload(s);
}

static void mk_run(MkState& s, const float* X, const int32_t* nframes, int U, int Tmax, int sFrame, int eFrame, int R, int fbin, double* wa, double* stats,
                   int32_t* info, double* cost, double* grad, bool evalOnly, hipStream_t st)
{
  if (!mk_batch_checks(s, U, Tmax, fbin, R, sFrame)) return;
  require_device();
  mk_upload(s);
  const MkCall c = mk_prepare(s, "MKSubbandBeamformer", X, nframes, U, Tmax, sFrame, eFrame, R, st);
  mk_minimize_launch<MkKurt>("MKSubbandBeamformer", s, c, MkKurt::Args{s.d_gam.p, stats}, nframes, wa, info, cost, grad, s.p, U, fbin, evalOnly, st);
}

}  // namespace dsr

using namespace dsr;
struct dsr_mk : MkState {};

extern "C" {

dsr_status dsr_mk_create(int fftLen, int chanN, int NC, int nSource, int halfBandShift, dsr_mk** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    mk_create_checks("MKSubbandBeamformer", fftLen, chanN, NC, nSource, halfBandShift);
    dsr_mk* s = new dsr_mk(); s->M = fftLen; s->C = chanN; *out = s;
  });
}
void dsr_mk_destroy(dsr_mk* s) { delete s; }

dsr_status dsr_mk_set_fixed_weights(dsr_mk* s, const double* wq, const double* B)
{ return guard([&] { if (!s || !wq) throw Error(DSR_E_PARAMETER, "null argument"); mk_fixed_set(*s, wq, B); }); }
dsr_status dsr_mk_set_fixed_weights_from_bf(dsr_mk* s, const dsr_bf* bf)
{ return guard([&] { if (!s || !bf) throw Error(DSR_E_PARAMETER, "null argument"); mk_fixed_from_bf(*s, bf); }); }
dsr_status dsr_mk_get_fixed_weights(const dsr_mk* s, double* wq, double* B)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); mk_fixed_get(*s, wq, B); }); }
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
    mk_apply(*s, X, U, Tmax, wa, Y, (hipStream_t) stream);
  });
}

}  // extern "C"
