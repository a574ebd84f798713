// csrc/k_lpc.hip -- LPC / MVDR spectral-envelope features, batched over frames.
//
// Replaces (btk/feature): BaseFeature::fftPower (lpc.cc:44-63), WarpFeature::autoCorrelation (lpc.cc:80-139),
// BurgFeature::autoCorrelation (lpc.cc:158-207), MVDRFeature<>::next (lpc.h:134-195) and LPCFeature<>::next
// (lpc.h:291-331), i.e. the operators WarpMVDRFeature, BurgMVDRFeature, WarpLPCFeature and BurgLPCFeature.
// Further down: WarpedTwiceMVDRFeature (lpc.cc:212-468) and SpectralSmoothing (lpc.cc:473-529), the header's other two operators.
//
// The recursions of one frame are sequential and in fp32 (warped all-pass chain, Levinson-Durbin, Burg lattice); they
// are kept in the reference's order so that results agree to the last bit, and the parallelism comes from the frames:
// one thread per frame, every per-frame array stored [index][frame] so that a wave's accesses are contiguous.
// The spectrum of the (short) coefficient sequence is a direct fp64 DFT on the reference's 2^ceil(log2 dim)-point grid,
// of which -- as in the reference -- the first dim/2+1 bins are the output.  Compiled with -ffp-contract=off.
#include "launch.h"
#include <cmath>

namespace dsr {

__global__ void k_lpc_transpose(const float* __restrict__ X, int Tc, int dim, float* __restrict__ XT)
{
  __shared__ float tile[32][33];
  const int j0 = blockIdx.x * 32, t0 = blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y) { const int t = t0 + r, j = j0 + threadIdx.x; tile[r][threadIdx.x] = (t < Tc && j < dim) ? X[(size_t) t * dim + j] : 0.f; }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += blockDim.y) { const int j = j0 + r, t = t0 + threadIdx.x; if (t < Tc && j < dim) XT[(size_t) j * Tc + t] = tile[threadIdx.x][r]; }
}

// WarpFeature::autoCorrelation (lpc.cc:80-139).  Scratch (all [index][Tc]): WX dim, R order+1, A0/A1 order+1.
__global__ void k_lpc_warp(const float* __restrict__ XT, int Tc, int dim, int order, float warp, float* __restrict__ WX,
                           float* __restrict__ R, float* __restrict__ A0, float* __restrict__ A1, float* __restrict__ LP, float* __restrict__ E0)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Tc) return;
  const size_t S = (size_t) Tc;
  float sum = 0.0f;
  for (int j = 0; j < dim; j++) { const float x = XT[j * S + t]; sum += x * x; WX[j * S + t] = x; }
  R[t] = sum;
  for (int i = 1; i <= order; i++) {
    // one all-pass stage in place: new[j] = warp (new[j-1] - old[j]) + old[j-1], new[0] = -warp old[0]
    float prevOld = 0.0f, prevNew = 0.0f; sum = 0.0f;
    for (int j = 0; j < dim; j++) {
      const float old = WX[j * S + t];
      const float nw = (j == 0) ? -warp * old : warp * (prevNew - old) + prevOld;
      WX[j * S + t] = nw; prevOld = old; prevNew = nw;
      sum += XT[j * S + t] * nw;
    }
    R[i * S + t] = sum;
  }
  float E = R[t];
  E0[t] = E;
  float* prev = A0; float* cur = A1;
  for (int i = 1; i <= order; i++) {
    float k = R[i * S + t];
    for (int j = 1; j < i; j++) k -= prev[j * S + t] * R[(i - j) * S + t];
    if (E != 0) k /= E; else k = 1000000000;
    cur[i * S + t] = k;
    for (int j = 1; j <= i - 1; j++) cur[j * S + t] = prev[j * S + t] - k * prev[(i - j) * S + t];
    E = (1 - k * k) * E;
    float* tmp = prev; prev = cur; cur = tmp;
  }
  LP[t] = 1.0f;
  for (int i = 1; i <= order; i++) LP[i * S + t] = -prev[i * S + t];
}

// BurgFeature::autoCorrelation (lpc.cc:158-207).  Scratch: EF, EB dim; A, Af order+1 (A is the output).
__global__ void k_lpc_burg(const float* __restrict__ XT, int Tc, int dim, int order, float* __restrict__ EF, float* __restrict__ EB,
                           float* __restrict__ A, float* __restrict__ Af, float* __restrict__ E0)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Tc) return;
  const size_t S = (size_t) Tc;
  float e0 = 0.0f;
  for (int j = 0; j < dim; j++) { const float x = XT[j * S + t]; e0 += x * x; EF[j * S + t] = x; EB[j * S + t] = x; }
  E0[t] = e0;
  for (int i = 0; i <= order; i++) { Af[i * S + t] = 0.0f; A[i * S + t] = 0.0f; }
  for (int i = 0; i < order; i++) {
    const int n = dim - i - 1;
    double num = 0.0, den = 0.0;
    for (int j = 0; j < n; j++) {
      const float efp = EF[(j + 1) * S + t], ebp = EB[j * S + t];
      num -= (double) (2 * ebp * efp);
      den += (double) (efp * efp + ebp * ebp);
    }
    const float k = (float) ((double) (float) num / den);
    for (int j = 0; j < n; j++) {
      const float efp = EF[(j + 1) * S + t], ebp = EB[j * S + t];
      EF[j * S + t] = efp + k * ebp; EB[j * S + t] = ebp + k * efp;
    }
    A[t] = 1.0f;
    for (int j = 0; j <= i + 1; j++) Af[j * S + t] = A[(i - j + 1) * S + t];
    for (int j = 1; j <= i + 1; j++) A[j * S + t] += k * Af[j * S + t];
  }
}

// MVDRFeature: the (order+1) distinct values of the symmetric sequence PC (lpc.h:157-170): V[i] = PC[order+i]
__global__ void k_lpc_mvdr_pc(const float* __restrict__ A, const float* __restrict__ E0, int Tc, int order, float* __restrict__ V)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Tc) return;
  const size_t S = (size_t) Tc; const bool pos = E0[t] > 0;
  for (int i = 0; i <= order; i++) {
    double temp = 0;
    for (int ii = 0; ii <= order - i; ii++) temp += (double) ((float) (order + 1 - i - 2 * ii) * A[ii * S + t] * A[(ii + i) * S + t]);
    V[i * S + t] = pos ? (float) -temp : 10000000.0f;
  }
}

// power spectrum of PA on the N-point grid + the envelope value.  kind 0: PA[n] = V[|n-1-order|], n = 1..2 order+1;
// kind 1: PA[n] = A[n-1], n = 1..order+1 (the shift by one "because of fft", lpc.h:172-174,318-319).
__global__ void k_lpc_envelope(const float* __restrict__ C, const float* __restrict__ E0, int Tc, int dim, int order, int N, int kind,
                               const double2* __restrict__ tw, double* __restrict__ out)
{
  const int outN = dim / 2 + 1;
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long) Tc * outN) return;
  const int t = (int) (idx / outN), k = (int) (idx - (long) t * outN);
  const size_t S = (size_t) Tc;
  const int L = (kind == 0) ? 2 * order + 1 : order + 1;
  double re = 0.0, im = 0.0;
  for (int n = 1; n <= L && n < dim; n++) {                    // (fftPower reads power[0..dim) only)
    const int ci = (kind == 0) ? ((n - 1 - order) < 0 ? order + 1 - n : n - 1 - order) : n - 1;
    const double v = (double) C[ci * S + t];
    const double2 w = tw[(int) (((long) n * k) % N)];
    re += v * w.x; im -= v * w.y;
  }
  const float p = (k == 0 || k == N / 2) ? (float) (re * re) : (float) (re * re + im * im);
  const float e0 = E0[t];
  double o;
  if (kind == 0) { o = sqrt((double) p); o = (o > 0) ? (double) e0 / o : 10000000.0; }
  else { o = (double) p; o = (o > 0) ? (double) (2 * e0) / (o * (double) dim) : 10000000.0; }
  out[idx] = o;
}

struct LpcPlan {
  int dim = 0, order = 0, method = 0, kind = 0, N = 0; float warp = 0.f;
  DevBuf<float> xt, s1, s2, r, a0, a1, lp, e0, v; DevBuf<double2> tw;
};

}  // namespace dsr

using namespace dsr;
struct dsr_lpc : LpcPlan {};

extern "C" {

dsr_status dsr_lpc_create(int dim, int order, int correlate, float warp, int method, int kind, dsr_lpc** out)
{
  return guard([&] {
    (void) correlate;                                          // stored but never used by the reference (lpc.h:124,302)
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (dim < 2 || order < 1) throw Error(DSR_E_PARAMETER, "bad dimension %d / order %d", dim, order);
    if (order >= dim / 2 + 1) throw Error(DSR_E_PARAMETER, "Order (%d) and dimension (%d) do not match.", order, dim / 2 + 1);   // lpc.h:126-127
    if (method < 0 || method > 1 || kind < 0 || kind > 1) throw Error(DSR_E_PARAMETER, "method/kind must be 0 or 1");
    require_device();
    dsr_lpc* p = new dsr_lpc(); p->dim = dim; p->order = order; p->warp = warp; p->method = method; p->kind = kind;
    const unsigned l2 = (unsigned) ceil(log((double) dim) / log(2.0));                 // lpc.cc:32-35
    p->N = 1 << l2;
    std::vector<double2> tw((size_t) p->N);
    for (int m = 0; m < p->N; m++) { const double a = 2.0 * M_PI * (double) m / (double) p->N; tw[m].x = cos(a); tw[m].y = sin(a); }
    p->tw.upload(tw);
    *out = p;
  });
}
void dsr_lpc_destroy(dsr_lpc* p) { delete p; }
int dsr_lpc_size(const dsr_lpc* p) { return p ? p->dim / 2 + 1 : 0; }

dsr_status dsr_lpc_run(dsr_lpc* p, const float* frames_dev, int64_t T, double* out_dev, void* stream)
{
  return guard([&] {
    if (!p || !frames_dev || !out_dev) throw Error(DSR_E_PARAMETER, "null argument");
    hipStream_t st = (hipStream_t) stream;
    const int dim = p->dim, order = p->order, outN = dim / 2 + 1;
    const int chunk = 65536;
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
      const int Tc = (int) ((T - t0 < chunk) ? T - t0 : chunk);
      const size_t S = (size_t) Tc;
      p->xt.reserve(S * dim); p->s1.reserve(S * dim); p->e0.reserve(S); p->lp.reserve(S * (order + 1));
      launch(k_lpc_transpose, dim3(cdiv(dim, 32), cdiv(Tc, 32)), dim3(32, 8), 0, st, frames_dev + t0 * dim, Tc, dim, p->xt.p);
      const int nb = cdiv(Tc, 64);
      if (p->method == 0) {
        p->r.reserve(S * (order + 1)); p->a0.reserve(S * (order + 1)); p->a1.reserve(S * (order + 1));
        launch(k_lpc_warp, dim3(nb), dim3(64), 0, st, p->xt.p, Tc, dim, order, p->warp, p->s1.p, p->r.p, p->a0.p, p->a1.p, p->lp.p, p->e0.p);
      } else {
        p->s2.reserve(S * dim); p->a0.reserve(S * (order + 1));
        launch(k_lpc_burg, dim3(nb), dim3(64), 0, st, p->xt.p, Tc, dim, order, p->s1.p, p->s2.p, p->lp.p, p->a0.p, p->e0.p);
      }
      const float* coef = p->lp.p;
      if (p->kind == 0) {
        p->v.reserve(S * (order + 1));
        launch(k_lpc_mvdr_pc, dim3(nb), dim3(64), 0, st, p->lp.p, p->e0.p, Tc, order, p->v.p);
        coef = p->v.p;
      }
      const long n = (long) Tc * outN;
      launch(k_lpc_envelope, dim3((unsigned) ((n + 255) / 256)), dim3(256), 0, st, coef, p->e0.p, Tc, dim, order, p->N, p->kind,
                         p->tw.p, out_dev + t0 * outN);
    }
  });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------------------------------------------
// WarpedTwiceMVDRFeature (lpc.h:205-246, lpc.cc:212-468) and SpectralSmoothing (lpc.h:342-358, lpc.cc:473-529).
//
// One thread per frame again, but the two long loop nests of the reference are interchanged so that a frame's state is short enough for LDS:
//   autocorrelation (lpc.cc:251-273): the samples are streamed once, and all order+1 all-pass stages advance by one sample at a time; the state is
//     R, the stages' previous input and previous output: 3 (order+2) floats a frame instead of dim;
//   trans_longchain (lpc.cc:374-389): the chain is run stage by stage over the tim = 2 order + 1 input samples; the state is those tim floats
//     instead of the dim+1 of xm.
// Every operation keeps its operands and every accumulator its order of addends, so the results are those of the reference's order to the last
// bit.  State element i of lane l lies at [i][l] in LDS (each lane its own bank); where 3 (order+2) 64 floats exceed a CU's LDS both kernels keep
// the same state [i][Tc] in global scratch.
namespace dsr {

// lpc.cc:392-407,425-428 (R1R0, rewarp), :244-324 (autoCorrelation), :432-445 (PC).  V[i] = PC[order+i], E0 = E[0], RW = _rewarp.
template <bool LDS> __global__ void __launch_bounds__(64)
k_wt_lp(const float* __restrict__ XT, const float* __restrict__ warps, int Tc, int dim, int order, int correlate, float warp0, int fixed, float sens,
        float* __restrict__ gstate, float* __restrict__ V, float* __restrict__ E0, float* __restrict__ RW)
{
  extern __shared__ double2 wt_lds[];
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= Tc) return;
  const size_t S = (size_t) Tc, ss = LDS ? (size_t) 64 : S;
  float* st = LDS ? reinterpret_cast<float*>(wt_lds) + threadIdx.x : gstate + t;
  const int n = order + 2;                                     // R[0..order+1]: the compensation reads R[order+1] (lpc.cc:259-260)
  float* R = st; float* PO = st + (size_t) n * ss; float* PN = st + (size_t) 2 * n * ss;
  const float warp = warps ? warps[t] : warp0;
  for (int i = 0; i < n; i++) R[i * ss] = 0.0f;
  float r0 = 0.0f, c0 = 0.0f, c1 = 0.0f, xp = 0.0f;
  for (int j = 0; j < dim; j++) {
    const float x = XT[j * S + t];
    r0 += x * x;
    if (j < correlate) { c0 += x * x; if (j >= 1) c1 += xp * x; }
    float old = x;
    for (int i = 1; i < n; i++) {                              // stage i: new[j] = warp (new[j-1] - old[j]) + old[j-1], new[0] = -warp old[0]
      const float nw = (j == 0) ? -warp * old : warp * (PN[i * ss] - old) + PO[i * ss];
      R[i * ss] += x * nw; PO[i * ss] = old; PN[i * ss] = nw; old = nw;
    }
    xp = x;
  }
  float wv;
  if (fixed) wv = sens + warp;                                 // lpc.cc:352-355
  else { const float r = fabsf(c1 / c0); wv = (float) ((double) sens * ((double) r - 0.5) + (double) warp); }   // lpc.cc:404,426
  const float rewarp = (wv - warp) / (1 - wv * warp);
  RW[t] = rewarp;
  // compensate for the warp value (lpc.cc:275-288); the double promotions are the reference's
  float a0 = (warp + rewarp) / (1 + warp * rewarp);
  const float gj = (float) (1.0 - (double) (a0 * a0));
  const float a1 = a0 / gj;
  a0 = (float) ((1.0 + (double) (a0 * a0)) / (double) gj);
  float g1 = r0;
  const float R0 = (float) ((double) (a0 * r0) + 2.0 * (double) a1 * (double) R[ss]);
  R[0] = R0;
  for (int i = 1; i <= order; i++) { const float ri = R[i * ss]; R[i * ss] = a0 * ri + a1 * (g1 + R[(i + 1) * ss]); g1 = ri; }
  float E = R0;
  E0[t] = E;
  float* prev = PO; float* cur = PN;                           // the all-pass state is done with: columns i-1 and i of _tmpA
  for (int i = 1; i <= order; i++) {
    float k = R[i * ss];
    for (int j = 1; j < i; j++) k -= prev[j * ss] * R[(i - j) * ss];
    if (E != 0) k /= E; else k = 1000000000;
    cur[i * ss] = k;
    for (int j = 1; j <= i - 1; j++) cur[j * ss] = prev[j * ss] - k * prev[(i - j) * ss];
    E = (1 - k * k) * E;
    float* tmp = prev; prev = cur; cur = tmp;
  }
  prev[0] = 1.0f;
  for (int i = 1; i <= order; i++) prev[i * ss] = -prev[i * ss];
  const bool pos = R0 > 0;
  for (int i = 0; i <= order; i++) {                           // float accumulator here (lpc.cc:433), signed weights as in lpc.h:156
    float temp = 0;
    for (int ii = 0; ii <= order - i; ii++) temp += (float) (order + 1 - i - 2 * ii) * prev[ii * ss] * prev[(ii + i) * ss];
    V[i * S + t] = pos ? -temp : 10000000.0f;
  }
}

// trans_longchain(PC, dim, -rewarp, PA, 2 order + 1) (lpc.cc:374-389,447-448), stage by stage: PA[e] is the last input of stage e
template <bool LDS> __global__ void __launch_bounds__(64)
k_wt_chain(const float* __restrict__ V, const float* __restrict__ RW, int Tc, int dim, int order, float* __restrict__ gstate, float* __restrict__ PAT,
           float* __restrict__ pa_out)
{
  extern __shared__ double2 wt_lds[];
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= Tc) return;
  const size_t S = (size_t) Tc, ss = LDS ? (size_t) 64 : S;
  float* x = LDS ? reinterpret_cast<float*>(wt_lds) + threadIdx.x : gstate + t;
  const int tim = 2 * order + 1;
  for (int w = 0; w < tim; w++) x[w * ss] = V[(size_t) (w < order ? order - w : w - order) * S + t];
  const float lam = -RW[t];
  float* pa = pa_out ? pa_out + (size_t) t * (dim + 1) : nullptr;
  for (int e = 0; e < dim; e++) {
    const float last = x[(size_t) (tim - 1) * ss];
    PAT[e * S + t] = last;
    if (pa) pa[e] = last;
    if (e == dim - 1) break;
    float xm1 = 0.0f, ym1 = 0.0f;
    for (int w = 0; w < tim; w++) {
      const float xw = x[w * ss];
      const float y = (xm1 + lam * ym1) - lam * xw;            // lpc.cc:383
      x[w * ss] = y; xm1 = xw; ym1 = y;
    }
  }
  if (pa) pa[dim] = 0.0f;                                       // xm[dim] is never written (lpc.cc:447)
}

// fftPower of PA[0..dim) on the N-point grid (lpc.cc:44-60) and the envelope (lpc.cc:457-465), as a direct fp64 sum.  A workgroup takes F frames;
// with LDS the twiddles and the frames' PA are staged there.
template <bool LDS> __global__ void __launch_bounds__(256)
k_wt_envelope(const float* __restrict__ PAT, const float* __restrict__ E0, int Tc, int dim, int N, int F, const double2* __restrict__ tw,
              double* __restrict__ out)
{
  extern __shared__ double2 wt_lds[];
  const int outN = dim / 2 + 1, f0 = blockIdx.x * F, tid = threadIdx.x;
  const size_t S = (size_t) Tc;
  double2* sTw = wt_lds; double* sPA = reinterpret_cast<double*>(wt_lds + N);
  if (LDS) {
    for (int m = tid; m < N; m += 256) sTw[m] = tw[m];
    for (int it = tid; it < F * dim; it += 256) {
      const int n = it / F, f = it - n * F, tt = f0 + f;
      sPA[(size_t) f * dim + n] = (tt < Tc) ? (double) PAT[n * S + tt] : 0.0;
    }
    __syncthreads();
  }
  for (int it = tid; it < F * outN; it += 256) {
    const int f = it / outN, k = it - f * outN, tt = f0 + f;
    if (tt >= Tc) break;
    double re = 0.0, im = 0.0; unsigned idx = 0;
    for (int n = 0; n < dim; n++) {
      const double v = LDS ? sPA[(size_t) f * dim + n] : (double) PAT[n * S + tt];
      const double2 w = LDS ? sTw[idx] : tw[idx];
      re = fma(v, w.x, re); im = fma(-v, w.y, im);
      idx = (idx + (unsigned) k) & (unsigned) (N - 1);
    }
    const float p = (k == 0 || k == N / 2) ? (float) (re * re) : (float) (re * re + im * im);
    double o = sqrt((double) p);
    o = (o > 0) ? (double) E0[tt] / o : 10000000.0;
    out[(size_t) tt * outN + k] = o;
  }
}

// SpectralSmoothing::next (lpc.cc:485-529): a wave per frame
__global__ void __launch_bounds__(64) k_specsmooth(const double* __restrict__ to, const double* __restrict__ from, int size, double* __restrict__ out)
{
  const size_t row = (size_t) blockIdx.x * size; const int lane = threadIdx.x;
  float maxFFT = 0.0f, maxSPEC = 0.0f;
  for (int i = lane; i < size; i += 64) {
    float r = 0.0f;
    if (i >= 2 && i + 2 < size) {
      const double* f = from + row + i;
      r = (float) (f[-2] / 9.0 + 2.0 * f[-1] / 9.0 + f[0] / 3.0 + 2.0 * f[1] / 9.0 + f[2] / 9.0);
    }
    if (maxFFT < r) maxFFT = r;
    const float v = (float) to[row + i];
    if (maxSPEC < v) maxSPEC = v;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float a = __shfl_xor(maxFFT, off), b = __shfl_xor(maxSPEC, off);
    if (maxFFT < a) maxFFT = a;
    if (maxSPEC < b) maxSPEC = b;
  }
  float mult;
  if ((double) maxSPEC < 0.01) mult = 100 * maxFFT; else mult = maxFFT / maxSPEC;
  for (int i = lane; i < size; i += 64) out[row + i] = (double) mult * to[row + i];
}

struct WtPlan {
  int dim = 0, order = 0, correlate = 0, N = 0, fixed = 0; float warp = 0.f, sens = 0.f;
  DevBuf<float> xt, st, v, e0, rw, pat; DevBuf<double2> tw;
  bool timing = false; double kms[4] = {0, 0, 0, 0};           // dsr_wtmvdr_set_timing: ms of transpose, k_wt_lp, k_wt_chain, k_wt_envelope
};

}  // namespace dsr

struct dsr_wtmvdr : dsr::WtPlan {};

extern "C" {

dsr_status dsr_wtmvdr_create(int dim, int order, int correlate, float warp, int warpFactorFixed, float sensibility, dsr_wtmvdr** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (dim < 2 || order < 1) throw Error(DSR_E_PARAMETER, "bad dimension %d / order %d", dim, order);
    if (correlate < 10) correlate = dim;                                                 // lpc.cc:348
    if (order >= dim / 2 + 1) throw Error(DSR_E_PARAMETER, "Order (%d) and dimension (%d) do not match.", order, dim / 2 + 1);   // lpc.cc:349-350
    if (correlate > dim) throw Error(DSR_E_PARAMETER, "correlate (%d) exceeds the frame length (%d)", correlate, dim);          // R1R0 would read past the frame
    require_device();
    dsr_wtmvdr* p = new dsr_wtmvdr(); p->dim = dim; p->order = order; p->correlate = correlate; p->warp = warp; p->fixed = warpFactorFixed ? 1 : 0; p->sens = sensibility;
    const unsigned l2 = (unsigned) ceil(log((double) dim) / log(2.0));                 // lpc.cc:32-35
    p->N = 1 << l2;
    std::vector<double2> tw((size_t) p->N);
    for (int m = 0; m < p->N; m++) { const double a = 2.0 * M_PI * (double) m / (double) p->N; tw[m].x = cos(a); tw[m].y = sin(a); }
    p->tw.upload(tw);
    *out = p;
  });
}
void dsr_wtmvdr_destroy(dsr_wtmvdr* p) { delete p; }
int dsr_wtmvdr_size(const dsr_wtmvdr* p) { return p ? p->dim / 2 + 1 : 0; }

dsr_status dsr_wtmvdr_run(dsr_wtmvdr* p, const float* frames_dev, const float* warp_dev, int64_t T, double* out_dev, float* pa_dev, float* rewarp_dev,
                          void* stream)
{
  return guard([&] {
    if (!p || !frames_dev || !out_dev) throw Error(DSR_E_PARAMETER, "null argument");
    hipStream_t st = (hipStream_t) stream;
    const int dim = p->dim, order = p->order, outN = dim / 2 + 1, N = p->N, tim = 2 * order + 1;
    // the state of a wave's 64 frames: 3 (order+2) floats a frame for the autocorrelation, 2 order + 1 for the chain (always the smaller).  One
    // rule for both kernels: LDS where the larger fits a CU's 160 KiB (order <= 211), global scratch otherwise.
    const size_t lds1 = (size_t) 3 * (order + 2) * 64 * sizeof(float), lds2 = (size_t) tim * 64 * sizeof(float);
    const bool lds = lds1 <= 160 * 1024;
    // the transform: twiddles and F frames of PA as doubles in at most 64 KiB of LDS, else read from global memory
    int F = (int) (((long) 64 * 1024 - (long) N * 16) / ((long) dim * 8));
    const bool ldsE = F >= 1;
    if (!ldsE || F > 8) F = 8;
    const size_t lds3 = ldsE ? (size_t) N * 16 + (size_t) F * dim * 8 : 0;
    const int chunk = 65536;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    if (p->timing) { for (int i = 0; i < 5; i++) DSR_HIP(hipEventCreate(&ev[i])); for (int i = 0; i < 4; i++) p->kms[i] = 0.0; }
    auto mark = [&](int i) { if (p->timing) DSR_HIP(hipEventRecord(ev[i], st)); };
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
      const int Tc = (int) ((T - t0 < chunk) ? T - t0 : chunk);
      const size_t S = (size_t) Tc;
      p->xt.reserve(S * dim); p->pat.reserve(S * dim); p->e0.reserve(S); p->rw.reserve(S); p->v.reserve(S * (order + 1));
      if (!lds) p->st.reserve(S * 3 * (order + 2));
      mark(0);
      launch(k_lpc_transpose, dim3(cdiv(dim, 32), cdiv(Tc, 32)), dim3(32, 8), 0, st, frames_dev + t0 * dim, Tc, dim, p->xt.p);
      mark(1);
      const int nb = cdiv(Tc, 64);
      const float* wd = warp_dev ? warp_dev + t0 : nullptr;
      float* pa = pa_dev ? pa_dev + t0 * (dim + 1) : nullptr;
      if (lds) {
        launch(k_wt_lp<true>, dim3(nb), dim3(64), lds1, st, p->xt.p, wd, Tc, dim, order, p->correlate, p->warp, p->fixed, p->sens, (float*) nullptr, p->v.p, p->e0.p, p->rw.p);
        mark(2);
        launch(k_wt_chain<true>, dim3(nb), dim3(64), lds2, st, p->v.p, p->rw.p, Tc, dim, order, (float*) nullptr, p->pat.p, pa);
      } else {
        launch(k_wt_lp<false>, dim3(nb), dim3(64), 0, st, p->xt.p, wd, Tc, dim, order, p->correlate, p->warp, p->fixed, p->sens, p->st.p, p->v.p, p->e0.p, p->rw.p);
        mark(2);
        launch(k_wt_chain<false>, dim3(nb), dim3(64), 0, st, p->v.p, p->rw.p, Tc, dim, order, p->st.p, p->pat.p, pa);
      }
      mark(3);
      if (ldsE) launch(k_wt_envelope<true>, dim3(cdiv(Tc, F)), dim3(256), lds3, st, p->pat.p, p->e0.p, Tc, dim, N, F, p->tw.p, out_dev + t0 * outN);
      else launch(k_wt_envelope<false>, dim3(cdiv(Tc, F)), dim3(256), 0, st, p->pat.p, p->e0.p, Tc, dim, N, F, p->tw.p, out_dev + t0 * outN);
      mark(4);
      if (rewarp_dev) DSR_HIP(hipMemcpyAsync(rewarp_dev + t0, p->rw.p, S * sizeof(float), hipMemcpyDeviceToDevice, st));
      if (p->timing) {
        DSR_HIP(hipEventSynchronize(ev[4]));
        for (int i = 0; i < 4; i++) { float ms = 0.f; DSR_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1])); p->kms[i] += (double) ms; }
      }
    }
    if (p->timing) for (int i = 0; i < 5; i++) (void) hipEventDestroy(ev[i]);
  });
}
dsr_status dsr_wtmvdr_set_timing(dsr_wtmvdr* p, int on)
{ return guard([&] { if (!p) throw Error(DSR_E_PARAMETER, "null argument"); p->timing = on != 0; }); }
dsr_status dsr_wtmvdr_kernel_ms(const dsr_wtmvdr* p, double* ms4)
{ return guard([&] { if (!p || !ms4) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 4; i++) ms4[i] = p->kms[i]; }); }

dsr_status dsr_specsmooth_run(const double* adjust_to_dev, const double* adjust_from_dev, int64_t T, int size, double* out_dev, void* stream)
{
  return guard([&] {
    if (size < 2) throw Error(DSR_E_PARAMETER, "SpectralSmoothing needs at least 2 coefficients, got %d", size);   // size()-2 wraps around below that (lpc.cc:500,507)
    if (!adjust_to_dev || !adjust_from_dev || !out_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (T <= 0) return;
    if (T > 0x7fffffff) throw Error(DSR_E_PARAMETER, "too many frames");
    launch(k_specsmooth, dim3((unsigned) T), dim3(64), 0, (hipStream_t) stream, adjust_to_dev, adjust_from_dev, size, out_dev);
  });
}

}  // extern "C"
