// csrc/k_wpe_tiled.hip -- multi-channel WPE past the LDS working set of k_wpe_multi (MultiChannelWPEDereverberation,
// btk/dereverberation/dereverberation.cc:281-620), at array size: 64 channels x 16 taps (C P <= 1024 stacked lags).
//
// The stacked lag vector x_n[t], t = ch P + l, is y_ch[n - lowerN - l] (zero before frame 0 and from nframes on); it is the same for every
// channel, only the weight 1 / theta_c[n] differs.  It is never materialised: every kernel reads it from the transposed copy of the
// snapshots Yt [utterance][subband][channel][frame] (k_wpe_series).  Four stages per iteration, separated by kernel boundaries, over chunks of
// (utterance, subband) pairs whose matrices fit the workspace:
//   k_wt_resid<false>  theta: d_c[n] = g_c^H x_n for all channels of a subband, one complex [N x CP].[CP x C] product on the fp64 MFMA;
//                      writes 1 / max(|y_c[n] - d_c[n]|, 1e-3)^2 (zero from nframes on)
//   k_wt_gram          R_c = sum_n x_n x_n^H / theta_c[n], lower block triangle, 32 x 32 (complex) tiles x 8 channels a workgroup: one LDS
//                      slab of x feeds the accumulators of all 8 channels (the weight goes onto the row operand in registers)
//   k_wt_rvec          r_c = sum_n conj(y_c[n]) x_n / theta_c[n], a complex [CP x N].[N x C] product
//   k_wt_chol          loading (:529-544), blocked Cholesky (16 x 16 diagonal block in LDS, panel by rows, trailing Hermitian update on
//                      the MFMA), the two triangular solves; one workgroup per (utterance, subband, channel) matrix in the HBM workspace
// and k_wt_resid<true> for getOutput (:365-395).  Everything accumulates in fp64 from the fp32 snapshots.  Deviation kept from the LDS kernels:
// the terms are weighted with the reciprocal of theta_n (one division per frame).  A matrix that is not positive definite gives NaN filters
// for its (utterance, channel, subband) and nothing else.
//
// The fp64 MFMA helpers and the instruction's lane map: csrc/mfma64.h.
#include "launch.h"
#include "mfma64.h"
#include <cmath>

namespace dsr {

// x_n[t] from the subband's series yb [C][Nmax]
__device__ __forceinline__ float2 lagv(const float2* yb, int Nmax, int N, int P, int lowerN, int n, int t)
{
  const int ch = t / P, l = t - ch * P, ix = n - lowerN - l;
  return (ix >= 0 && ix < N) ? yb[(long) ch * Nmax + ix] : make_float2(0.f, 0.f);
}
__device__ __forceinline__ bool wt_selected(int b, int M, int lowerBW) { return (b <= lowerBW) || (b >= M - lowerBW); }    // dereverberation.cc:552

// residual y_c[n] - g^H x_n: a wave owns 16 frames x 16 channels of one (utterance, subband); OUT: the output frames (filterChan >= 0: every
// channel through that channel's filter), else 1 / theta_c[n] into rth [chunk pair][C][Npad]
template <bool OUT>
__global__ __launch_bounds__(256) void k_wt_resid(const float2* __restrict__ Yt, const int* __restrict__ nframesArr, const double2* __restrict__ gn,
                                                  double* __restrict__ rth, float2* __restrict__ out, int ub0, int C, int Nmax, int Npad, int F, int M,
                                                  int lowerN, int P, int lowerBW, int filterChan)
{
  const int lane = threadIdx.x & 63, n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16, c0 = blockIdx.y * 16;
  const int ubl = blockIdx.z, ub = ub0 + ubl, u = ub / F, b = ub - u * F;
  if (n0 >= (OUT ? Nmax : Npad)) return;                                    // wave-uniform
  const int N = nframesArr[u] < Nmax ? nframesArr[u] : Nmax, PT = P * C;
  const bool sel = wt_selected(b, M, lowerBW);
  if (!OUT && !sel) return;
  const float2* yb = Yt + (long) ub * C * Nmax;
  const int i = lane & 15, kq = lane >> 4;
  const int cB = c0 + i, fB = filterChan >= 0 ? filterChan : cB;
  const double2* gB = cB < C ? gn + (((long) u * C + fB) * F + b) * PT : nullptr;
  d4 dr = {0.0, 0.0, 0.0, 0.0}, di = {0.0, 0.0, 0.0, 0.0};
  if (sel && n0 + 15 >= lowerN && n0 < N) {
    for (int t0 = 0; t0 < PT; t0 += 4) {                                    // D[n][c] = sum_t x_n[t] conj(g_c[t])
      const int t = t0 + kq;
      const float2 a = t < PT ? lagv(yb, Nmax, N, P, lowerN, n0 + i, t) : make_float2(0.f, 0.f);
      const double2 g = (t < PT && gB) ? gB[t] : make_double2(0.0, 0.0);
      cmfma((double) a.x, (double) a.y, g.x, -g.y, dr, di);
    }
  }
  const int c = c0 + (lane & 15);
  if (c >= C) return;
  const float2* yc = yb + (long) c * Nmax;
  for (int q = 0; q < 4; q++) {
    const int n = n0 + (lane >> 4) + 4 * q;
    if (OUT) {
      if (n >= Nmax) continue;
      float2 o = make_float2(0.f, 0.f);
      if (n < N) {
        const float2 v = yc[n]; double cr = (double) v.x, ci = (double) v.y;
        if (sel && n >= lowerN) { cr -= dr[q]; ci -= di[q]; }
        o = make_float2((float) cr, (float) ci);
      }
      out[(((long) u * C + c) * Nmax + n) * F + b] = o;
    } else {
      if (n >= Npad) continue;
      double w = 0.0;
      if (n < N) {                                                          // _calculateThetan (:499-527)
        const float2 v = yc[n]; double cr = (double) v.x, ci = (double) v.y;
        if (n >= lowerN) { cr -= dr[q]; ci -= di[q]; }
        double th = hypot(cr, ci); if (th < 1.0E-03) th = 1.0E-03;
        w = 1.0 / (th * th);
      }
      rth[((long) ubl * C + c) * Npad + n] = w;
    }
  }
}

// r_c[t] = sum_n conj(y_c[n]) w_c[n] x_n[t]: a wave owns 16 lags x 16 channels; rv [chunk pair][C][PT]
__global__ __launch_bounds__(256) void k_wt_rvec(const float2* __restrict__ Yt, const int* __restrict__ nframesArr, const double* __restrict__ rth,
                                                 double2* __restrict__ rv, int ub0, int C, int Nmax, int Npad, int F, int M, int lowerN, int P, int lowerBW)
{
  const int lane = threadIdx.x & 63, t0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 16, c0 = blockIdx.y * 16;
  const int ubl = blockIdx.z, ub = ub0 + ubl, u = ub / F, b = ub - u * F, PT = P * C;
  if (t0 >= PT || !wt_selected(b, M, lowerBW)) return;
  const int N = nframesArr[u] < Nmax ? nframesArr[u] : Nmax;
  const float2* yb = Yt + (long) ub * C * Nmax;
  const int i = lane & 15, kq = lane >> 4, tA = t0 + i, cB = c0 + i;
  const float2* yB = cB < C ? yb + (long) cB * Nmax : nullptr;
  const double* wB = cB < C ? rth + ((long) ubl * C + cB) * Npad : nullptr;
  d4 sr = {0.0, 0.0, 0.0, 0.0}, si = {0.0, 0.0, 0.0, 0.0};
  for (int n0 = 0; n0 < N; n0 += 4) {
    const int n = n0 + kq;                                                  // n < Npad: rth is zero from N on
    const float2 a = tA < PT ? lagv(yb, Nmax, N, P, lowerN, n, tA) : make_float2(0.f, 0.f);
    double br = 0.0, bi = 0.0;
    if (yB && n < N) { const float2 v = yB[n]; const double w = wB[n]; br = (double) v.x * w; bi = -(double) v.y * w; }
    cmfma((double) a.x, (double) a.y, br, bi, sr, si);
  }
  const int c = c0 + (lane & 15);
  if (c >= C) return;
  for (int q = 0; q < 4; q++) {
    const int t = t0 + (lane >> 4) + 4 * q;
    if (t < PT) rv[((long) ubl * C + c) * PT + t] = make_double2(sr[q], si[q]);
  }
}

// R_c, lower block triangle: workgroup = one 32 x 32 tile (I, J), J <= I, of 8 channels' matrices of one (utterance, subband); wave w owns
// channels cg 8 + 2 w and + 1.  Per slab of 32 frames: the tile's 32 row lags and 32 column lags (fp32) and the 8 channels' weights in LDS.
constexpr int WT_TILE = 32, WT_SLAB = 32, WT_CG = 8;
__global__ __launch_bounds__(256) void k_wt_gram(const float2* __restrict__ Yt, const int* __restrict__ nframesArr, const double* __restrict__ rth,
                                                 double2* __restrict__ Rws, int ub0, int C, int Nmax, int Npad, int F, int M, int lowerN, int P, int lowerBW)
{
  __shared__ float2 xr[WT_TILE][WT_SLAB + 1], xc[WT_TILE][WT_SLAB + 1];
  __shared__ double ws[WT_CG][WT_SLAB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ubl = blockIdx.z, ub = ub0 + ubl, u = ub / F, b = ub - u * F, PT = P * C;
  if (!wt_selected(b, M, lowerBW)) return;
  int I = (int) ((sqrt(8.0 * blockIdx.x + 1.0) - 1.0) * 0.5);              // blockIdx.x = I (I + 1) / 2 + J
  while (I * (I + 1) / 2 > (int) blockIdx.x) I--; while ((I + 1) * (I + 2) / 2 <= (int) blockIdx.x) I++;
  const int J = blockIdx.x - I * (I + 1) / 2, r0 = I * WT_TILE, q0 = J * WT_TILE;
  const int cg0 = blockIdx.y * WT_CG;
  const int N = nframesArr[u] < Nmax ? nframesArr[u] : Nmax;
  const float2* yb = Yt + (long) ub * C * Nmax;
  const int i = lane & 15, kq = lane >> 4;
  d4 acc[2][2][2][2];                                                       // [channel of the wave][row half][column half][re, im]
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int q = 0; q < 2; q++) { acc[a][p][q][0] = (d4){0.0, 0.0, 0.0, 0.0}; acc[a][p][q][1] = (d4){0.0, 0.0, 0.0, 0.0}; }
  const int ca = cg0 + 2 * wv;                                              // this wave's channels ca, ca + 1 (either may be >= C)
  for (int s0 = 0; s0 < N; s0 += WT_SLAB) {
    __syncthreads();
    for (int e = tid; e < WT_TILE * WT_SLAB; e += 256) {
      const int row = e / WT_SLAB, k = e - row * WT_SLAB, n = s0 + k;
      xr[row][k] = r0 + row < PT ? lagv(yb, Nmax, N, P, lowerN, n, r0 + row) : make_float2(0.f, 0.f);
      xc[row][k] = q0 + row < PT ? lagv(yb, Nmax, N, P, lowerN, n, q0 + row) : make_float2(0.f, 0.f);
    }
    for (int e = tid; e < WT_CG * WT_SLAB; e += 256) {
      const int cl = e / WT_SLAB, k = e - cl * WT_SLAB, c = cg0 + cl;
      ws[cl][k] = c < C ? rth[((long) ubl * C + c) * Npad + s0 + k] : 0.0;  // s0 + k < Npad (Npad: Nmax rounded up to the slab)
    }
    __syncthreads();
    if (ca >= C) continue;                                                  // wave-uniform
#pragma unroll 2
    for (int k0 = 0; k0 < WT_SLAB; k0 += 4) {
      const int k = k0 + kq;
      const float2 a0 = xr[i][k], a1 = xr[16 + i][k], b0 = xc[i][k], b1 = xc[16 + i][k];
      const double bR[2] = {(double) b0.x, (double) b1.x}, bI[2] = {-(double) b0.y, -(double) b1.y};     // B = conj(x[col])
#pragma unroll
      for (int a = 0; a < 2; a++) {
        const double w = ws[2 * wv + a][k];
        const double aR[2] = {w * (double) a0.x, w * (double) a1.x}, aI[2] = {w * (double) a0.y, w * (double) a1.y};
#pragma unroll
        for (int p = 0; p < 2; p++)
#pragma unroll
          for (int q = 0; q < 2; q++) cmfma(aR[p], aI[p], bR[q], bI[q], acc[a][p][q][0], acc[a][p][q][1]);
      }
    }
  }
#pragma unroll
  for (int a = 0; a < 2; a++) {
    const int c = ca + a;
    if (c >= C) continue;
    double2* Rc = Rws + ((long) ubl * C + c) * PT * PT;
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
    for (int q = 0; q < 2; q++)
#pragma unroll
    for (int z = 0; z < 4; z++) {
      const int row = r0 + 16 * p + (lane >> 4) + 4 * z, col = q0 + 16 * q + (lane & 15);
      if (row < PT && col < PT) Rc[(long) row * PT + col] = make_double2(acc[a][p][q][0][z], acc[a][p][q][1][z]);
    }
  }
}

// loading, blocked Cholesky (lower, in place) and the two solves of one (utterance, subband, channel) matrix; g -> gn
constexpr int WT_NB = 16, WT_PTMAX = 1024;
__global__ __launch_bounds__(256) void k_wt_chol(double2* __restrict__ Rws, const double2* __restrict__ rv, double2* __restrict__ gn, int ub0, int C,
                                                 int F, int M, int P, int lowerBW, double loadFactor)
{
  __shared__ double2 L[WT_NB][WT_NB + 1];
  __shared__ double2 x[WT_PTMAX];
  __shared__ double red[256];
  __shared__ int s_fail;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c = blockIdx.x, ubl = blockIdx.y, ub = ub0 + ubl, u = ub / F, b = ub - u * F, PT = P * C;
  double2* gOut = gn + (((long) u * C + c) * F + b) * PT;
  if (!wt_selected(b, M, lowerBW)) { for (int t = tid; t < PT; t += 256) gOut[t] = make_double2(0.0, 0.0); return; }
  double2* A = Rws + ((long) ubl * C + c) * PT * PT;
  // _loadR: |R_kk| + max_k |R_kk| 10^(loadDb / 10) on the diagonal
  double mx = 0.0;
  for (int k = tid; k < PT; k += 256) { const double2 v = A[(long) k * PT + k]; const double d = hypot(v.x, v.y); if (d > mx) mx = d; }
  red[tid] = mx;
  if (tid == 0) s_fail = 0;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if (tid < s && red[tid + s] > red[tid]) red[tid] = red[tid + s]; __syncthreads(); }
  const double maxd = red[0];
  for (int k = tid; k < PT; k += 256) { const double2 v = A[(long) k * PT + k]; A[(long) k * PT + k] = make_double2(hypot(v.x, v.y) + maxd * loadFactor, 0.0); }
  for (int t = tid; t < PT; t += 256) x[t] = rv[((long) ubl * C + c) * PT + t];
  __syncthreads();
  const int ti = tid >> 4, tk = tid & 15;                                   // this thread's entry of the diagonal block
  for (int kb = 0; kb < PT; kb += WT_NB) {
    const int nb = PT - kb < WT_NB ? PT - kb : WT_NB;
    if (ti < nb && tk <= ti) L[ti][tk] = A[(long) (kb + ti) * PT + kb + tk];
    __syncthreads();
    for (int j = 0; j < nb; j++) {                                          // the diagonal block, right-looking in LDS
      if (tid == 0) { const double d = L[j][j].x; if (!(d > 0.0)) s_fail = 1; else L[j][j] = make_double2(sqrt(d), 0.0); }
      __syncthreads();
      if (s_fail) break;
      if (tk == j && ti > j && ti < nb) { const double d = L[j][j].x; L[ti][j] = make_double2(L[ti][j].x / d, L[ti][j].y / d); }
      __syncthreads();
      if (tk > j && tk <= ti && ti < nb) {
        const double2 p = L[ti][j], q = L[tk][j];                           // L[ti][tk] -= p conj(q)
        L[ti][tk].x -= p.x * q.x + p.y * q.y; L[ti][tk].y -= p.y * q.x - p.x * q.y;
      }
      __syncthreads();
    }
    if (s_fail) break;
    if (ti < nb && tk <= ti) A[(long) (kb + ti) * PT + kb + tk] = L[ti][tk];
    for (int row = kb + nb + tid; row < PT; row += 256) {                   // panel: X L_kk^H = A[row][kb:kb+nb], by rows
      double2 v[WT_NB]; double2* Ar = A + (long) row * PT + kb;          // (constant trip counts: v stays in registers)
#pragma unroll
      for (int j = 0; j < WT_NB; j++) v[j] = j < nb ? Ar[j] : make_double2(0.0, 0.0);
#pragma unroll
      for (int j = 0; j < WT_NB; j++) {
        double sr = v[j].x, si = v[j].y;
#pragma unroll
        for (int k = 0; k < j; k++) { const double2 p = v[k], q = L[j][k]; sr -= p.x * q.x + p.y * q.y; si -= p.y * q.x - p.x * q.y; }
        const double d = j < nb ? L[j][j].x : 1.0; v[j] = make_double2(sr / d, si / d);
      }
#pragma unroll
      for (int j = 0; j < WT_NB; j++) if (j < nb) Ar[j] = v[j];
    }
    __syncthreads();
    // trailing Hermitian update A[i][j] -= X_i X_j^H over 16 x 16 tiles of the lower triangle below the panel, one tile a wave at a time
    const int t0 = kb + nb, nt = (PT - t0 + 15) / 16, nPairs = nt * (nt + 1) / 2;
    for (int pr = wv; pr < nPairs; pr += 4) {
      int a = (int) ((sqrt(8.0 * pr + 1.0) - 1.0) * 0.5); while (a * (a + 1) / 2 > pr) a--; while ((a + 1) * (a + 2) / 2 <= pr) a++;
      const int bb = pr - a * (a + 1) / 2, R0 = t0 + 16 * a, C0 = t0 + 16 * bb;
      d4 cr, ci;
      for (int z = 0; z < 4; z++) {
        const int row = R0 + (lane >> 4) + 4 * z, col = C0 + (lane & 15);
        const double2 v = (row < PT && col < PT) ? A[(long) row * PT + col] : make_double2(0.0, 0.0);
        cr[z] = v.x; ci[z] = v.y;
      }
      const int ra = R0 + (lane & 15), cb = C0 + (lane & 15);
      for (int k0 = 0; k0 < nb; k0 += 4) {
        const int k = k0 + (lane >> 4);
        const double2 p = (ra < PT && k < nb) ? A[(long) ra * PT + kb + k] : make_double2(0.0, 0.0);
        const double2 q = (cb < PT && k < nb) ? A[(long) cb * PT + kb + k] : make_double2(0.0, 0.0);
        cmfma(-p.x, -p.y, q.x, -q.y, cr, ci);                               // -= p conj(q)
      }
      for (int z = 0; z < 4; z++) {
        const int row = R0 + (lane >> 4) + 4 * z, col = C0 + (lane & 15);
        if (row < PT && col < PT && col <= row) A[(long) row * PT + col] = make_double2(cr[z], ci[z]);
      }
    }
    __syncthreads();
  }
  if (s_fail) { for (int t = tid; t < PT; t += 256) gOut[t] = make_double2(NAN, NAN); return; }
  // L y = r, then L^H g = y, in blocks of 16: the block by one thread, the rest of the vector by all
  for (int kb = 0; kb < PT; kb += WT_NB) {
    const int nb = PT - kb < WT_NB ? PT - kb : WT_NB;
    if (tid == 0)
      for (int j = kb; j < kb + nb; j++) {
        double sr = x[j].x, si = x[j].y; const double2* Aj = A + (long) j * PT;
        for (int k = kb; k < j; k++) { const double2 a = Aj[k]; sr -= a.x * x[k].x - a.y * x[k].y; si -= a.x * x[k].y + a.y * x[k].x; }
        const double d = Aj[j].x; x[j] = make_double2(sr / d, si / d);
      }
    __syncthreads();
    for (int i2 = kb + nb + tid; i2 < PT; i2 += 256) {
      double sr = x[i2].x, si = x[i2].y; const double2* Ai = A + (long) i2 * PT;
      for (int k = kb; k < kb + nb; k++) { const double2 a = Ai[k]; sr -= a.x * x[k].x - a.y * x[k].y; si -= a.x * x[k].y + a.y * x[k].x; }
      x[i2] = make_double2(sr, si);
    }
    __syncthreads();
  }
  for (int kb = ((PT - 1) / WT_NB) * WT_NB; kb >= 0; kb -= WT_NB) {
    const int nb = PT - kb < WT_NB ? PT - kb : WT_NB;
    if (tid == 0)
      for (int j = kb + nb - 1; j >= kb; j--) {
        double sr = x[j].x, si = x[j].y;
        for (int k = j + 1; k < kb + nb; k++) { const double2 a = A[(long) k * PT + j]; const double ar = a.x, ai = -a.y; sr -= ar * x[k].x - ai * x[k].y; si -= ar * x[k].y + ai * x[k].x; }
        const double d = A[(long) j * PT + j].x; x[j] = make_double2(sr / d, si / d);
      }
    __syncthreads();
    for (int i2 = tid; i2 < kb; i2 += 256) {
      double sr = x[i2].x, si = x[i2].y;
      for (int k = kb; k < kb + nb; k++) { const double2 a = A[(long) k * PT + i2]; const double ar = a.x, ai = -a.y; sr -= ar * x[k].x - ai * x[k].y; si -= ar * x[k].y + ai * x[k].x; }
      x[i2] = make_double2(sr, si);
    }
    __syncthreads();
  }
  for (int t = tid; t < PT; t += 256) gOut[t] = x[t];
}

// The tiled path.  Yt: the transposed snapshots (k_wpe_series); gn: the filters (zero, or the previous block's when warm) in and the result out.
void wpe_multi_tiled(const float2* Yt, const int32_t* nframes, int U, int C, int Nmax, int fftLen, int lowerN, int P, int iterationsN, double loadFactor,
                     int lowerBW, int filterChan, float2* out, double2* gn, bool warm, hipStream_t st)
{
  const int F = fftLen / 2 + 1, PT = P * C, UF = U * F;
  const int Npad = (Nmax + WT_SLAB - 1) / WT_SLAB * WT_SLAB;
  if (!warm) DSR_HIP(hipMemsetAsync(gn, 0, sizeof(double2) * (size_t) UF * C * PT, st));
  if (iterationsN > 0) {
    // workspace per (utterance, subband): C matrices PT x PT, C right-hand sides, C weight series; chunks of pairs within WT_WS_BYTES
    const size_t perPair = (size_t) C * PT * PT * sizeof(double2) + (size_t) C * PT * sizeof(double2) + (size_t) C * Npad * sizeof(double);
    const size_t budget = (size_t) 4 << 30;
    int nub = (int) (budget / perPair); if (nub < 1) nub = 1; if (nub > UF) nub = UF;
    double2* Rws = nullptr;
    DSR_HIP(hipMallocAsync((void**) &Rws, perPair * nub, st));
    double2* rv = Rws + (size_t) nub * C * PT * PT;
    double* rth = reinterpret_cast<double*>(rv + (size_t) nub * C * PT);
    const int T = (PT + WT_TILE - 1) / WT_TILE;
    for (int it = 0; it < iterationsN; it++)
      for (int ub0 = 0; ub0 < UF; ub0 += nub) {
        const int n = UF - ub0 < nub ? UF - ub0 : nub;
        launch(k_wt_resid<false>, dim3((Npad + 63) / 64, (C + 15) / 16, n), dim3(256), 0, st, Yt, nframes, (const double2*) gn, rth, (float2*) nullptr,
                           ub0, C, Nmax, Npad, F, fftLen, lowerN, P, lowerBW, -1);
        launch(k_wt_gram, dim3(T * (T + 1) / 2, (C + WT_CG - 1) / WT_CG, n), dim3(256), 0, st, Yt, nframes, (const double*) rth, Rws,
                           ub0, C, Nmax, Npad, F, fftLen, lowerN, P, lowerBW);
        launch(k_wt_rvec, dim3((PT + 63) / 64, (C + 15) / 16, n), dim3(256), 0, st, Yt, nframes, (const double*) rth, rv,
                           ub0, C, Nmax, Npad, F, fftLen, lowerN, P, lowerBW);
        launch(k_wt_chol, dim3(C, n), dim3(256), 0, st, Rws, (const double2*) rv, gn, ub0, C, F, fftLen, P, lowerBW, loadFactor);
      }
    DSR_HIP(hipFreeAsync(Rws, st));
  }
  launch(k_wt_resid<true>, dim3((Nmax + 63) / 64, (C + 15) / 16, UF), dim3(256), 0, st, Yt, nframes, (const double2*) gn, (double*) nullptr, out,
                     0, C, Nmax, Npad, F, fftLen, lowerN, P, lowerBW, filterChan);
}

}  // namespace dsr
