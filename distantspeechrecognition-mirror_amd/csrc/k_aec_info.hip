// csrc/k_aec_info.hip -- the information-filter echo cancellers of btk/cancelVP, include/dsr.h section 2d.
//
// Restates InformationFilterEchoCancellationFeature (cancelVP.cc:388-650) and SquareRootInformationFilterEchoCancellationFeature (:655-1053)
// as two more kinds of the dsr_aec handle.  fp64 throughout, built without FMA contraction.  Two kernels:
//   k_aec_sqrt  the square-root kind.  Its (utterance, bin) chains share nothing (no counter, the three smoothed scalars are per bin), so
//               they spread over the device as k_aec_block's do: one wave a workgroup, LPC = 2 sampleN (rounded up to a power of two) lanes
//               per chain, 64 / LPC chains per wave, frames walked in order.  A chain's (2L+1) x 2L pre-array of the temporal update lives
//               in LDS, column-major, a lane per row: a Givens rotation touches two columns over the rows below the pivot.  The three
//               sweeps (:887-905 and :916-944, :997-1013, :1035-1051) keep the reference's rotation order; K and the information state stay
//               in the array's A22 block and last row from frame to frame, the observational update's extra column and the loading sweep's
//               scratch vector use column 0, which the temporal update rebuilds anyway.
//   k_aec_info  the plain kind.  The running count of skipped (frame, bin) pairs (:550-560) couples the bins of a frame, so one workgroup
//               owns an utterance and walks the frames, as k_aec_dtd does: (A) every bin's residual, the floor rule and both gates, (B) a
//               prefix count of the skip flags over the bins in order plus the carried counter, and the resets it causes, (C) the adapting
//               bins update, a wave per bin.  The two inverses of an update (:570, :617) are of Hermitian positive-definite matrices and
//               the reference's _invert is exact (its eigenvalue threshold is commented out, :496), so each is a Cholesky factorisation,
//               a forward substitution and the product Linv^H Linv, in the wave's LDS scratch.
// Nothing waits on another workgroup.
#include "launch.h"
#include "dev_math.h"
#include "aec.h"

using namespace dsr;

namespace {

struct IPar { double threshold, beta, su, amp, engTh, smooth, loading, load; };
struct ISt { double2* R; double2* K; double* sv; double2* H; double* band; double2* info; int* cnt; };      // cnt [U][4]: skip counter, resets, arithmetic error, -
struct ILayout { size_t oR, oK, oSv, oH, oB, oI, oC, bytes; };

ILayout ilayout(const dsr_aec& a, int U)
{
  const size_t n = (size_t) U * (a.M / 2 + 1), L = (size_t) a.L; ILayout l;
  l.oR = 0; l.oK = l.oR + n * L * 16; l.oSv = l.oK + n * L * L * 16; l.oH = l.oSv + n * 8; l.oB = l.oH + n * L * 16; l.oI = l.oB + n * 3 * 8;
  l.oC = l.oI + (a.kind == DSR_AEC_SQRT_INFO ? n * L * 16 : 0); l.bytes = l.oC + (size_t) U * 4 * 4;
  return l;
}
ISt icarve(const dsr_aec& a, void* base, int U)
{
  const ILayout l = ilayout(a, U); char* b = (char*) base;
  return ISt{(double2*) (b + l.oR), (double2*) (b + l.oK), (double*) (b + l.oSv), (double2*) (b + l.oH), (double*) (b + l.oB), (double2*) (b + l.oI), (int*) (b + l.oC)};
}



// sqrtKind: K = Sigma_u = I / sqrt(sigmau2) and the information state zero (:670-680), else K = sigmak2 I (:243); R = (1, 0, ...) (:405-407)
__global__ void k_aec_info_init(ISt s, long nChain, int L, int U, double k0, double sv0, int sqrtKind)
{
  const long c = (long) blockIdx.x * 256 + threadIdx.x;
  if (c < (long) U * 4) s.cnt[c] = 0;
  if (c >= nChain) return;
  s.sv[c] = sv0; s.band[c * 3] = 0.0; s.band[c * 3 + 1] = 0.0; s.band[c * 3 + 2] = 0.0;
  for (int i = 0; i < L; i++) {
    s.R[c * L + i] = make_double2(i == 0 ? 1.0 : 0.0, 0.0); s.H[c * L + i] = z2();
    if (sqrtKind) s.info[c * L + i] = z2();
    for (int j = 0; j < L; j++) s.K[(c * L + i) * L + j] = make_double2(i == j ? k0 : 0.0, 0.0);
  }
}

// _updateBand (:449-475): the bin's three smoothed scalars move on; true = adapt (sf >= 0, or a NaN sf, which `sf < 0` lets through)
__device__ __forceinline__ bool update_band(double2 Ak, double2 Ek, int frameX, const IPar& p, double& ek, double& sk, double& snr)
{
  const double sm = frameX < 100 ? 1.0 - (double) frameX * (1.0 - p.smooth) / 100.0 : p.smooth;
  const double2 Sk = make_double2(Ak.x - Ek.x, Ak.y - Ek.y);
  const double ce = abs2(Ek), cs = abs2(Sk);
  ek = ce * sm + ek * (1.0 - sm);
  sk = cs * sm + sk * (1.0 - sm);
  const double csnr = cs / (ce + 1.0e-15);
  snr = csnr * sm + snr * (1.0 - sm);
  double sf = -1.0;
  if (frameX < 100 || (snr > p.threshold && sk > p.engTh)) sf = 2.0 / (1.0 + exp(-snr)) - 1.0;
  return !(sf < 0.0);
}

// ---- the square-root kind -----------------------------------------------------------------------------------------------------------------
// X: the chain's array, column-major, NR = 2L+1 rows, 2L columns.  Lane q of the chain's LPC lanes owns row q; row 0 is never below a pivot, so
// lane 0 owns row 2L instead.
__global__ __launch_bounds__(64) void k_aec_sqrt(const float2* __restrict__ V, const float2* __restrict__ A, const int* __restrict__ nf, int U, int Tmax, int F, int L,
                                                 int LPC, IPar p, ISt s, float2* __restrict__ out, int frame0, int mode)
{
  extern __shared__ double2 ldsq[];
  const int lane = threadIdx.x, q = lane % LPC, cw = lane / LPC, CPW = 64 / LPC, chainBase = lane - q;
  const int NR = 2 * L + 1, NC = 2 * L, per = NC * NR + 2 * L;
  double2* X = ldsq + (size_t) cw * per; double2* Rl = X + NC * NR; double2* Hl = Rl + L;
  const long chain = (long) blockIdx.x * CPW + cw;
  const bool valid = chain < (long) U * F;
  const int u = valid ? (int) (chain / F) : 0, f = valid ? (int) (chain % F) : 0;
  int T = valid ? (nf ? nf[u] : Tmax) : 0; T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  int Tw = T;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const int x = __shfl_xor(Tw, o); Tw = x > Tw ? x : Tw; }
  const int myrow = q == 0 ? 2 * L : q; const bool rowLane = q < 2 * L;
  for (int e = q; e < per; e += LPC) X[e] = z2();
  __syncthreads();
  if (valid) {
    for (int e = q; e < L * L; e += LPC) { const int i = e / L, j = e % L; X[(L + j) * NR + L + i] = s.K[((size_t) chain * L + i) * L + j]; }
    for (int e = q; e < L; e += LPC) { X[(L + e) * NR + 2 * L] = s.info[(size_t) chain * L + e]; Rl[e] = s.R[(size_t) chain * L + e]; Hl[e] = s.H[(size_t) chain * L + e]; }
  }
  double sv = valid ? s.sv[chain] : 1.0;
  double ek = valid ? s.band[chain * 3] : 0.0, sk = valid ? s.band[chain * 3 + 1] : 0.0, snr = valid ? s.band[chain * 3 + 2] : 0.0;
  bool bad = false;
  __syncthreads();
  // one Givens rotation (:693-720): the pivot row's pair (ca, cb) gives c and s, rows piv+1 .. r1-1 of the two columns turn.  Every lane of
  // the wave runs it; `on` = the lane's chain adapts this frame (the others leave their array alone).
  auto rot = [&](int ca, int cb, int piv, int r1, bool on) {
    const double2 v1 = X[ca * NR + piv], v2 = X[cb * NR + piv];
    const double norm = sqrt(abs2(v1) + abs2(v2));
    const double2 c = make_double2(v1.x / norm, v1.y / norm), sn = make_double2(v2.x / norm, -v2.y / norm);
    if (on && rowLane && myrow > piv && myrow < r1) {
      const double2 a = X[ca * NR + myrow], b = X[cb * NR + myrow];
      const double2 p1 = cmul(cj(c), a), p2 = cmul(sn, b), p3 = cmul(c, b), p4 = cmul(cj(sn), a);
      X[ca * NR + myrow] = make_double2(p1.x + p2.x, p1.y + p2.y);
      X[cb * NR + myrow] = make_double2(p3.x - p4.x, p3.y - p4.y);
    }
    if (on && q == 0) { X[ca * NR + piv] = make_double2(norm, 0.0); X[cb * NR + piv] = z2(); }
    if (on && norm == 0.0) bad = true;                                               // _calcGivensRotation throws here (:699-700)
    __syncthreads();
  };
  const size_t base = (size_t) u * Tmax * F + f;
  for (int t = 0; t < Tw; t++) {
    const bool act = t < T;
    double2 nv = z2(), Ak = z2();
    if (act) { const float2 v = V[base + (size_t) t * F], a = A[base + (size_t) t * F]; nv = make_double2(p.amp * (double) v.x, p.amp * (double) v.y); Ak = make_double2(a.x, a.y); }
    double2 hin = z2();
    if (q < L) hin = q == 0 ? nv : Hl[q - 1];                                        // nextSample(playBlock, amp4play) (:757)
    __syncthreads();
    if (act && q < L) Hl[q] = hin;
    __syncthreads();
    double2 dot = z2();
    for (int j = 0; j < L; j++) { const double2 pr = cmul(Rl[j], Hl[j]); dot.x += pr.x; dot.y += pr.y; }      // zdotu(Rk, Vk) (:766)
    const double2 Ek = make_double2(Ak.x - dot.x, Ak.y - dot.y);
    if (act && q == 0) out[base + (size_t) t * F] = make_float2((float) Ek.x, (float) Ek.y);
    bool upd = false;
    if (act && abs2(Hl[0]) > p.threshold) upd = update_band(Ak, Ek, mode == 0 ? frame0 + t : -5, p, ek, sk, snr);      // :781
    if (!__any(upd)) continue;
    if (upd) sv = p.beta * sv + (1.0 - p.beta) * abs2(Ek);                           // :784-786
    // the temporal update's pre-array (:862-876): [[Sigma_u, -K], [0, K], [0, info]]; K and info are in place
    if (upd) {
      for (int e = q; e < L * NR; e += LPC) { const int c = e / NR, n = e % NR; X[e] = make_double2(n == c ? p.su : 0.0, 0.0); }
      for (int e = q; e < L * L; e += LPC) { const int c = e / L, n = e % L; const double2 k = X[(L + c) * NR + L + n]; X[(L + c) * NR + n] = make_double2(-k.x, -k.y); }
    }
    __syncthreads();
    for (int colX = 0; colX < L; colX++)                                             // zero out A12 (:887-905)
      for (int rowX = colX; rowX < L; rowX++) rot(rowX, L + colX, rowX, NR, upd);
    for (int rowX = 0; rowX < L - 1; rowX++)                                         // lower triangularize A22 (:916-944)
      for (int colX = L - 1; colX > rowX; colX--) rot(L + rowX, L + colX, L + rowX, NR, upd);
    // the observational update (:962-1013): its last column [conj(v); conj(A)] / sqrt(sigma2_v) goes to column 0, rows L..2L
    if (upd) {
      const double scale = 1.0 / sqrt(sv);
      if (q < L) { const double2 h = Hl[q]; X[L + q] = make_double2(h.x * scale, -h.y * scale); }
      if (q == 0) X[2 * L] = make_double2(Ak.x * scale, -Ak.y * scale);
    }
    __syncthreads();
    for (int rowX = 0; rowX < L; rowX++) rot(L + rowX, 0, L + rowX, NR, upd);
    for (int diagX = 0; diagX < L; diagX++) {                                        // _diagonalLoading (:1028-1053), the scratch vector in column 0
      if (upd && q < L) X[L + q] = make_double2(q == diagX ? p.load : 0.0, 0.0);
      __syncthreads();
      for (int colX = diagX; colX < L; colX++) rot(L + colX, 0, L + colX, 2 * L, upd);
    }
    // _extractCovarianceState (:723-735): K^H x = conj(info) from the last row up; lane j keeps row j's running difference, m descending
    double2 acc = z2();
    if (q < L) acc = cj(X[(L + q) * NR + 2 * L]);
    for (int m = L - 1; m >= 0; m--) {
      double2 x = z2();
      if (q == m) x = gsl_div(acc, cj(X[(L + m) * NR + L + m]));
      x = shfl2(x, chainBase + m);
      if (upd && q == m) Rl[m] = x;
      if (q < m) { const double2 pr = cmul(cj(X[(L + q) * NR + L + m]), x); acc = make_double2(acc.x - pr.x, acc.y - pr.y); }
    }
    __syncthreads();
  }
  if (!valid) return;
  if (q == 0) {
    for (int t = T; t < Tmax; t++) out[base + (size_t) t * F] = make_float2(0.f, 0.f);
    s.sv[chain] = sv; s.band[chain * 3] = ek; s.band[chain * 3 + 1] = sk; s.band[chain * 3 + 2] = snr;
  }
  for (int e = q; e < L * L; e += LPC) { const int i = e / L, j = e % L; s.K[((size_t) chain * L + i) * L + j] = X[(L + j) * NR + L + i]; }
  for (int e = q; e < L; e += LPC) { s.info[(size_t) chain * L + e] = X[(L + e) * NR + 2 * L]; s.R[(size_t) chain * L + e] = Rl[e]; s.H[(size_t) chain * L + e] = Hl[e]; }
  if (bad) s.cnt[(size_t) u * 4 + 2] = 1;
}

// ---- the plain kind: one workgroup per utterance -----------------------------------------------------------------------------------------
constexpr int INFO_NT = 256, INFO_NW = INFO_NT / 64, MAX_SKIPPED = 30;               // _maxSkippedN (:230)

// the inverse of the Hermitian positive-definite L x L matrix in Am (row-major, LDS), in place; Bm: scratch of the same size.  One wave.
__device__ void chol_invert(double2* Am, double2* Bm, int L, int lane)
{
  for (int j = 0; j < L; j++) {                                                      // right-looking Cholesky, lower triangle
    const double d = sqrt(Am[j * L + j].x);
    if (lane > j && lane < L) { const double2 a = Am[lane * L + j]; Am[lane * L + j] = make_double2(a.x / d, a.y / d); }
    if (lane == j) Am[j * L + j] = make_double2(d, 0.0);
    wave_sync();
    const int m = L - 1 - j;
    for (int e = lane; e < m * m; e += 64) {
      const int i = j + 1 + e / m, k = j + 1 + e % m;
      if (k <= i) { const double2 pr = cmul(Am[i * L + j], cj(Am[k * L + j])), a = Am[i * L + k]; Am[i * L + k] = make_double2(a.x - pr.x, a.y - pr.y); }
    }
    wave_sync();
  }
  if (lane < L) {                                                                    // forward substitution: lane c solves column c of the factor's inverse
    const int c = lane;
    for (int i = 0; i < c; i++) Bm[i * L + c] = z2();
    for (int i = c; i < L; i++) {
      double2 acc = make_double2(i == c ? 1.0 : 0.0, 0.0);
      for (int k = c; k < i; k++) { const double2 pr = cmul(Am[i * L + k], Bm[k * L + c]); acc = make_double2(acc.x - pr.x, acc.y - pr.y); }
      const double d = Am[i * L + i].x;
      Bm[i * L + c] = make_double2(acc.x / d, acc.y / d);
    }
  }
  wave_sync();
  for (int e = lane; e < L * L; e += 64) {                                           // Linv^H Linv
    const int a = e / L, b = e % L; double2 acc = z2();
    for (int k = a > b ? a : b; k < L; k++) { const double2 pr = cmul(cj(Bm[k * L + a]), Bm[k * L + b]); acc.x += pr.x; acc.y += pr.y; }
    Am[e] = acc;
  }
  wave_sync();
}

__global__ __launch_bounds__(INFO_NT) void k_aec_info(const float2* __restrict__ V, const float2* __restrict__ A, const int* __restrict__ nf, int U, int Tmax, int F, int L,
                                                      IPar p, ISt s, float2* __restrict__ out, int frame0, int mode)
{
  extern __shared__ double2 ldsi[];
  double2* Eb = ldsi;                                    // [F] the residual after the floor rule
  int* flag = (int*) (ldsi + F);                         // [F] 1 = skip, 0 = adapt
  const int tid = threadIdx.x, wave = tid / 64, lane = tid % 64, u = blockIdx.x;
  const size_t fl = ((size_t) F * 4 + 15) / 16;          // the flags, in double2 units
  double2* Am = ldsi + F + fl + (size_t) wave * (2 * L * L + 2 * L); double2* Bm = Am + L * L; double2* yv = Bm + L * L; double2* vv = yv + L;
  __shared__ int carried;
  int T = nf ? nf[u] : Tmax; T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  const size_t ubase = (size_t) u * Tmax * F;
  if (tid == 0) carried = s.cnt[(size_t) u * 4];
  // the played sample j frames before frame t, scaled: this call's frames, before them the carried history
  auto getv = [&](int f, int j, int t) -> double2 {
    const int tt = t - j;
    if (tt >= 0) { const float2 v = V[ubase + (size_t) tt * F + f]; return make_double2(p.amp * (double) v.x, p.amp * (double) v.y); }
    return s.H[((size_t) u * F + f) * L + (-tt - 1)];
  };
  __syncthreads();
  for (int t = 0; t < T; t++) {
    const int frameX = mode == 0 ? frame0 + t : -5;
    for (int f = tid; f < F; f += INFO_NT) {                                         // (A) :525-550
      const size_t chain = (size_t) u * F + f;
      const float2 a = A[ubase + (size_t) t * F + f]; const double2 Ak = make_double2(a.x, a.y);
      double2 dot = z2();
      for (int j = 0; j < L; j++) { const double2 pr = cmul(s.R[chain * L + j], getv(f, j, t)); dot.x += pr.x; dot.y += pr.y; }
      double2 Ek = make_double2(Ak.x - dot.x, Ak.y - dot.y);
      const double absE = hypot(Ek.x, Ek.y);
      if (absE < 0.01) Ek = make_double2(Ek.x / absE, Ek.y / absE);                  // _floorVal (:410, :533-535); 0 / 0 = NaN as in the reference
      out[ubase + (size_t) t * F + f] = make_float2((float) Ek.x, (float) Ek.y);
      bool upd = false;
      if (abs2(getv(f, 0, t)) > p.threshold) {
        double ek = s.band[chain * 3], sk = s.band[chain * 3 + 1], snr = s.band[chain * 3 + 2];
        upd = update_band(Ak, Ek, frameX, p, ek, sk, snr);
        s.band[chain * 3] = ek; s.band[chain * 3 + 1] = sk; s.band[chain * 3 + 2] = snr;
      }
      Eb[f] = Ek; flag[f] = upd ? 0 : 1;
    }
    __syncthreads();
    if (wave == 0) {                                                                 // (B) :550-560 as a prefix count, 64 bins at a time
      int total = carried;                                                           // the counter the next skip would find, were there no wrap
      for (int f0 = 0; f0 < F; f0 += 64) {
        const int f = f0 + lane; const bool sk = f < F && flag[f] != 0;
        const unsigned long long m = __ballot(sk);
        const int before = total + __popcll(m & ((1ull << lane) - 1ull));            // skips counted before this one
        if (sk && before > 0 && before % MAX_SKIPPED == 0) {
          const size_t chain = (size_t) u * F + f;
          for (int j = 0; j < L; j++) s.R[chain * L + j] = make_double2(j == 0 ? 1.0 : 0.0, 0.0);
          atomicAdd(&s.cnt[(size_t) u * 4 + 1], 1);
        }
        total += __popcll(m);
      }
      if (lane == 0 && total != carried) carried = (total - 1) % MAX_SKIPPED + 1;
    }
    for (int f = wave; f < F; f += INFO_NW) {                                        // (C) :562-619, a wave per adapting bin
      if (flag[f] != 0) continue;
      const size_t chain = (size_t) u * F + f;
      const double2 Ek = Eb[f]; const float2 af = A[ubase + (size_t) t * F + f]; const double2 Ak = make_double2(af.x, af.y);
      const double sv = p.beta * s.sv[chain] + (1.0 - p.beta) * abs2(Ek);            // :563-565
      for (int e = lane; e < L * L; e += 64) { double2 k = s.K[chain * L * L + e]; if (e / L == e % L) k.x = p.su + k.x; Am[e] = k; }      // :568-569
      if (lane < L) vv[lane] = getv(f, lane, t);
      wave_sync();
      chol_invert(Am, Bm, L, lane);                                                  // Y- (:570)
      const double scale = 1.0 / sv;
      double2 value = z2();
      if (lane < L) {
        double2 y = z2();
        for (int j = 0; j < L; j++) { const double2 pr = cmul(Am[lane * L + j], s.R[chain * L + j]); y.x += pr.x; y.y += pr.y; }      // y- = Y- R (:571)
        const double2 v = vv[lane]; value = make_double2(v.x * scale, -v.y * scale);
        const double2 ik = cmul(value, Ak);                                          // :584-587
        yv[lane] = make_double2(y.x + ik.x, y.y + ik.y);                             // :597
      }
      wave_sync();
      for (int e = lane; e < L * L; e += 64) {                                       // conj(v) v^T / sigma2_v + Y- (:589-596), the loading (:611-614)
        const int i = e / L, j = e % L; const double2 vi = vv[i], vl = make_double2(vi.x * scale, -vi.y * scale), pr = cmul(vl, vv[j]), y = Am[e];
        double2 sij = make_double2(pr.x + y.x, pr.y + y.y);
        if (i == j) sij.x = sij.x + p.loading;
        Am[e] = sij;
      }
      wave_sync();
      chol_invert(Am, Bm, L, lane);                                                  // K (:617-618)
      for (int e = lane; e < L * L; e += 64) s.K[chain * L * L + e] = Am[e];
      if (lane < L) {
        double2 r = z2();
        for (int j = 0; j < L; j++) { const double2 pr = cmul(Am[lane * L + j], yv[j]); r.x += pr.x; r.y += pr.y; }      // R = K y (:619)
        s.R[chain * L + lane] = r;
      }
      if (lane == 0) s.sv[chain] = sv;
      wave_sync();
    }
    __syncthreads();
  }
  if (tid == 0) s.cnt[(size_t) u * 4] = carried;
  for (int f = tid; f < F; f += INFO_NT) {
    for (int t = T; t < Tmax; t++) out[ubase + (size_t) t * F + f] = make_float2(0.f, 0.f);
    if (T > 0) for (int k = L - 1; k >= 0; k--) s.H[((size_t) u * F + f) * L + k] = getv(f, k, T - 1);      // descending: reads index k - T < k
  }
}

struct IScratch { DevBuf<unsigned char> st; };
PerStream<IScratch> g_iscratch;

size_t sqrt_lds(int L, int LPC) { return (size_t) (64 / LPC) * ((size_t) 2 * L * (2 * L + 1) + 2 * L) * sizeof(double2); }
size_t info_lds(int F, int L) { return ((size_t) F + ((size_t) F * 4 + 15) / 16 + (size_t) INFO_NW * (2 * L * L + 2 * L)) * sizeof(double2); }

}  // namespace

namespace dsr {
namespace aec_info {

size_t state_bytes(const dsr_aec& a, int U) { return ilayout(a, U).bytes; }

void init_state(const dsr_aec& a, void* state, int U, hipStream_t st)
{
  const ISt s = icarve(a, state, U); const long n = (long) U * (a.M / 2 + 1);
  const bool sq = a.kind == DSR_AEC_SQRT_INFO;
  launch(k_aec_info_init, dim3(cdiv(n > (long) U * 4 ? n : (long) U * 4, 256)), dim3(256), 0, st, s, n, a.L, U, sq ? 1.0 / sqrt(a.sigmau2) : a.sigmak2,
                     a.sigmau2, sq ? 1 : 0);
}

void apply(const dsr_aec& a, const float2* V, const float2* A, const int* nf, int U, int Tmax, int frame0, float2* out, void* state, hipStream_t st)
{
  const int F = a.M / 2 + 1, L = a.L;
  if (a.kind == DSR_AEC_INFO && F > 1024) throw Error(DSR_E_DIMENSION, "information filter: fftLen %d above 2046 (a frame's per-bin residuals live in LDS)", a.M);
  if (!state) { IScratch& sc = g_iscratch.at(st); sc.st.reserve(ilayout(a, U).bytes); state = sc.st.p; init_state(a, state, U, st); }
  const ISt s = icarve(a, state, U);
  const bool sq = a.kind == DSR_AEC_SQRT_INFO;
  IPar p{a.threshold, a.beta, sq ? 1.0 / sqrt(a.sigmau2) : a.sigmau2, a.amp, a.engTh, a.smooth, a.loading, sqrt(a.loading)};      // _load = sqrt(loading) (:660)
  if (sq) {
    int LPC = 2; while (LPC < 2 * L) LPC *= 2;                                       // 2 .. 64 lanes a chain
    const size_t lds = sqrt_lds(L, LPC);
    launch(k_aec_sqrt, dim3(cdiv((long) U * F, 64 / LPC)), dim3(64), lds, st, V, A, nf, U, Tmax, F, L, LPC, p, s, out, frame0, a.frameMode);
    // _calcGivensRotation's jarithmetic_error (:699-700): the kernel records a zero norm per utterance
    std::vector<int> cnt((size_t) U * 4);
    DSR_HIP(hipMemcpyAsync(cnt.data(), s.cnt, cnt.size() * 4, hipMemcpyDeviceToHost, st));
    DSR_HIP(hipStreamSynchronize(st));
    for (int u = 0; u < U; u++) if (cnt[(size_t) u * 4 + 2]) throw Error(DSR_E_ARITHMETIC, "calcGivensRotation: Norm is zero (utterance %d).", u);
  } else {
    const size_t lds = info_lds(F, L);
    launch(k_aec_info, dim3(U), dim3(INFO_NT), lds, st, V, A, nf, U, Tmax, F, L, p, s, out, frame0, a.frameMode);
  }
}

void read(const dsr_aec& a, const void* state, int U, int what, double* host_out, size_t outDoubles)
{
  const ILayout l = ilayout(a, U); const size_t n = (size_t) U * (a.M / 2 + 1), L = (size_t) a.L;
  const bool sq = a.kind == DSR_AEC_SQRT_INFO;
  size_t off, doubles;
  switch (what) {
    case DSR_AEC_STATE_FILTER: off = l.oR; doubles = n * L * 2; break;
    case DSR_AEC_STATE_K: off = l.oK; doubles = n * L * L * 2; break;
    case DSR_AEC_STATE_SIGMA2V: off = l.oSv; doubles = n; break;
    case DSR_AEC_STATE_HISTORY: off = l.oH; doubles = n * L * 2; break;
    case DSR_AEC_STATE_BAND: off = l.oB; doubles = n * 3; break;
    case DSR_AEC_STATE_INFO: if (!sq) throw Error(DSR_E_PARAMETER, "not a square-root information filter"); off = l.oI; doubles = n * L * 2; break;
    case DSR_AEC_STATE_SKIPPED: case DSR_AEC_STATE_RESETS:
      if (sq) throw Error(DSR_E_PARAMETER, "the square-root information filter has no skip counter"); off = l.oC; doubles = (size_t) U; break;
    default: throw Error(DSR_E_PARAMETER, "state part %d: not a part of an information filter's state", what);
  }
  if (outDoubles < doubles) throw Error(DSR_E_DIMENSION, "state part %d needs %zu doubles, the buffer holds %zu", what, doubles, outDoubles);
  require_device();
  DSR_HIP(hipDeviceSynchronize());
  if (what == DSR_AEC_STATE_SKIPPED || what == DSR_AEC_STATE_RESETS) {
    std::vector<int> tmp((size_t) U * 4);
    DSR_HIP(hipMemcpy(tmp.data(), (const char*) state + off, tmp.size() * 4, hipMemcpyDeviceToHost));
    for (int u = 0; u < U; u++) host_out[u] = (double) tmp[(size_t) u * 4 + (what == DSR_AEC_STATE_RESETS ? 1 : 0)];
  } else {
    DSR_HIP(hipMemcpy(host_out, (const char*) state + off, doubles * 8, hipMemcpyDeviceToHost));
  }
}

}  // namespace aec_info
}  // namespace dsr

extern "C" {

dsr_status dsr_aec_create_info(int squareRoot, int fftLen, int sampleN, dsr_aec** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftLen <= 0 || (fftLen & 1)) throw Error(DSR_E_PARAMETER, "fftLen %d: a positive even number is needed", fftLen);
    if (sampleN < 1 || sampleN > DSR_AEC_MAX_SAMPLE_N) throw Error(DSR_E_PARAMETER, "sampleN %d outside [1, %d]", sampleN, DSR_AEC_MAX_SAMPLE_N);
    dsr_aec* a = new dsr_aec(); a->kind = squareRoot ? DSR_AEC_SQRT_INFO : DSR_AEC_INFO; a->M = fftLen; a->L = sampleN;
    a->threshold = 2.0;                                                              // snrTh (cancelVP.i:162), the base class's threshold (cancelVP.cc:392)
    *out = a;
  });
}

dsr_status dsr_aec_set_info(dsr_aec* a, double snrTh, double engTh, double smooth, double loading)
{
  return guard([&] {
    if (!a) throw Error(DSR_E_PARAMETER, "null argument");
    if (!aec_info::is_info(*a)) throw Error(DSR_E_PARAMETER, "not an information filter echo canceller");
    a->threshold = snrTh; a->engTh = engTh; a->smooth = smooth; a->loading = loading;
  });
}

}  // extern "C"
