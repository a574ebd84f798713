// csrc/abf_kernels.hip -- the kernels of the data-adaptive subband beamformers of btk/lib/subbandBeamforming.py, their dispatch and their launch:
// SubbandBeamformerGriffithsJim (:982-1104), SubbandBeamformerMVDR (:1107-1183, sample matrix inversion) and SubbandBeamformerMPDR (:1185-1265), and
// the fixed-weight apply of SubbandBeamformerDS / SubbandBeamformerGSC (:350-436, :549-676).  The handle and what this file exports: csrc/abf.h.
//
// As k_gsc_rls (csrc/k_beamform.hip): one thread owns one (utterance, bin) and walks the frames, all fp64; a thread's state is an array of complex
// entries that lives in registers (compile-time channel counts), in LDS as [entry][lane] (conflict free) while the 64 lanes' entries fit, else in
// memory as [entry][utterance x bin] (coalesced).  The sample-matrix kernels also need the Cholesky factor of the loaded matrix: it never shares
// the registers with the matrix (a triangle of order 8 is 72 fp64 values, the two together would leave nothing for the vectors), it lies in LDS
// next to a register-resident state.
#include "launch.h"
#include "dev_math.h"
#include "abf.h"

using namespace dsr;

namespace {

__device__ __forceinline__ int tri(int i, int j) { return i * (i + 1) / 2 + j; }          // entry (i, j), j <= i, of a stored lower triangle

// sigmaK of a frame (:1014): |x_0|^2 / fftLen over the full spectrum of channel 0 -- DC and Nyquist once, the bins in between twice.
// One wave per (utterance, frame).
__global__ __launch_bounds__(64) void k_abf_power(const float2* __restrict__ X, double* __restrict__ sig, int C, int Tmax, int F, int fftLen)
{
  const long ut = blockIdx.x; const int u = (int) (ut / Tmax), t = (int) (ut - (long) u * Tmax);
  const float2* row = X + (((long) u * C) * Tmax + t) * F;
  double s = 0.0;
  for (int f = threadIdx.x; f < F; f += 64) {
    const float2 v = row[f]; const double p = (double) v.x * (double) v.x + (double) v.y * (double) v.y;
    s += (f == 0 || f == F - 1) ? p : 2.0 * p;
  }
  s = wave_sum(s);
  if (threadIdx.x == 0) sig[ut] = s / (double) fftLen;
}

// One thread per utterance walks its frames: where the call's first frame stands in the stream (start[u]), and for Griffiths-Jim the step size of
// every frame, negative where the gate is closed (:1017-1021, :1087).  utt [U][4]: frame counter, gamma, average power -- the carried part.
__global__ __launch_bounds__(64) void k_abf_frames(const double* __restrict__ sig, double* __restrict__ gam, int* __restrict__ start,
                                                   double* __restrict__ utt, const int* __restrict__ nframesArr, int U, int Tmax, int gj, double gamma0,
                                                   double avg0, double beta, double silThresh, int staticAfter, int carryIn)
{
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  const int Tu = clampT(nframesArr, u, Tmax);
  int k = carryIn ? (int) utt[4 * u] : 0; double gamma = carryIn ? utt[4 * u + 1] : gamma0, avg = carryIn ? utt[4 * u + 2] : avg0;
  start[u] = k;
  if (gj)
    for (int t = 0; t < Tu; t++) {
      if (k + t == staticAfter) gamma /= 10.0;
      const double s = sig[(long) u * Tmax + t];
      gam[(long) u * Tmax + t] = s > avg / silThresh ? gamma : -1.0;
      avg = avg * beta + (1.0 - beta) * s;
    }
  utt[4 * u] = (double) (k + Tu); utt[4 * u + 1] = gamma; utt[4 * u + 2] = avg; utt[4 * u + 3] = 0.0;
}

// the post-filter weight of frame t (:376-379, :1078-1081, :1154-1155): rows t < wpFrames[u] of wp [U][Tmax][F] scale the output
__device__ __forceinline__ float2 abf_out(double2 y, const float* wp, const int* wpFrames, int u, int t, int Tmax, int F, int f)
{
  if (wp && (!wpFrames || t < wpFrames[u])) { const double g = (double) wp[((long) u * Tmax + t) * F + f]; y.x *= g; y.y *= g; }
  return make_float2((float) y.x, (float) y.y);
}

#define ST(e) (REG ? sr[REG ? (e) : 0] : P[(long) (e) * S])

// SubbandBeamformerGriffithsJim.__iter__ (:1023-1084) for bins 0..fftLen/2.  State: the active weights waHK (entries 0..n-1) and subBandSigmaK (entry n).
template <int CT, bool REG, int CAP>
__global__ __launch_bounds__(64) void k_abf_gj(const float2* __restrict__ X, const double2* __restrict__ wq, const double2* __restrict__ B,
                                               double2* __restrict__ work, float2* __restrict__ Y, double2* __restrict__ wOut, int U, int Crt, int Tmax,
                                               int F, double beta, double floorSb, double alpha2, double sb0, int ldsState,
                                               const int* __restrict__ nframesArr, const int* __restrict__ start, const double* __restrict__ gam,
                                               const float* __restrict__ wp, const int* __restrict__ wpFrames, double2* __restrict__ carry, int carryIn,
                                               int carryOut)
{
  const int C = CT ? CT : Crt, n = C - 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const long tix = (long) blockIdx.x * blockDim.x + threadIdx.x, UF = (long) U * F;
  if (tix >= UF) return;
  const int u = (int) (tix / F), f = (int) (tix - (long) u * F);
  const long S = ldsState ? 64 : UF;
  double2* P = ldsState ? reinterpret_cast<double2*>(smem) + threadIdx.x : work + tix;
  constexpr int CA = CT ? CT : CAP;
  double2 x[CA], Z[CA];
  double2 sr[REG ? CA : 1];
  const float2* Xu = X + (long) u * C * Tmax * F; float2* Yu = Y + (long) u * Tmax * F;
  const double2* wqf = wq + (long) f * C; const double2* Bf = B + f;           // wq [F][C]; B [C][n][F]: the lanes of a wave read neighbouring bins
#pragma unroll
  for (int e = 0; e <= n; e++) ST(e) = carryIn ? carry[(long) e * UF + tix] : (e < n ? z2() : make_double2(sb0, 0.0));
  const int Tu = clampT(nframesArr, u, Tmax), k0 = start[u];
  for (int t = Tu; t < Tmax; t++) Yu[(long) t * F + f] = make_float2(0.f, 0.f);
  float2 xn[CA];                                                               // the next frame's snapshot, in flight while this one is worked on
  if (Tu > 0) {
#pragma unroll
    for (int c = 0; c < C; c++) xn[c] = Xu[((long) c * Tmax) * F + f];
  }
  for (int t = 0; t < Tu; t++) {
    double pw = 0.0; double2 yc = z2();
#pragma unroll
    for (int c = 0; c < C; c++) x[c] = make_double2((double) xn[c].x, (double) xn[c].y);
    if (t + 1 < Tu) {
#pragma unroll
      for (int c = 0; c < C; c++) xn[c] = Xu[((long) c * Tmax + t + 1) * F + f];
    }
#pragma unroll
    for (int c = 0; c < C; c++) {
      pw += abs2(x[c]); const double2 q = conj_mul(wqf[c], x[c]); yc.x += q.x; yc.y += q.y;
    }
#pragma unroll
    for (int j = 0; j < n; j++) {
      double2 a = z2();
#pragma unroll
      for (int c = 0; c < C; c++) { const double2 q = conj_mul(Bf[(long) (c * n + j) * F], x[c]); a.x += q.x; a.y += q.y; }
      Z[j] = a;
    }
    const double g = gam[(long) u * Tmax + t];
    if (g >= 0.0) {
      double2 epa = yc;
#pragma unroll
      for (int j = 0; j < n; j++) { const double2 q = cmul(ST(j), Z[j]); epa.x -= q.x; epa.y -= q.y; }
      double sb = k0 + t > 0 ? ST(n).x * beta + (1.0 - beta) * pw : pw;
      if (sb < floorSb) sb = floorSb;
      ST(n) = make_double2(sb, 0.0);
      const double ak = g / sb; double nr = 0.0;
#pragma unroll
      for (int j = 0; j < n; j++) {
        const double2 q = cmul_conj(epa, Z[j]), o = ST(j);
        const double2 w = make_double2(o.x + q.x * ak, o.y + q.y * ak); nr += abs2(w); ST(j) = w;
      }
      if (nr > alpha2) {
        const double ck = sqrt(alpha2 / nr);
#pragma unroll
        for (int j = 0; j < n; j++) { const double2 o = ST(j); ST(j) = make_double2(ck * o.x, ck * o.y); }
      }
    }
    double2 y = yc;
#pragma unroll
    for (int j = 0; j < n; j++) { const double2 q = cmul(ST(j), Z[j]); y.x -= q.x; y.y -= q.y; }
    Yu[(long) t * F + f] = abf_out(y, wp, wpFrames, u, t, Tmax, F, f);
  }
  if (carryOut) {
#pragma unroll
    for (int e = 0; e <= n; e++) carry[(long) e * UF + tix] = ST(e);
  }
  if (wOut) {
#pragma unroll
    for (int j = 0; j < n; j++) wOut[tix * n + j] = ST(j);
  }
}

// SubbandBeamformerMVDR.__iter__ (:1135-1165) and SubbandBeamformerMPDR.__iter__ with updateActiveWeight (:1210-1225, :1251-1265), bins 0..fftLen/2.
// Both average a Hermitian matrix of order m over the frames 0..end of the stream, M <- lambda M + (1 - lambda) a a^H (M = a a^H at frame 0), and
// solve (M + diagLoad I) s = r by a Cholesky factorisation and two triangular solves; no inverse is formed.
//   MVDR: m = C, a = x, r = v (the array manifold), w = s / (v^H s), output w^H x.
//   MPDR: m = C - 1, a = z = B^H x: M is R = B^H Sx B, and r is h = conj(wq^H Sx B), averaged like M from conj(wq^H x) z; wa = s,
//         output wq^H x - wa^H z = conj(x^H wq - (x^H B) wa).  (Propagating R and h instead of Sx is the same mathematics with fewer entries.)
// After frame `end` the weights stay and the rest of the stream is a plain apply (MPDR: of wq - B wa, formed once).
// State: the lower triangle of M (entries tri(i, j)), then MVDR: w [m]; MPDR: h [m], wa [m].  LF: the factor's lower triangle.
template <bool MPDR, int CT, bool REG, int CAP>
__global__ __launch_bounds__(64) void k_abf_smi(const float2* __restrict__ X, const double2* __restrict__ wq, const double2* __restrict__ B,
                                                double2* __restrict__ work, float2* __restrict__ Y, double2* __restrict__ wOut, int U, int Crt, int Tmax,
                                                int F, double lambda, double diagLoad, int end, int ldsState, const int* __restrict__ nframesArr,
                                                const int* __restrict__ start, const float* __restrict__ wp, const int* __restrict__ wpFrames,
                                                double2* __restrict__ carry, int carryIn, int carryOut)
{
  const int C = CT ? CT : Crt, n = C - 1, m = MPDR ? n : C;
  const int NT = m * (m + 1) / 2, NS = MPDR ? NT + 2 * m : NT + m;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const long tix = (long) blockIdx.x * blockDim.x + threadIdx.x, UF = (long) U * F;
  if (tix >= UF) return;
  const int u = (int) (tix / F), f = (int) (tix - (long) u * F);
  const long S = ldsState ? 64 : UF;
  double2* P = ldsState ? reinterpret_cast<double2*>(smem) + threadIdx.x : work + tix;
  // the factor: behind the state where the state is (LDS, memory); alone in LDS next to a register-resident state
  const long SF = (REG || ldsState) ? 64 : UF;
  double2* Lf = REG ? reinterpret_cast<double2*>(smem) + threadIdx.x : P + (long) NS * S;
#define LF(e) Lf[(long) (e) * SF]
  constexpr int CA = CT ? CT : CAP;
  constexpr int MT = CT ? (MPDR ? CT - 1 : CT) : 1;
  double2 x[CA], a[MPDR ? CA : 1], s[CA];
  double2 sr[REG ? MT * (MT + 1) / 2 + (MPDR ? 2 : 1) * MT : 1];
#define AV(i) (MPDR ? a[MPDR ? (i) : 0] : x[i])
  const float2* Xu = X + (long) u * C * Tmax * F; float2* Yu = Y + (long) u * Tmax * F;
  const double2* wqf = wq + (long) f * C; const double2* Bf = B + f;           // wq [F][C]; B [C][n][F]: the lanes of a wave read neighbouring bins
#pragma unroll
  for (int e = 0; e < NS; e++) ST(e) = carryIn ? carry[(long) e * UF + tix] : z2();
  const int Tu = clampT(nframesArr, u, Tmax), k0 = start[u];
  const double om = 1.0 - lambda;
  bool frozen = false;
  for (int t = Tu; t < Tmax; t++) Yu[(long) t * F + f] = make_float2(0.f, 0.f);
  float2 xn[CA];                                                               // the next frame's snapshot, in flight while this one is worked on
  if (Tu > 0) {
#pragma unroll
    for (int c = 0; c < C; c++) xn[c] = Xu[((long) c * Tmax) * F + f];
  }
  for (int t = 0; t < Tu; t++) {
    double2 yc = z2();
    const int k = k0 + t;
#pragma unroll
    for (int c = 0; c < C; c++) x[c] = make_double2((double) xn[c].x, (double) xn[c].y);
    if (t + 1 < Tu) {
#pragma unroll
      for (int c = 0; c < C; c++) xn[c] = Xu[((long) c * Tmax + t + 1) * F + f];
    }
    if (MPDR && k > end) {
      // frozen: the weights wq - B wa, formed once at the first frame past `end`, then a plain apply
      if (!frozen) {
#pragma unroll
        for (int c = 0; c < C; c++) {
          double2 v = wqf[c];
#pragma unroll
          for (int j = 0; j < n; j++) { const double2 q = cmul(Bf[(long) (c * n + j) * F], ST(NT + m + j)); v.x -= q.x; v.y -= q.y; }
          s[c] = v;
        }
        frozen = true;
      }
#pragma unroll
      for (int c = 0; c < C; c++) { const double2 q = conj_mul(s[c], x[c]); yc.x += q.x; yc.y += q.y; }
      Yu[(long) t * F + f] = abf_out(yc, wp, wpFrames, u, t, Tmax, F, f);
      continue;
    }
    if (MPDR) {
#pragma unroll
      for (int c = 0; c < C; c++) { const double2 q = conj_mul(wqf[c], x[c]); yc.x += q.x; yc.y += q.y; }
#pragma unroll
      for (int j = 0; j < n; j++) {
        double2 z = z2();
#pragma unroll
        for (int c = 0; c < C; c++) { const double2 q = conj_mul(Bf[(long) (c * n + j) * F], x[c]); z.x += q.x; z.y += q.y; }
        a[MPDR ? j : 0] = z;
      }
    }
    if (k <= end) {
      // the averaged matrix (and MPDR's right-hand side)
#pragma unroll
      for (int i = 0; i < m; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) {
          const double2 q = cmul_conj(AV(i), AV(j)), o = ST(tri(i, j));
          ST(tri(i, j)) = k == 0 ? q : make_double2(lambda * o.x + om * q.x, lambda * o.y + om * q.y);
        }
        if (MPDR) {
          const double2 q = cmul_conj(AV(i), yc), o = ST(NT + i);
          ST(NT + i) = k == 0 ? q : make_double2(lambda * o.x + om * q.x, lambda * o.y + om * q.y);
        }
      }
      // M + diagLoad I = L L^H, column by column
#pragma unroll
      for (int j = 0; j < m; j++) {
        double d = ST(tri(j, j)).x + diagLoad;
#pragma unroll
        for (int q = 0; q < j; q++) d -= abs2(LF(tri(j, q)));
        d = sqrt(d);
        LF(tri(j, j)) = make_double2(d, 0.0);
        const double rd = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < m; i++) {
          double2 v = ST(tri(i, j));
#pragma unroll
          for (int q = 0; q < j; q++) { const double2 p = cmul_conj(LF(tri(i, q)), LF(tri(j, q))); v.x -= p.x; v.y -= p.y; }
          LF(tri(i, j)) = make_double2(v.x * rd, v.y * rd);
        }
      }
      // L y = r, then L^H s = y
#pragma unroll
      for (int i = 0; i < m; i++) {
        double2 v = MPDR ? ST(NT + i) : wqf[i];
#pragma unroll
        for (int q = 0; q < i; q++) { const double2 p = cmul(LF(tri(i, q)), s[q]); v.x -= p.x; v.y -= p.y; }
        const double rd = 1.0 / LF(tri(i, i)).x;
        s[i] = make_double2(v.x * rd, v.y * rd);
      }
#pragma unroll
      for (int i = m - 1; i >= 0; i--) {
        double2 v = s[i];
#pragma unroll
        for (int q = i + 1; q < m; q++) { const double2 p = conj_mul(LF(tri(q, i)), s[q]); v.x -= p.x; v.y -= p.y; }
        const double rd = 1.0 / LF(tri(i, i)).x;
        s[i] = make_double2(v.x * rd, v.y * rd);
      }
      if (MPDR) {
#pragma unroll
        for (int i = 0; i < m; i++) ST(NT + m + i) = s[i];
      } else {
        double2 den = z2();
#pragma unroll
        for (int i = 0; i < m; i++) { const double2 q = conj_mul(wqf[i], s[i]); den.x += q.x; den.y += q.y; }
#pragma unroll
        for (int i = 0; i < m; i++) ST(NT + i) = gsl_div(s[i], den);
      }
    }
    double2 y = yc;
    if (MPDR) {
#pragma unroll
      for (int j = 0; j < m; j++) { const double2 q = cmul_conj(AV(j), ST(NT + m + j)); y.x -= q.x; y.y -= q.y; }
    } else {
#pragma unroll
      for (int c = 0; c < m; c++) { const double2 q = conj_mul(ST(NT + c), x[c]); y.x += q.x; y.y += q.y; }
    }
    Yu[(long) t * F + f] = abf_out(y, wp, wpFrames, u, t, Tmax, F, f);
  }
  if (carryOut) {
#pragma unroll
    for (int e = 0; e < NS; e++) carry[(long) e * UF + tix] = ST(e);
  }
  if (wOut) {
#pragma unroll
    for (int j = 0; j < m; j++) wOut[tix * m + j] = ST(NT + (MPDR ? m : 0) + j);
  }
}
#undef ST
#undef LF
#undef AV

// SubbandBeamformerDS / SubbandBeamformerGSC.__iter__ (:374-379, :577-592): Y = w^H x with the fixed w = wq (- B wa), times the post-filter weight
__global__ __launch_bounds__(256) void k_abf_static(const float2* __restrict__ X, const double2* __restrict__ W, float2* __restrict__ Y, int C, int Tmax,
                                                    int F, long total, const int* __restrict__ nframesArr, const float* __restrict__ wp,
                                                    const int* __restrict__ wpFrames)
{
  const long perUtt = (long) Tmax * F;
  for (long idx = (long) blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long) gridDim.x * blockDim.x) {
    const int u = (int) (idx / perUtt); const long r = idx - (long) u * perUtt; const int t = (int) (r / F), f = (int) (r - (long) t * F);
    if (t >= clampT(nframesArr, u, Tmax)) { Y[idx] = make_float2(0.f, 0.f); continue; }
    double2 y = z2();
    for (int c = 0; c < C; c++) {
      const float2 v = X[((long) u * C + c) * perUtt + r];
      const double2 q = conj_mul(W[f * C + c], make_double2((double) v.x, (double) v.y)); y.x += q.x; y.y += q.y;
    }
    Y[idx] = abf_out(y, wp, wpFrames, u, t, Tmax, F, f);
  }
}

}  // namespace

// The dispatch of abf_launch, in one place: the launch below switches on it and dsr_abf_path reports it.  A thread's state is stateN complex fp64
// entries, the sample-matrix kinds add factorN for the Cholesky factor (n = C - 1):
//   Griffiths-Jim  n + 1                 (waHK, subBandSigmaK)                           no factor
//   MVDR           C (C + 1) / 2 + C     (triangle of Sx, w)                             C (C + 1) / 2
//   MPDR           n (n + 1) / 2 + 2 n   (triangle of R, h, wa)                          n (n + 1) / 2
// State in registers for the channel counts with a compile-time instance (AbfCt), the factor then alone in LDS; else state and factor in LDS
// ([entry][lane]) when (stateN + factorN) x 16 B x 64 lanes fit 150 KB (MVDR: C <= 11, MPDR: C <= 11, Griffiths-Jim: every C <= 64); else in
// memory.  The vectors of a thread have room for 16 channels, or 64 above that.  DSR_ABF_NOREGS / DSR_ABF_MEMSTATE (set to anything) take the
// first / the first two residences out; both are read on every call.
using AbfCt = ints<4, 6, 8>;
AbfPath dsr::abf_path(int kind, int C)
{
  AbfPath r; const int n = C - 1, m = kind == DSR_ABF_MPDR ? n : C;
  r.stateN = kind == DSR_ABF_GJ ? n + 1 : kind == DSR_ABF_MVDR ? m * (m + 1) / 2 + m : m * (m + 1) / 2 + 2 * m;
  r.factorN = kind == DSR_ABF_GJ ? 0 : m * (m + 1) / 2;
  r.ct = has_value(AbfCt{}, C) ? C : 0;
  r.cap = C <= 16 ? 16 : 64;
  r.stateBytes = (size_t) (r.stateN + r.factorN) * 16 * 64;
  const bool lds = r.stateBytes <= 150 * 1024 && !getenv("DSR_ABF_MEMSTATE");
  const bool regs = getenv("DSR_ABF_NOREGS") == nullptr && r.ct != 0;
  r.residence = regs ? DSR_ABF_STATE_REGS : lds ? DSR_ABF_STATE_LDS : DSR_ABF_STATE_MEM;
  r.ldsBytes = regs ? (size_t) r.factorN * 16 * 64 : lds ? r.stateBytes : 0;
  return r;
}

void dsr::abf_launch(AbfState& s, const float* X, const int32_t* nframes, int U, int Tmax, const float* wp, const int32_t* wpFrames, float* Y,
                     double* wOut, hipStream_t st)
{
  const int C = s.C, F = s.M / 2 + 1, kind = s.kind;
  const long UF = (long) U * F;
  if (kind == DSR_ABF_DS || kind == DSR_ABF_GSC) {
    const long total = UF * Tmax; int gx = cdiv(total, 256 * 4); if (gx < 1) gx = 1; if (gx > 16384) gx = 16384;
    launch(k_abf_static, dim3(gx), dim3(256), 0, st, (const float2*) X, s.d_weff.p, (float2*) Y, C, Tmax, F, total, nframes, wp, wpFrames);
    return;
  }
  const AbfPath pa = abf_path(kind, C);
  const bool regs = pa.residence == DSR_ABF_STATE_REGS; const int ldsState = pa.residence == DSR_ABF_STATE_LDS ? 1 : 0;
  const bool gj = kind == DSR_ABF_GJ;
  // the carried state: one layout whatever the residence -- [entry][U x F] and [U][4]; every residence copies in at the start and out at the end
  const int carryIn = s.carry && s.haveState ? 1 : 0, carryOut = s.carry ? 1 : 0;
  if (carryIn && s.stateU != U)
    throw Error(DSR_E_CONSISTENCY, "AdaptiveBeamformer: the carried state holds %d streams, this call has %d (reset the state first)", s.stateU, U);
  if (s.carry) s.d_carry.reserve((size_t) UF * pa.stateN);
  s.d_utt.reserve((size_t) U * 4); s.d_start.reserve((size_t) U);
  s.d_work.reserve(pa.residence == DSR_ABF_STATE_MEM ? (size_t) UF * (pa.stateN + pa.factorN) : 16);
  if (gj) {
    s.d_sig.reserve((size_t) U * Tmax); s.d_gam.reserve((size_t) U * Tmax);
    launch(k_abf_power, dim3((unsigned) ((long) U * Tmax)), dim3(64), 0, st, (const float2*) X, s.d_sig.p, C, Tmax, F, s.M);
  }
  launch(k_abf_frames, dim3((unsigned) cdiv(U, 64)), dim3(64), 0, st, s.d_sig.p, s.d_gam.p, s.d_start.p, s.d_utt.p, nframes, U, Tmax, gj ? 1 : 0, s.p.gamma,
         s.p.initDiagLoad, s.p.beta, s.p.silThresh, s.p.staticAfter, carryIn);
  const dim3 grid((unsigned) ((UF + 63) / 64));
  auto go = [&](auto kernel) {
    if constexpr (std::is_same_v<decltype(kernel), decltype(&k_abf_gj<0, false, 16>)>)
      launch(kernel, grid, dim3(64), pa.ldsBytes, st, (const float2*) X, s.d_wq.p, s.d_B.p, s.d_work.p, (float2*) Y, (double2*) wOut, U, C, Tmax, F, s.p.beta,
             s.p.floorSb, s.p.alpha2, s.p.initDiagLoad, ldsState, nframes, s.d_start.p, s.d_gam.p, wp, wpFrames, s.d_carry.p, carryIn, carryOut);
    else
      launch(kernel, grid, dim3(64), pa.ldsBytes, st, (const float2*) X, s.d_wq.p, s.d_B.p, s.d_work.p, (float2*) Y, (double2*) wOut, U, C, Tmax, F, s.p.lambda,
             s.p.diagLoad, s.p.end, ldsState, nframes, s.d_start.p, wp, wpFrames, s.d_carry.p, carryIn, carryOut);
  };
  auto pick = [&](auto ct, auto reg, auto cap) {
    if (gj) go(k_abf_gj<ct(), reg(), cap()>);
    else if (kind == DSR_ABF_MVDR) go(k_abf_smi<false, ct(), reg(), cap()>);
    else go(k_abf_smi<true, ct(), reg(), cap()>);
  };
  using T = std::true_type; using Fa = std::false_type; using C16 = std::integral_constant<int, 16>;
  const bool launched = pa.ct != 0 ? for_value(AbfCt{}, pa.ct, [&](auto ct) { if (regs) pick(ct, T{}, C16{}); else pick(ct, Fa{}, C16{}); })
                                   : for_value(ints<16, 64>{}, pa.cap, [&](auto cap) { pick(std::integral_constant<int, 0>{}, Fa{}, cap); });
  if (!launched) throw Error(DSR_E_ERROR, "AdaptiveBeamformer: no kernel for kind %d, <%d, %d, %d>", kind, pa.ct, regs ? 1 : 0, pa.cap);
  if (s.carry) { s.haveState = true; s.stateU = U; }
}
