// csrc/k_beamform.hip -- the kernels of the subband beamformers, the RLS path pick and their launchers.  Weight design and the dsr_bf_*
// entries are host code in csrc/beamformer.cpp; csrc/beamformer.h holds the handle and declares what this file exports.
//
// The hot loop -- SnapShotArray::update + one zdotc per bin per frame (btk/beamformer/beamformer.cc:76-90, :2609-2631) -- is
// k_bf_apply: one thread per (frame, bin), channel spectra read coalesced along the bin axis from the
// [chan][frame][bin] layout the analysis kernel writes, weights staged in LDS.  k_gsc_rls: SubbandGSCRLS, below.
#include "launch.h"
#include "dev_math.h"
#include "beamformer.h"

namespace dsr {

// Y[u][t][f] = sum_c conj(w[f][c]) X[u][c][t][f]
__global__ __launch_bounds__(256) void k_bf_apply(const float2* __restrict__ X, const float2* __restrict__ W,
                                                  float2* __restrict__ Y, int C, int Tmax, int F, long perUtt /*Tmax*F*/)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* w = reinterpret_cast<float2*>(smem);
  for (int i = threadIdx.x; i < F * C; i += blockDim.x) w[i] = W[i];
  __syncthreads();
  const int u = blockIdx.y;
  const float2* Xu = X + (long) u * C * perUtt;
  float2* Yu = Y + (long) u * perUtt;
  for (long idx = (long) blockIdx.x * blockDim.x + threadIdx.x; idx < perUtt; idx += (long) gridDim.x * blockDim.x) {
    const int f = (int) (idx % F);
    float2 acc = make_float2(0.f, 0.f);
    for (int c = 0; c < C; c++) {
      const float2 x = Xu[(long) c * perUtt + idx];
      const float2 wc = w[f * C + c];
      acc.x += wc.x * x.x + wc.y * x.y;       // conj(w) * x
      acc.y += wc.x * x.y - wc.y * x.x;
    }
    Yu[idx] = acc;
  }
}

}  // namespace dsr

using namespace dsr;

// SubbandGSCRLS::next + _updateActiveWeightVector2 (beamformer.cc:1554-1698).  One thread owns one (utterance, bin) and walks the frames: the
// frame's output with the weights as they stand, then Z = B^H X, the gain vector, the precision matrix and the active weights (quadratic
// constraint optional), all fp64 in the reference's order of operations; precision matrix and active weights live in a state array
// [entry][utterance x bin] (coalesced across the threads of a wave).  Every utterance starts from P0 and wa = 0.

// (CT: compile-time channel count -- the small vectors then live in registers and the loops unroll; 0: run-time count, arrays in scratch)
// nframesArr (optional): utterance u is adapted over its first nframesArr[u] frames only and the rest of its rows is zero filled -- the reference
// stops at the stream's last frame (beamformer.cc:1552-1612); adapting on zero-padded frames would still scale P by 1/myu and wa by (I - sigma2 P).
// carry (optional, [entry][U x F]): start from / leave the adaptation state there instead of P0 and wa = 0 (carryIn) / nowhere (carryOut).
// CA: capacity of the per-thread vectors for the run-time channel count (16, or 64 for the large arrays of BASELINE configs[4]; those live in scratch).
template <int CT, bool REG, int CAP>
__global__ __launch_bounds__(64) void k_gsc_rls(const float2* __restrict__ X, const double2* __restrict__ wq, const double2* __restrict__ B,
                                                const double2* __restrict__ P0, const double* __restrict__ diagW, double2* __restrict__ state,
                                                float2* __restrict__ Y, double2* __restrict__ waOut, int U, int Crt, int Tmax, int F, double rmu,
                                                double alpha, int qctype, int adapt, int normalize, int ldsState,
                                                const int* __restrict__ nframesArr, double2* __restrict__ carry, int carryIn, int carryOut)
{
  const int C = CT ? CT : Crt;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const long tix = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (tix >= (long) U * F) return;
  const int u = (int) (tix / F), f = (int) (tix - (long) u * F), n = C - 1;
  // the adaptation state of a thread, entry e at P[e * S]: in LDS ([entry][lane], conflict free) when (n^2 + n) x 16 B x 64 lanes fit, else in memory
  const long S = ldsState ? 64 : (long) U * F;
  const float2* Xu = X + (long) u * C * Tmax * F; float2* Yu = Y + (long) u * Tmax * F;
  const double2* wqf = wq + (long) f * C; const double2* Bf = B + (long) f * C * n;
  double2* P = ldsState ? reinterpret_cast<double2*>(smem) + threadIdx.x : state + tix; double2* wa = P + (long) n * n * S;
  constexpr int CA = CT ? CT : CAP;
  double2 x[CA], w[CA], Z[CA], PH[CA], g[CA], wn[CA];
  // REG (needs CT): precision matrix and active weights in registers -- every index below is a compile-time constant after unrolling
  double2 Pr[REG ? CA : 1][REG ? CA : 1], war[REG ? CA : 1];
#define PX(i, j) (REG ? Pr[REG ? (i) : 0][REG ? (j) : 0] : P[(long) ((i) * n + (j)) * S])
#define WA(j) (REG ? war[REG ? (j) : 0] : wa[(long) (j) * S])
  const long SC = (long) U * F;                                   // the carried state's entry pitch
  if (f > 0) {
    for (int i = 0; i < n; i++) {
      for (int j = 0; j < n; j++) PX(i, j) = carryIn ? carry[(long) (i * n + j) * SC + tix] : P0[(long) f * n * n + i * n + j];
      WA(i) = carryIn ? carry[(long) (n * n + i) * SC + tix] : make_double2(0.0, 0.0);
    }
  }
  const double dw = diagW[f];
  const int Tu = nframesArr ? (nframesArr[u] < Tmax ? nframesArr[u] : Tmax) : Tmax;
  for (int t = Tu; t < Tmax; t++) Yu[(long) t * F + f] = make_float2(0.f, 0.f);
  for (int t = 0; t < Tu; t++) {
    for (int c = 0; c < C; c++) { const float2 v = Xu[((long) c * Tmax + t) * F + f]; x[c] = make_double2((double) v.x, (double) v.y); }
    double2 y = make_double2(0.0, 0.0);
    if (f == 0) { for (int c = 0; c < C; c++) { const double2 q = cmul_conj(x[c], wqf[c]); y.x += q.x; y.y += q.y; } }
    else {
      double nrm = 0.0;
      for (int i = 0; i < C; i++) {
        double2 wl = make_double2(0.0, 0.0);
        for (int j = 0; j < n; j++) { const double2 q = cmul(Bf[i * n + j], WA(j)); wl.x += q.x; wl.y += q.y; }
        w[i] = make_double2(wqf[i].x - wl.x, wqf[i].y - wl.y); nrm += w[i].x * w[i].x + w[i].y * w[i].y;
      }
      if (normalize) { nrm = sqrt(nrm) * (double) C; for (int i = 0; i < C; i++) { w[i].x /= nrm; w[i].y /= nrm; } }
      for (int c = 0; c < C; c++) { const double2 q = cmul_conj(x[c], w[c]); y.x += q.x; y.y += q.y; }
    }
    Yu[(long) t * F + f] = make_float2((float) y.x, (float) y.y);
    if (f == 0 || !adapt) continue;
    for (int j = 0; j < n; j++) { double2 a = make_double2(0.0, 0.0); for (int c = 0; c < C; c++) { const double2 q = cmul_conj(x[c], Bf[c * n + j]); a.x += q.x; a.y += q.y; } Z[j] = a; }
    for (int j = 0; j < n; j++) { double2 a = make_double2(0.0, 0.0); for (int i = 0; i < n; i++) { const double2 q = cmul_conj(Z[i], PX(i, j)); a.x += q.x; a.y += q.y; } PH[j] = a; }
    for (int i = 0; i < n; i++) { double2 a = make_double2(0.0, 0.0); for (int j = 0; j < n; j++) { const double2 q = cmul(PX(i, j), Z[j]); a.x += q.x; a.y += q.y; } g[i] = make_double2(a.x * rmu, a.y * rmu); }
    double2 de = make_double2(0.0, 0.0);
    for (int j = 0; j < n; j++) { const double2 q = cmul_conj(Z[j], PH[j]); de.x += q.x; de.y += q.y; }
    de = make_double2(de.x * rmu + 1.0, de.y * rmu);
    for (int i = 0; i < n; i++) g[i] = gsl_div(g[i], de);
    for (int i = 0; i < n; i++)
      for (int j = 0; j < n; j++) {
        const double2 o = PX(i, j), q = cmul_conj(g[i], PH[j]);
        PX(i, j) = make_double2((o.x - q.x) * rmu, (o.y - q.y) * rmu);
      }
    const double2 epA = make_double2(y.x, -y.y);
    for (int i = 0; i < n; i++) {
      double2 a = make_double2(0.0, 0.0);
      for (int j = 0; j < n; j++) {
        const double2 p = PX(i, j); double2 m1 = make_double2(p.x * (-dw), p.y * (-dw)); if (i == j) m1.x += 1.0;
        const double2 q = cmul(m1, WA(j)); a.x += q.x; a.y += q.y;
      }
      const double2 q = cmul(g[i], epA); wn[i] = make_double2(a.x + q.x, a.y + q.y);
    }
    if (qctype == 1 || qctype == 2) {
      double nr = 0.0; for (int i = 0; i < n; i++) nr += wn[i].x * wn[i].x + wn[i].y * wn[i].y;
      nr = sqrt(nr);
      if (qctype == 1 || nr * nr >= alpha) { const double sc = alpha / nr; for (int i = 0; i < n; i++) { wn[i].x *= sc; wn[i].y *= sc; } }
    }
    for (int i = 0; i < n; i++) WA(i) = wn[i];
  }
  if (carryOut && f > 0)
    for (int i = 0; i < n; i++) {
      for (int j = 0; j < n; j++) carry[(long) (i * n + j) * SC + tix] = PX(i, j);
      carry[(long) (n * n + i) * SC + tix] = WA(i);
    }
  if (waOut && f > 0) for (int j = 0; j < n; j++) waOut[((long) u * F + f) * n + j] = WA(j);
  if (waOut && f == 0) for (int j = 0; j < n; j++) waOut[((long) u * F) * n + j] = make_double2(0.0, 0.0);
}
#undef PX
#undef WA

// The dispatch of bf_launch_rls, in one place: the launch below switches on it and dsr_bf_rls_path reports it.  n = C - 1; the precision matrix and the
// active weights of a thread are n^2 + n complex fp64 values: in registers for the channel counts k_gsc_rls is instantiated for with a compile-time
// count (RlsCt), else in LDS ([entry][lane]) when the 64 lanes' values fit 150 KB (C <= 12), else in memory, in place.  The vectors of a thread
// have room for 16 channels, or 64 above that.  DSR_RLS_NOREGS / DSR_RLS_MEMSTATE (set to anything) take the first / the first two residences out;
// both are read on every call.
using RlsCt = ints<4, 6, 8>;
RlsPath dsr::rls_path(int C)
{
  RlsPath r; const int n = C - 1;
  r.ct = has_value(RlsCt{}, C) ? C : 0;
  r.cap = C <= 16 ? 16 : 64;
  r.stateBytes = (size_t) (n * n + n) * 16 * 64;
  const bool lds = r.stateBytes <= 150 * 1024 && !getenv("DSR_RLS_MEMSTATE");
  const bool regs = getenv("DSR_RLS_NOREGS") == nullptr && r.ct != 0;
  r.residence = regs ? DSR_RLS_STATE_REGS : lds ? DSR_RLS_STATE_LDS : DSR_RLS_STATE_MEM;
  r.ldsBytes = r.residence == DSR_RLS_STATE_LDS ? r.stateBytes : 0;
  return r;
}

void dsr::bf_launch_rls(BfState& s, const float* X, const int32_t* nframes, int U, int Tmax, float* Y, double* waOut, hipStream_t st)
{
  const int C = s.C, n = C - 1, F = s.M / 2 + 1;
  const long S = (long) U * F;
  const RlsPath pa = rls_path(C);
  const size_t ldsB = pa.stateBytes; const int ldsState = pa.residence == DSR_RLS_STATE_LDS ? 1 : 0;
  const bool regs = pa.residence == DSR_RLS_STATE_REGS;        // precision matrix + active weights in registers (C = 8: 256 VGPRs, no scratch)
  // carried state: its own array (the register / LDS variants copy in and out; the memory variant works in it directly)
  int carryIn = 0, carryOut = 0; double2* carry = nullptr;
  if (s.rlsCarry) {
    if (s.rlsHaveState && s.rlsStateU != U) throw Error(DSR_E_CONSISTENCY, "SubbandGSCRLS: the carried state holds %d streams, this call has %d (reset the state first)", s.rlsStateU, U);
    s.d_carry.reserve((size_t) S * (n * n + n));
    carry = s.d_carry.p; carryIn = s.rlsHaveState ? 1 : 0; carryOut = 1;
  }
  const bool memInPlace = !regs && !ldsState;                   // state array == working array
  if (memInPlace && !s.rlsCarry) s.d_state.reserve((size_t) S * (n * n + n));
  double2* work = memInPlace ? (s.rlsCarry ? s.d_carry.p : s.d_state.p) : (s.d_state.reserve(16), s.d_state.p);
  // in-place memory variant with carry: the working array IS the carried one: reading "carry" at start and writing it at the end are no-ops on the
  // same addresses (same [entry][U x F] layout), so the flags are passed as they are.
  auto go = [&](auto kernel) {
    launch(kernel, dim3((unsigned) ((S + 63) / 64)), dim3(64), ldsState ? ldsB : 0, st, (const float2*) X, s.d_wq.p, s.d_B.p, s.d_P0.p, s.d_diag.p, work, (float2*) Y,
           (double2*) waOut, U, C, Tmax, F, 1.0 / s.rlsMyu, s.rlsAlpha, s.rlsQc, s.rlsAdapt ? 1 : 0, s.mode == 3 ? 1 : 0, ldsState, nframes, carry, carryIn, carryOut);
  };
  const bool launched = pa.ct != 0 ? for_value(RlsCt{}, pa.ct, [&](auto ct) { if (regs) go(k_gsc_rls<ct(), true, 16>); else go(k_gsc_rls<ct(), false, 16>); })
                                   : for_value(ints<16, 64>{}, pa.cap, [&](auto cap) { go(k_gsc_rls<0, false, cap()>); });
  if (!launched) throw Error(DSR_E_ERROR, "SubbandGSCRLS: no kernel k_gsc_rls<%d, %d, %d>", pa.ct, regs ? 1 : 0, pa.cap);
  if (s.rlsCarry) { s.rlsHaveState = true; s.rlsStateU = U; }
}

void dsr::bf_launch_apply(const float* X, const float2* W, int C, int F, int U, int Tmax, float* Y, hipStream_t st)
{
  const long perUtt = (long) Tmax * F; const size_t lds = sizeof(float2) * (size_t) F * C;
  int gx = cdiv(perUtt, 256 * 4); if (gx < 1) gx = 1; if (gx > 4096) gx = 4096;
  launch(k_bf_apply, dim3(gx, U), dim3(256), lds, st, (const float2*) X, W, (float2*) Y, C, Tmax, F, perUtt);
}
