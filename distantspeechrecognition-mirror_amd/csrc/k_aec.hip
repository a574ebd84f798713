// csrc/k_aec.hip -- subband acoustic echo (voice prompt) cancellation, include/dsr.h section 2d.
//
// Restates four operators of btk/cancelVP/cancelVP.{h,cc}: NLMSAcousticEchoCancellationFeature (cancelVP.cc:57-104),
// KalmanFilterEchoCancellationFeature (:141-209), BlockKalmanFilterEchoCancellationFeature (:287-383) and
// DTDBlockKalmanFilterEchoCancellationFeature (:1077-1198).  Every (utterance, bin) pair is a chain of T dependent steps in fp64.
//
// Three kernels:
//   k_aec_scalar  NLMS / Kalman: one thread per chain, bins fastest, so a wave's loads and stores are contiguous.
//   k_aec_block   block Kalman: LPC lanes per chain, the L x L covariance spread over their registers (row-contiguous chunks of CH entries),
//                 row sums by butterfly shuffles, the played history shifted through registers.  sampleN = 1 is the same kernel with one
//                 lane per chain, i.e. a thread per chain.
//   k_aec_dtd     the double-talk variant: its three smoothed scalars couple the bins of a frame, so one workgroup owns one utterance and
//                 walks the frames with three barriers each; the covariances stay in the caller's state between frames.
// The covariance update is the rank-1 form K = K- - s s^H / sigma2_s with s = K- conj(v): K stays exactly Hermitian (s_i conj(s_j) and
// s_j conj(s_i) are exact conjugates without FMA contraction), so v^T K- = s^H needs no second reduction.
// The two information filters of the same directory are k_aec_info.hip; the C entries at the end of this file hand their kinds on (aec.h).
#include "launch.h"
#include "dev_math.h"
#include "aec.h"

using namespace dsr;

namespace {

struct Par { double delta, epsilon, threshold, beta, su, amp, engTh, smooth; };
struct St { double2* R; double2* K; double* sv; double2* H; double* dtd; };
struct Layout { size_t oR, oK, oSv, oH, oD, bytes; };

Layout layout(const dsr_aec& a, int U)
{
  const size_t n = (size_t) U * (a.M / 2 + 1), L = (size_t) a.L; Layout l;
  l.oR = 0; l.oK = l.oR + n * L * 16; l.oSv = l.oK + n * L * L * 16; l.oH = l.oSv + n * 8; l.oD = l.oH + n * L * 16; l.bytes = l.oD + (size_t) U * 4 * 8;
  return l;
}
St carve(const dsr_aec& a, void* base, int U)
{
  const Layout l = layout(a, U); char* b = (char*) base;
  return St{(double2*) (b + l.oR), (double2*) (b + l.oK), (double*) (b + l.oSv), (double2*) (b + l.oH), (double*) (b + l.oD)};
}

// butterfly sum over W consecutive lanes (W a power of two): every lane ends with the same bits, because x + y == y + x
template <int W> __device__ __forceinline__ double bsum(double x)
{
#pragma unroll
  for (int o = W / 2; o >= 1; o >>= 1) x += __shfl_xor(x, o);
  return x;
}
template <int W> __device__ __forceinline__ double2 bsum2(double2 a) { return make_double2(bsum<W>(a.x), bsum<W>(a.y)); }

__global__ void k_aec_init(St s, long nChain, int L, int U, double k0, double sv0)
{
  const long c = (long) blockIdx.x * 256 + threadIdx.x;
  if (c < (long) U * 4) s.dtd[c] = 0.0;
  if (c >= nChain) return;
  s.sv[c] = sv0;
  for (int i = 0; i < L; i++) {
    s.R[c * L + i] = make_double2(0.0, 0.0); s.H[c * L + i] = make_double2(0.0, 0.0);
    for (int j = 0; j < L; j++) s.K[(c * L + i) * L + j] = make_double2(i == j ? k0 : 0.0, 0.0);
  }
}

// ---- NLMS (KIND 0, cancelVP.cc:68-100) and scalar Kalman (KIND 1, :152-205): a thread per chain --------------------------------------------
template <int KIND> __global__ __launch_bounds__(256) void k_aec_scalar(const float2* __restrict__ V, const float2* __restrict__ A, const int* __restrict__ nf,
                                                                       int U, int Tmax, int F, Par p, St s, float2* __restrict__ out)
{
  const long c = (long) blockIdx.x * 256 + threadIdx.x;
  if (c >= (long) U * F) return;
  const int u = (int) (c / F), f = (int) (c % F);
  int T = nf ? nf[u] : Tmax; T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  double2 R = s.R[c]; double sv = s.sv[c], K = s.K[c].x;
  const size_t base = (size_t) u * Tmax * F + f;
  float2 vn = make_float2(0.f, 0.f), an = vn;
  if (T > 0) { vn = V[base]; an = A[base]; }
  for (int t = 0; t < T; t++) {
    const double2 Vk = make_double2(vn.x, vn.y), Ak = make_double2(an.x, an.y);
    if (t + 1 < T) { vn = V[base + (size_t) (t + 1) * F]; an = A[base + (size_t) (t + 1) * F]; }      // the next frame's loads ahead of the dependent step
    const double2 RV = cmul(R, Vk), Ek = make_double2(Ak.x - RV.x, Ak.y - RV.y);
    out[base + (size_t) t * F] = make_float2((float) Ek.x, (float) Ek.y);
    const double Vk2 = abs2(Vk);
    if (Vk2 > p.threshold) {
      if (KIND == 0) {
        const double2 Gh = gsl_div(Ak, Vk), dC = make_double2(R.x - Gh.x, R.y - Gh.y);
        const double w = p.epsilon * Vk2 / (p.delta + abs2(Ak));
        R = make_double2(R.x - dC.x * w, R.y - dC.y * w);
      } else {
        sv = p.beta * sv + (1.0 - p.beta) * abs2(Ek);
        const double Kp = K + p.su, sig = Vk2 * Kp + sv, g = Kp / sig;
        const double2 Gk = make_double2(Vk.x * g, -Vk.y * g), GE = cmul(Gk, Ek);
        R = make_double2(R.x + GE.x, R.y + GE.y);
        K = (1.0 - Kp * Vk2 / sig) * Kp;
      }
    }
  }
  for (int t = T; t < Tmax; t++) out[base + (size_t) t * F] = make_float2(0.f, 0.f);
  s.R[c] = R; s.sv[c] = sv; s.K[c] = make_double2(K, 0.0);
}

// ---- the block Kalman step shared by k_aec_block and k_aec_dtd ----------------------------------------------------------------------------
// LP = sampleN rounded up to a power of two.  A chain's LP x LP covariance is cut into row-contiguous chunks of CH entries, one per lane:
//   LP   32  16   8   4   2   1
//   CH   16   4   1   1   1   1     entries (complex fp64) per lane: 64 / 16 / 4 VGPRs
//   LPR   2   4   8   4   2   1     lanes per row
//   LPC  64  64  64  16   4   1     lanes per chain  -> 64 / LPC chains per wave
// Rows and columns from sampleN on hold zeros and stay zero.
template <int LP> struct Geo {
  static constexpr int CH = LP * LP >= 64 ? LP * LP / 64 : 1, LPR = LP / CH, LPC = LP * LPR, CPW = 64 / LPC;
};

template <int LP> __device__ __forceinline__ double2 aec_residual(double2 Rrow, double2 vrow, bool leader, double2 Ak)
{
  const double2 pr = leader ? cmul(Rrow, vrow) : make_double2(0.0, 0.0), dot = bsum2<Geo<LP>::LPC>(pr);       // zdotu(Rk, Vk) (:306)
  return make_double2(Ak.x - dot.x, Ak.y - dot.y);
}

// One update (cancelVP.cc:321-354, :1163-1193) of the lanes' chunk; suS = Sigma_u's diagonal (times sf for DTD).  Every lane runs it (the
// shuffles need all of a chain's lanes); the caller keeps the results of the chains that adapt.
template <int LP> __device__ __forceinline__ void aec_update(double2 (&K)[Geo<LP>::CH], double2& Rrow, double& sv, const double2 (&vcol)[Geo<LP>::CH], double2 vrow,
                                                            double2 Ek, double suS, double beta, int row, int col0, int L, bool leader, int chainBase)
{
  constexpr int CH = Geo<LP>::CH, LPR = Geo<LP>::LPR, LPC = Geo<LP>::LPC;
  sv = beta * sv + (1.0 - beta) * abs2(Ek);
  double2 s = make_double2(0.0, 0.0);
#pragma unroll
  for (int c = 0; c < CH; c++) {
    if (row == col0 + c && row < L) K[c].x = suS + K[c].x;                           // K- = Sigma_u + K (:326-327)
    const double2 pr = cmul_conj(K[c], vcol[c]); s.x += pr.x; s.y += pr.y;               // s = K- conj(v) (:329-330)
  }
  s = bsum2<LPR>(s);
  const double sig = bsum<LPC>(leader ? vrow.x * s.x - vrow.y * s.y : 0.0) + sv;     // sigma2_s = Re(v^T s) + sigma2_v (:331-338)
  const double inv = 1.0 / sig;
  const double2 G = make_double2(inv * s.x, inv * s.y), EG = cmul(Ek, G);            // G = s / sigma2_s, R += E G (:339-343)
  Rrow = make_double2(Rrow.x + EG.x, Rrow.y + EG.y);
#pragma unroll
  for (int c = 0; c < CH; c++) {                                                     // K = (I - G v^T) K- = K- - s s^H / sigma2_s (:346-354)
    const double2 sc = shfl2(s, chainBase + (col0 + c) * LPR), P = cmul_conj(s, sc);
    K[c] = make_double2(K[c].x - P.x * inv, K[c].y - P.y * inv);
  }
}

template <int LP> __global__ __launch_bounds__(64) void k_aec_block(const float2* __restrict__ V, const float2* __restrict__ A, const int* __restrict__ nf,
                                                                    int U, int Tmax, int F, int L, Par p, St s, float2* __restrict__ out)
{
  constexpr int CH = Geo<LP>::CH, LPR = Geo<LP>::LPR, LPC = Geo<LP>::LPC, CPW = Geo<LP>::CPW;
  const int lane = threadIdx.x, q = lane % LPC, row = q / LPR, col0 = (q % LPR) * CH, chainBase = lane - q;
  const bool leader = (q % LPR) == 0;
  const long chain = (long) blockIdx.x * CPW + lane / LPC;
  const bool valid = chain < (long) U * F;
  const int u = valid ? (int) (chain / F) : 0, f = valid ? (int) (chain % F) : 0;
  int T = valid ? (nf ? nf[u] : Tmax) : 0; T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  int Tw = T;
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const int x = __shfl_xor(Tw, o); Tw = x > Tw ? x : Tw; }
  double2 K[CH], vcol[CH];                                                           // vcol: the previous frame's history, shifted at every frame
#pragma unroll
  for (int c = 0; c < CH; c++) {
    const bool in = valid && row < L && col0 + c < L;
    K[c] = in ? s.K[((size_t) chain * L + row) * L + col0 + c] : z2();
    vcol[c] = (valid && col0 + c < L) ? s.H[(size_t) chain * L + col0 + c] : z2();
  }
  const bool rowIn = valid && row < L;
  double2 Rrow = rowIn ? s.R[(size_t) chain * L + row] : z2(), vrow = rowIn ? s.H[(size_t) chain * L + row] : z2();
  double sv = valid ? s.sv[chain] : 1.0;
  const size_t base = (size_t) u * Tmax * F + f;
  float2 vn = make_float2(0.f, 0.f), an = vn;
  if (T > 0) { vn = V[base]; an = A[base]; }
  for (int t = 0; t < Tw; t++) {
    const bool act = t < T;
    const double2 nv = make_double2(p.amp * (double) vn.x, p.amp * (double) vn.y), Ak = make_double2(an.x, an.y);      // nextSample(playBlock, amp4play) (:297)
    if (t + 1 < T) { vn = V[base + (size_t) (t + 1) * F]; an = A[base + (size_t) (t + 1) * F]; }                     // the next frame's loads ahead of the dependent step
    // v[j] <- v[j-1], v[0] <- the new sample: inside the chunk by register moves, across chunks and rows by one shuffle each
    double2 cin = shfl2(vcol[CH - 1], lane - 1), rin = shfl2(vrow, lane - LPR);
    if (leader) cin = nv;
    if (row == 0) rin = nv;
    if (act) {
#pragma unroll
      for (int c = CH - 1; c >= 1; c--) vcol[c] = col0 + c < L ? vcol[c - 1] : z2();
      vcol[0] = col0 < L ? cin : z2();
      vrow = row < L ? rin : z2();
    }
    const double2 Ek = aec_residual<LP>(Rrow, vrow, leader, Ak);
    if (act && q == 0) out[base + (size_t) t * F] = make_float2((float) Ek.x, (float) Ek.y);
    const bool upd = act && abs2(nv) > p.threshold;                                  // _update: |v[0]|^2 > threshold (:270-275)
    if (CPW == 1) {                                                                  // one chain per wave: the gate is wave-uniform, update in place
      if (upd) aec_update<LP>(K, Rrow, sv, vcol, vrow, Ek, p.su, p.beta, row, col0, L, leader, chainBase);
    } else if (__any(upd)) {                                                         // several chains per wave (CH = 1): all lanes run, the adapting chains keep
      double2 Kn[CH]; double2 Rn = Rrow; double svn = sv;
#pragma unroll
      for (int c = 0; c < CH; c++) Kn[c] = K[c];
      aec_update<LP>(Kn, Rn, svn, vcol, vrow, Ek, p.su, p.beta, row, col0, L, leader, chainBase);
      if (upd) {
#pragma unroll
        for (int c = 0; c < CH; c++) K[c] = Kn[c];
        Rrow = Rn; sv = svn;
      }
    }
  }
  if (!valid) return;
  if (q == 0) { for (int t = T; t < Tmax; t++) out[base + (size_t) t * F] = make_float2(0.f, 0.f); s.sv[chain] = sv; }
#pragma unroll
  for (int c = 0; c < CH; c++) if (row < L && col0 + c < L) s.K[((size_t) chain * L + row) * L + col0 + c] = K[c];
  if (leader && row < L) { s.R[(size_t) chain * L + row] = Rrow; s.H[(size_t) chain * L + row] = vrow; }
}

// ---- DTD: one workgroup per utterance -----------------------------------------------------------------------------------------------------
// Per frame: (A) every bin's residual, as the reference's first loop (:1134-1146), with the three per-bin inputs of _updateBand; (B) lanes
// 0..2 walk the bins in order, one smoothed scalar each (_EkEnergy, _SkEnergy, _snr: three independent recurrences, :1093-1096); (C) the
// bins that adapt update in parallel.  Nothing waits on another workgroup.
// 512 threads a workgroup; 256 at LP = 32, whose 64 covariance registers a lane plus the step's temporaries do not fit 256 VGPRs
template <int LP> struct DtdNT { static constexpr int v = LP >= 32 ? 256 : 512; };

template <int LP> __global__ __launch_bounds__(DtdNT<LP>::v) void k_aec_dtd(const float2* __restrict__ V, const float2* __restrict__ A, const int* __restrict__ nf,
                                                                      int U, int Tmax, int F, int L, Par p, St s, float2* __restrict__ out, int frame0, int mode)
{
  constexpr int CH = Geo<LP>::CH, LPR = Geo<LP>::LPR, LPC = Geo<LP>::LPC, CPW = Geo<LP>::CPW, DTD_NT = DtdNT<LP>::v, NW = DTD_NT / 64;
  extern __shared__ double lds[];
  double* in3 = lds;                       // [3][F]: |E|^2, |A - E|^2, their ratio
  double* sm3 = lds + 3 * (size_t) F;      // [3][F]: the three scalars after bin f
  double2* Eb = (double2*) (lds + 6 * (size_t) F);
  const int u = blockIdx.x, tid = threadIdx.x, wave = tid / 64, lane = tid % 64;
  const int q = lane % LPC, row = q / LPR, col0 = (q % LPR) * CH, chainBase = lane - q;
  const bool leader = (q % LPR) == 0;
  int T = nf ? nf[u] : Tmax; T = T < 0 ? 0 : (T > Tmax ? Tmax : T);
  const int nGroups = (F + CPW - 1) / CPW;
  double x = tid < 3 ? s.dtd[(size_t) u * 4 + tid] : 0.0;
  const size_t ubase = (size_t) u * Tmax * F;
  // the played sample j frames before frame t, scaled: this call's frames, before them the carried history
  auto getv = [&](int f, int j, int t) -> double2 {
    const int tt = t - j;
    if (tt >= 0) { const float2 v = V[ubase + (size_t) tt * F + f]; return make_double2(p.amp * (double) v.x, p.amp * (double) v.y); }
    return s.H[((size_t) u * F + f) * L + (-tt - 1)];
  };
  for (int t = 0; t < T; t++) {
    const int frameX = mode == 0 ? frame0 + t : -5;
    const double smth = frameX < 100 ? 1.0 - (double) frameX * (1.0 - p.smooth) / 100.0 : p.smooth;      // :1081-1087
    for (int g0 = 0; g0 < nGroups; g0 += NW) {
      const int f = (g0 + wave) * CPW + lane / LPC; const bool valid = f < F, rowIn = valid && row < L;
      const double2 vrow = rowIn ? getv(f, row, t) : z2(), Rrow = rowIn ? s.R[((size_t) u * F + f) * L + row] : z2();
      float2 a = make_float2(0.f, 0.f); if (valid) a = A[ubase + (size_t) t * F + f];
      const double2 Ak = make_double2(a.x, a.y), Ek = aec_residual<LP>(Rrow, vrow, leader, Ak);
      if (valid && q == 0) {
        out[ubase + (size_t) t * F + f] = make_float2((float) Ek.x, (float) Ek.y);
        const double2 Sk = make_double2(Ak.x - Ek.x, Ak.y - Ek.y); const double ce = abs2(Ek), cs = abs2(Sk);
        Eb[f] = Ek; in3[f] = ce; in3[F + f] = cs; in3[2 * (size_t) F + f] = cs / (ce + 1.0e-15);
      }
    }
    __syncthreads();
    if (tid < 3) {
      const double* src = in3 + (size_t) tid * F; double* dst = sm3 + (size_t) tid * F;
      for (int f = 0; f < F; f++) { x = src[f] * smth + x * (1.0 - smth); dst[f] = x; }
    }
    __syncthreads();
    for (int g0 = 0; g0 < nGroups; g0 += NW) {
      const int f = (g0 + wave) * CPW + lane / LPC; const bool valid = f < F;
      double sf = -1.0;
      if (valid) {
        const double snr = sm3[2 * (size_t) F + f], sk = sm3[F + f];
        if (frameX < 100 || (snr > p.threshold && sk > p.engTh)) sf = 2.0 / (1.0 + exp(-snr)) - 1.0;      // :1097-1100
      }
      const bool upd = valid && !(sf < 0.0);
      if (!__any(upd)) continue;
      const size_t chain = (size_t) u * F + (valid ? f : 0);
      double2 K[CH], vcol[CH];
#pragma unroll
      for (int c = 0; c < CH; c++) {
        const bool in = upd && row < L && col0 + c < L;
        K[c] = in ? s.K[(chain * L + row) * L + col0 + c] : z2();
        vcol[c] = (upd && col0 + c < L) ? getv(f, col0 + c, t) : z2();
      }
      const bool rowIn = upd && row < L;
      double2 Rrow = rowIn ? s.R[chain * L + row] : z2(); const double2 vrow = rowIn ? getv(f, row, t) : z2();
      double sv = upd ? s.sv[chain] : 1.0;
      const double2 Ek = upd ? Eb[f] : z2();
      aec_update<LP>(K, Rrow, sv, vcol, vrow, Ek, p.su * sf, p.beta, row, col0, L, leader, chainBase);      // Sigma_u scaled by sf (:1169-1171)
      if (upd) {
#pragma unroll
        for (int c = 0; c < CH; c++) if (row < L && col0 + c < L) s.K[(chain * L + row) * L + col0 + c] = K[c];
        if (leader && row < L) s.R[chain * L + row] = Rrow;
        if (q == 0) s.sv[chain] = sv;
      }
    }
    __syncthreads();
  }
  if (tid < 3) s.dtd[(size_t) u * 4 + tid] = x;
  for (int f = tid; f < F; f += DTD_NT) {
    for (int t = T; t < Tmax; t++) out[ubase + (size_t) t * F + f] = make_float2(0.f, 0.f);
    if (T > 0) for (int k = L - 1; k >= 0; k--) s.H[((size_t) u * F + f) * L + k] = getv(f, k, T - 1);      // descending: reads index k - T < k
  }
}

struct Scratch { DevBuf<unsigned char> st; };
PerStream<Scratch> g_scratch;

void init_state(const dsr_aec& a, void* state, int U, hipStream_t st)
{
  const St s = carve(a, state, U); const long n = (long) U * (a.M / 2 + 1);
  const double k0 = a.kind == 0 ? 0.0 : (a.kind == 1 ? a.sigma2 : a.sigmak2), sv0 = a.kind == 1 ? a.sigma2 : a.sigmau2;      // :117-121, :233-246
  launch(k_aec_init, dim3(cdiv(n > (long) U * 4 ? n : (long) U * 4, 256)), dim3(256), 0, st, s, n, a.L, U, k0, sv0);
}

template <int LP> void launch_block(const dsr_aec& a, const float2* V, const float2* A, const int* nf, int U, int Tmax, int F, const Par& p, const St& s, float2* out,
                                    int frame0, hipStream_t st)
{
  if (a.kind == 3) {
    launch(k_aec_dtd<LP>, dim3(U), dim3(DtdNT<LP>::v), (size_t) 8 * F * sizeof(double), st, V, A, nf, U, Tmax, F, a.L, p, s, out, frame0, a.frameMode);
  } else {
    launch(k_aec_block<LP>, dim3(cdiv((long) U * F, Geo<LP>::CPW)), dim3(64), 0, st, V, A, nf, U, Tmax, F, a.L, p, s, out);
  }
}

}  // namespace

extern "C" {

dsr_status dsr_aec_create(int kind, int fftLen, int sampleN, dsr_aec** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < DSR_AEC_NLMS || kind > DSR_AEC_DTD) throw Error(DSR_E_PARAMETER, "unknown echo canceller kind %d", kind);
    if (fftLen <= 0 || (fftLen & 1)) throw Error(DSR_E_PARAMETER, "fftLen %d: a positive even number is needed", fftLen);
    if (sampleN < 1 || sampleN > DSR_AEC_MAX_SAMPLE_N) throw Error(DSR_E_PARAMETER, "sampleN %d outside [1, %d]", sampleN, DSR_AEC_MAX_SAMPLE_N);
    dsr_aec* a = new dsr_aec(); a->kind = kind; a->M = fftLen; a->L = kind >= DSR_AEC_BLOCK ? sampleN : 1;
    if (kind == DSR_AEC_DTD) a->threshold = 2.0;                                   // snrTh (cancelVP.i:242)
    *out = a;
  });
}
void dsr_aec_destroy(dsr_aec* a) { delete a; }
int dsr_aec_kind(const dsr_aec* a) { return a ? a->kind : -1; }
int dsr_aec_fft_len(const dsr_aec* a) { return a ? a->M : 0; }
int dsr_aec_sample_n(const dsr_aec* a) { return a ? a->L : 0; }

dsr_status dsr_aec_set_nlms(dsr_aec* a, double delta, double epsilon, double threshold)
{
  return guard([&] {
    if (!a) throw Error(DSR_E_PARAMETER, "null argument");
    if (a->kind != DSR_AEC_NLMS) throw Error(DSR_E_PARAMETER, "not an NLMS echo canceller");
    a->delta = delta; a->epsilon = epsilon; a->threshold = threshold;
  });
}
static void check_beta(double beta) { if (!(beta > 0.0 && beta <= 1.0)) throw Error(DSR_E_PARAMETER, "beta %g outside (0, 1]", beta); }
dsr_status dsr_aec_set_kalman(dsr_aec* a, double beta, double sigma2, double threshold)
{
  return guard([&] {
    if (!a) throw Error(DSR_E_PARAMETER, "null argument");
    if (a->kind != DSR_AEC_KALMAN) throw Error(DSR_E_PARAMETER, "not a Kalman echo canceller");
    check_beta(beta); a->beta = beta; a->sigma2 = sigma2; a->threshold = threshold;
  });
}
dsr_status dsr_aec_set_block(dsr_aec* a, double beta, double sigmau2, double sigmak2, double threshold, double amp4play)
{
  return guard([&] {
    if (!a) throw Error(DSR_E_PARAMETER, "null argument");
    if (a->kind != DSR_AEC_BLOCK && a->kind != DSR_AEC_DTD && !aec_info::is_info(*a)) throw Error(DSR_E_PARAMETER, "not a block Kalman echo canceller");
    check_beta(beta); a->beta = beta; a->sigmau2 = sigmau2; a->sigmak2 = sigmak2; a->amp = amp4play;
    if (a->kind == DSR_AEC_BLOCK) a->threshold = threshold;                        // DTD: the threshold is snrTh (cancelVP.cc:1061), see dsr_aec_set_dtd
  });
}
dsr_status dsr_aec_set_dtd(dsr_aec* a, double snrTh, double engTh, double smooth)
{
  return guard([&] {
    if (!a) throw Error(DSR_E_PARAMETER, "null argument");
    if (a->kind != DSR_AEC_DTD) throw Error(DSR_E_PARAMETER, "not a DTD block Kalman echo canceller");
    a->threshold = snrTh; a->engTh = engTh; a->smooth = smooth;
  });
}
dsr_status dsr_aec_set_frame_mode(dsr_aec* a, int mode)
{
  return guard([&] {
    if (!a) throw Error(DSR_E_PARAMETER, "null argument");
    if (mode != 0 && mode != 1) throw Error(DSR_E_PARAMETER, "frame mode %d: 0 (running index) or 1 (constant -5)", mode);
    a->frameMode = mode;
  });
}

size_t dsr_aec_state_bytes(const dsr_aec* a, int U) { return (a && U > 0) ? (aec_info::is_info(*a) ? aec_info::state_bytes(*a, U) : layout(*a, U).bytes) : 0; }

dsr_status dsr_aec_state_init(const dsr_aec* a, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!a || !state_dev || U < 1) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    if (aec_info::is_info(*a)) aec_info::init_state(*a, state_dev, U, (hipStream_t) stream);
    else init_state(*a, state_dev, U, (hipStream_t) stream);
  });
}

dsr_status dsr_aec_reset_filter(const dsr_aec* a, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!a || !state_dev || U < 1) throw Error(DSR_E_PARAMETER, "null argument");
    if (a->kind >= DSR_AEC_BLOCK) return;                                          // the block variants' reset() keeps everything (cancelVP.h:134-142)
    require_device();
    const Layout l = layout(*a, U);
    DSR_HIP(hipMemsetAsync((char*) state_dev + l.oR, 0, l.oK - l.oR, (hipStream_t) stream));      // cancelVP.h:60, :98
  });
}

dsr_status dsr_aec_apply(const dsr_aec* a, const float* played_dev, const float* recorded_dev, const int32_t* nframes_dev, int U, int Tmax, int frame0,
                         float* out_dev, void* state_dev, void* stream)
{
  return guard([&] {
    if (!a || !played_dev || !recorded_dev || !out_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 1 || Tmax < 0) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d Tmax=%d", U, Tmax);
    require_device();
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    if (aec_info::is_info(*a)) {
      aec_info::apply(*a, (const float2*) played_dev, (const float2*) recorded_dev, nframes_dev, U, Tmax, frame0, (float2*) out_dev, state_dev, st);
      return;
    }
    void* state = state_dev;
    if (!state) { Scratch& sc = g_scratch.at(st); sc.st.reserve(layout(*a, U).bytes); state = sc.st.p; init_state(*a, state, U, st); }
    const St s = carve(*a, state, U);
    const int F = a->M / 2 + 1;
    if (a->kind == DSR_AEC_DTD && F > 1024) throw Error(DSR_E_DIMENSION, "DTD: fftLen %d above 2046 (a frame's per-bin scalars live in 64 KiB of LDS)", a->M);
    Par p{a->delta, a->epsilon, a->threshold, a->beta, a->kind == DSR_AEC_KALMAN ? a->sigma2 : a->sigmau2, a->amp, a->engTh, a->smooth};
    const float2* V = (const float2*) played_dev; const float2* A = (const float2*) recorded_dev; float2* out = (float2*) out_dev;
    if (a->kind == DSR_AEC_NLMS)
      launch(k_aec_scalar<0>, dim3(cdiv((long) U * F, 256)), dim3(256), 0, st, V, A, nframes_dev, U, Tmax, F, p, s, out);
    else if (a->kind == DSR_AEC_KALMAN)
      launch(k_aec_scalar<1>, dim3(cdiv((long) U * F, 256)), dim3(256), 0, st, V, A, nframes_dev, U, Tmax, F, p, s, out);
    else if (a->L == 1) launch_block<1>(*a, V, A, nframes_dev, U, Tmax, F, p, s, out, frame0, st);
    else if (a->L == 2) launch_block<2>(*a, V, A, nframes_dev, U, Tmax, F, p, s, out, frame0, st);
    else if (a->L <= 4) launch_block<4>(*a, V, A, nframes_dev, U, Tmax, F, p, s, out, frame0, st);
    else if (a->L <= 8) launch_block<8>(*a, V, A, nframes_dev, U, Tmax, F, p, s, out, frame0, st);
    else if (a->L <= 16) launch_block<16>(*a, V, A, nframes_dev, U, Tmax, F, p, s, out, frame0, st);
    else launch_block<32>(*a, V, A, nframes_dev, U, Tmax, F, p, s, out, frame0, st);
  });
}

dsr_status dsr_aec_state_read(const dsr_aec* a, const void* state_dev, int U, int what, double* host_out, size_t outDoubles)
{
  return guard([&] {
    if (!a || !state_dev || !host_out || U < 1) throw Error(DSR_E_PARAMETER, "null argument");
    if (aec_info::is_info(*a)) { aec_info::read(*a, state_dev, U, what, host_out, outDoubles); return; }
    const Layout l = layout(*a, U); const size_t n = (size_t) U * (a->M / 2 + 1), L = (size_t) a->L;
    size_t off, doubles;
    switch (what) {
      case DSR_AEC_STATE_FILTER: off = l.oR; doubles = n * L * 2; break;
      case DSR_AEC_STATE_K: if (a->kind == DSR_AEC_NLMS) throw Error(DSR_E_PARAMETER, "the NLMS filter has no covariance"); off = l.oK; doubles = n * L * L * 2; break;
      case DSR_AEC_STATE_SIGMA2V: if (a->kind == DSR_AEC_NLMS) throw Error(DSR_E_PARAMETER, "the NLMS filter has no noise variance"); off = l.oSv; doubles = n; break;
      case DSR_AEC_STATE_DTD: if (a->kind != DSR_AEC_DTD) throw Error(DSR_E_PARAMETER, "not a DTD block Kalman echo canceller"); off = l.oD; doubles = (size_t) U * 3; break;
      case DSR_AEC_STATE_HISTORY: off = l.oH; doubles = n * L * 2; break;
      default: throw Error(DSR_E_PARAMETER, "unknown state part %d", what);
    }
    if (outDoubles < doubles) throw Error(DSR_E_DIMENSION, "state part %d needs %zu doubles, the buffer holds %zu", what, doubles, outDoubles);
    require_device();
    DSR_HIP(hipDeviceSynchronize());
    if (what == DSR_AEC_STATE_DTD) {
      std::vector<double> tmp((size_t) U * 4);
      DSR_HIP(hipMemcpy(tmp.data(), (const char*) state_dev + off, tmp.size() * 8, hipMemcpyDeviceToHost));
      for (int u = 0; u < U; u++) for (int k = 0; k < 3; k++) host_out[(size_t) u * 3 + k] = tmp[(size_t) u * 4 + k];
    } else {
      DSR_HIP(hipMemcpy(host_out, (const char*) state_dev + off, doubles * 8, hipMemcpyDeviceToHost));
    }
  });
}

}  // extern "C"
