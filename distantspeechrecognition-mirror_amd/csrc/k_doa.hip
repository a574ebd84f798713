// csrc/k_doa.hip -- steered-response-power direction-of-arrival estimation for a linear array:
// DOAEstimatorSRPDSBLA (btk/beamformer/beamformer.h:462-560, beamformer.cc:2920-3283).
//
// Host side (the steering table, the dsr_doa_* entries): csrc/doa.cpp; the handle and the launchers below: csrc/srp_common.h.
//
// Device side, a batch of utterances X [U][C][Tmax][M/2+1] complex64 (the layout dsr_fb_analysis writes):
//   k_doa_srp    rp[u][t][theta] = sum_f g_f |w_theta,f^H X_f|^2 / (fbinMax - fbinMin + 1) (_calcResponsePower :3154-3186) as one complex
//                GEMM per bin on v_mfma_f64_16x16x4_f64: rows theta (16 a tile), columns 16 frames a wave, K = channels (4 a step, zero
//                padded), complex as four real MFMAs.  |.|^2 and the bin sum stay in registers; every rp is written once.  A workgroup owns
//                64 frames of one utterance and TG theta tiles; the snapshots of a bin chunk are staged in LDS as [c][frame][bin] rows
//                (bins on the lanes: coalesced), converted to double in registers.  The steering table is pre-permuted to the MFMA's A
//                operand ([bin][theta tile][k step][lane], conjugated) and read straight from L2.  The workgroups of theta group 0 also
//                compute the frame energy (calcEnergy :3043-3074) from the staged chunk on the VALU, in the reference's order: a float
//                accumulator of double terms, so the gate decision is the reference's bit for bit.  The workgroup owning the last
//                theta writes that unit's beamformed bins (the reference's _vector after next()).
//   k_doa_frame  per frame: the energy gate and the frame's N-best (strict >: on a tie the earlier theta wins; :3207-3239)
//   k_doa_acc    acc[u][theta] += rp of every ungated frame, frame by frame in order (caller-owned: block streaming carries it)
// The MFMA's lane map: csrc/mfma64.h.
#include "launch.h"
#include "srp_common.h"
#include <cmath>
#include <complex>

using namespace dsr;

typedef std::complex<double> zc;

namespace {

template <int TG>
__global__ __launch_bounds__(256) void k_doa_srp(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ Wp,
                                                 int C, int Tmax, int F, int M2, int fbinMin, int fbinMax, int nTheta, int NT, int KS, int BC,
                                                 double* __restrict__ rpOut, float* __restrict__ energy, float2* __restrict__ Y)
{
  extern __shared__ float2 xs[];                             // [C][FB][pitch]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int th0 = blockIdx.x * TG, t0 = blockIdx.y * FB, u = blockIdx.z;
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  if (t0 >= N) return;                                       // workgroup-uniform
  const int BP = bin_pitch(BC), tw = t0 + wave * 16 + i;
  const float2* Xu = X + (long) u * C * Tmax * F;
  const bool doEnergy = blockIdx.x == 0 && threadIdx.x < FB;
  const int lastTile = (nTheta - 1) >> 4, lastRow = (nTheta - 1) & 15;
  d4 rp[TG];
#pragma unroll
  for (int g = 0; g < TG; g++) rp[g] = (d4){0.0, 0.0, 0.0, 0.0};
  float e = 0.0f;
  for (int f0 = fbinMin; f0 <= fbinMax; f0 += BC) {
    const int nb = fbinMax - f0 + 1 < BC ? fbinMax - f0 + 1 : BC;
    srp_stage_chunk(xs, Xu, C, Tmax, F, BC, BP, t0, N, f0, nb);
    if (doEnergy) e = srp_energy_chunk(xs, C, FB, BP, threadIdx.x, f0, nb, M2, e);   // calcEnergy (:3043-3074)
    for (int b = 0; b < nb; b++) {
      const int f = f0 + b;
      const double g = f < M2 ? 2.0 : 1.0;
#pragma unroll
      for (int tg = 0; tg < TG; tg++) {
        const int th = th0 + tg;
        if (th >= NT) break;                                 // uniform
        d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
        const double2* wp = Wp + ((long) f * NT + th) * KS * 64 + lane;   // lane: conj(w[theta = th 16 + (l & 15)][c = 4 ks + (l >> 4)])
        const float2* xb = xs + (kq * FB + wave * 16 + i) * BP + b;       // + 4 ks FB BP: channel 4 ks + (l >> 4)
        int ks = 0;
        for (; ks + 4 <= KS; ks += 4) {                      // four L2 loads in flight before the MFMAs that need them
          double2 a[4]; float2 x[4];
#pragma unroll
          for (int j = 0; j < 4; j++) { a[j] = wp[(ks + j) * 64]; x[j] = ks * 4 + 4 * j + kq < C ? xb[(ks + j) * 4 * FB * BP] : make_float2(0.f, 0.f); }
#pragma unroll
          for (int j = 0; j < 4; j++) cmfma(a[j].x, a[j].y, (double) x[j].x, (double) x[j].y, cr, ci);
        }
        for (; ks + 2 <= KS; ks += 2) {
          double2 a[2]; float2 x[2];
#pragma unroll
          for (int j = 0; j < 2; j++) { a[j] = wp[(ks + j) * 64]; x[j] = ks * 4 + 4 * j + kq < C ? xb[(ks + j) * 4 * FB * BP] : make_float2(0.f, 0.f); }
#pragma unroll
          for (int j = 0; j < 2; j++) cmfma(a[j].x, a[j].y, (double) x[j].x, (double) x[j].y, cr, ci);
        }
        for (; ks < KS; ks++) {
          const double2 a = wp[ks * 64];
          const float2 x = ks * 4 + kq < C ? xb[ks * 4 * FB * BP] : make_float2(0.f, 0.f);
          cmfma(a.x, a.y, (double) x.x, (double) x.y, cr, ci);
        }
        srp_accumulate(rp[tg], cr, ci, g, Y, th == lastTile, lastRow, kq, tw < N, (long) u * Tmax + tw, F, f);
      }
    }
  }
  srp_write_rp(rp, th0, NT, kq, nTheta, tw < N, (long) u * Tmax + tw, fbinMin, fbinMax, rpOut);
  if (doEnergy && t0 + (int) threadIdx.x < N) energy[(long) u * Tmax + t0 + threadIdx.x] = srp_energy_final(e, M2, C);
}

// per frame: gate + N-best of the frame (DOAEstimatorSRPDSBLA::next :3188-3245); nbIdx -1 = an empty rank (rp -10e10, DOA (-pi, -pi))
__global__ void k_doa_frame(const double* __restrict__ rp, const float* __restrict__ energy, const int* __restrict__ nframes, int U, int Tmax,
                            int nTheta, int nBest, float thr, double* __restrict__ nbRp, int* __restrict__ nbIdx, int* __restrict__ gated)
{
  const long k = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (long) U * Tmax) return;
  const int u = (int) (k / Tmax), t = (int) (k - (long) u * Tmax);
  if (t >= nframes[u]) return;
  double* R = nbRp + k * nBest; int* I = nbIdx + k * nBest;
  nbest_reset(R, I, nBest);
  const bool gate = energy[k] < thr;
  if (gated) gated[k] = gate ? 1 : 0;
  if (gate) return;
  const double* r = rp + k * nTheta;
  for (int th = 0; th < nTheta; th++) nbest_insert(R, I, nBest, r[th], th);
}

// acc[u][theta] += rp[u][t][theta] over the ungated frames t < nframes[u], in frame order (_accRPs, :3201)
__global__ void k_doa_acc(const double* __restrict__ rp, const float* __restrict__ energy, const int* __restrict__ nframes, int U, int Tmax,
                          int nTheta, float thr, double* __restrict__ acc)
{
  const long k = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (long) U * nTheta) return;
  const int u = (int) (k / nTheta), th = (int) (k - (long) u * nTheta);
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  const double* r = rp + (long) u * Tmax * nTheta + th; const float* E = energy + (long) u * Tmax;
  double a = acc[k];
  int t = 0;
  for (; t + 8 <= N; t += 8) {                               // loads first, then the additions in frame order
    double v[8]; bool ok[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { v[j] = r[(long) (t + j) * nTheta]; ok[j] = !(E[t + j] < thr); }
#pragma unroll
    for (int j = 0; j < 8; j++) if (ok[j]) a += v[j];
  }
  for (; t < N; t++) if (!(E[t] < thr)) a += r[(long) t * nTheta];
  acc[k] = a;
}

void upload_table(dsr_doa& s, hipStream_t st)
{
  if (!s.dDirty) return;
  const int F = s.M / 2 + 1, C = s.C, nT = s.nTheta; s.NT = srp_tiles(nT); s.KS = srp_ksteps(C);
  std::vector<double2> h((size_t) F * s.NT * s.KS * 64, make_double2(0.0, 0.0));
  for (int f = 0; f <= s.tblFbinMax; f++)
    for (int th = 0; th < s.NT; th++)
      for (int ks = 0; ks < s.KS; ks++)
        for (int l = 0; l < 64; l++) {
          const int k = th * 16 + (l & 15), c = ks * 4 + (l >> 4);
          if (k >= nT || c >= C) continue;
          const zc w = s.W[((size_t) f * nT + k) * C + c];
          h[(((size_t) f * s.NT + th) * s.KS + ks) * 64 + l] = make_double2(w.real(), -w.imag());
        }
  s.dW.upload(h, st); s.dDirty = false;
}

template <int TG>
void launch_srp(const dsr_doa& s, const SrpCell& c, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st)
{
  const int F = s.M / 2 + 1;
  dim3 grid((s.NT + TG - 1) / TG, (Tmax + FB - 1) / FB, U);
  launch(k_doa_srp<TG>, grid, dim3(256), c.ldsBytes, st, (const float2*) X, nf, s.dW.p, s.C, Tmax, F, s.M / 2, s.fbinMin, s.fbinMax,
                     s.nTheta, s.NT, c.KS, c.BC, rp, en, (float2*) Y);
}

}  // namespace

namespace dsr {

void doa_launch_rp(dsr_doa& s, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st)
{
  upload_table(s, st);
  const SrpCell c = doa_srp_cell(s.nTheta, s.C);             // what dsr_doa_srp_cell reports
  if (c.TG == 4) launch_srp<4>(s, c, X, nf, U, Tmax, rp, en, Y, st);
  else if (c.TG == 2) launch_srp<2>(s, c, X, nf, U, Tmax, rp, en, Y, st);
  else launch_srp<1>(s, c, X, nf, U, Tmax, rp, en, Y, st);
}

void doa_launch_frame(const double* rp, const float* en, const int* nf, int U, int Tmax, int nUnits, int nBest, float thr, double* nbRp, int* nbIdx,
                      int* gated, hipStream_t st)
{
  launch(k_doa_frame, dim3(cdiv((long) U * Tmax, 256)), dim3(256), 0, st, rp, en, nf, U, Tmax, nUnits, nBest, thr, nbRp, nbIdx, gated);
}

void doa_launch_acc(const double* rp, const float* en, const int* nf, int U, int Tmax, int nUnits, float thr, double* acc, hipStream_t st)
{
  launch(k_doa_acc, dim3(cdiv((long) U * nUnits, 256)), dim3(256), 0, st, rp, en, nf, U, Tmax, nUnits, thr, acc);
}

}  // namespace dsr
