// csrc/k_sph.hip -- the kernels of spherical-array (modal) beamforming and 2-D steered-response-power DOA estimation (EigenBeamformer,
// SphericalDSBeamformer and the further kinds, DOAEstimatorSRPEB, DOAEstimatorSRPSphDSB; btk/beamformer/modalBeamformer.{h,cc}), with what knows
// a kernel's operand layout or instantiations: the uploads in MFMA operand order, the path picks and the launchers.  The weight designs, the
// steering table and the dsr_sph_* entries are host code in csrc/sph.cpp; csrc/sph.h holds the handle and declares what this file exports.
//
// A batch of utterances X [U][C][Tmax][M/2+1] complex64 (the layout dsr_fb_analysis writes):
//   k_sph_apply  the beamformer: F = sh_s X per bin and frame (sphericalHarmonicsTransformation), y = w^H F, optionally F itself.  One
//                thread per (utterance, frame, bin) on the VALU, the eigenbeams 8 at a time in registers; X is re-read per group of 8
//                from L1/L2.  S and w are wave-uniform or per-bin reads.
//   k_sph_srp    rp[u][t][unit] = sum_f g_f |w_unit,f^H (S X_f)|^2 / (fbinMax - fbinMin + 1) fused on v_mfma_f64_16x16x4_f64: the
//                staging, frame tiles and energy of k_doa_srp; stage 1 forms the 16 frames' eigenbeams F (rows dim, 16 a tile, K = C)
//                in registers; stage 2 contracts them with 16-unit tiles.  The MFMA's result register q of lane l holds
//                F[16 dt + (l >> 4) + 4 q][frame l & 15], exactly the B operand of a K step q whose k index is (l >> 4): the weights are
//                pre-permuted to that order ([bin][unit tile][dim tile][q][lane], conjugated), so F never leaves the registers.
//   folded       W_f^H S precomputed on the host as a [units][C] table and run through k_doa_srp (csrc/k_doa.hip) unchanged: exact up to
//                fp64 rounding, cheaper when dim (C + units) >= C units.  sph_srp_path picks by that flop count; DSR_SPH_SRP_PATH=fused|folded
//                forces one.
//   k_sph_frame  per frame, one wave: the gate and the frame's N-best by (rp descending, unit ascending), which is the reference's strict-">"
//                insertion (:922-943) since every rp >= 0 > -10e10; nBest rounds of a wave arg-max over the frame's row
//   k_doa_acc    (csrc/k_doa.hip) acc[u][unit] += rp of every ungated frame, frame by frame in order
//   k_sph_beams_valu / k_sph_beams_mfma   NB <= 16 beams in one pass over X: Y[u][b][t][f] = v_{b,f}^H X[u][:,t,f] with sensor-domain vectors v
//                (the modal kinds' w_eff^H S folded on the host in fp64, the sensor-domain kinds' weights as they are).  Up to 4 beams: one thread
//                per (t, f) on the VALU, x read once (the (t, f) plane of a channel is contiguous: coalesced whatever F is), the beams'
//                accumulators in registers (fp64), conj(v) staged in LDS a few channels at a time.  Above 4: the complex GEMM of k_doa_srp
//                (rows 16 beams zero padded, columns 16 frames a wave, K = C) without the power reduction; every result is stored.
// The MFMA's lane map: csrc/mfma64.h; the frame tiling (FB, bin_chunk) and the shared kernel parts: csrc/srp_common.h.
#include "launch.h"
#include "sph.h"

using namespace dsr;

typedef std::complex<double> zc;

namespace {

// y[u][t][f] = w_f^H (S X_f), Fo[u][t][f][d] = (S X_f)_d (optional), for t < nframes[u], f = 0..M/2
__global__ __launch_bounds__(256) void k_sph_apply(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ S,
                                                   const double2* __restrict__ Wl, int C, int Tmax, int F, int dim, float2* __restrict__ Y, float2* __restrict__ Fo)
{
  const long k = (long) blockIdx.x * blockDim.x + threadIdx.x;
  const int u = blockIdx.y;
  if (k >= (long) Tmax * F) return;
  const int t = (int) (k / F), f = (int) (k - (long) t * F);
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  if (t >= N) return;
  const float2* x = X + ((long) u * C * Tmax + t) * F + f;   // + c Tmax F
  const double2* w = Wl + (long) f * dim;
  double yr = 0.0, yi = 0.0;
  float2* fo = Fo ? Fo + (((long) u * Tmax + t) * F + f) * dim : nullptr;
  for (int d0 = 0; d0 < dim; d0 += 8) {
    double fr[8], fi[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { fr[j] = 0.0; fi[j] = 0.0; }
    for (int c = 0; c < C; c++) {
      const float2 v = x[(long) c * Tmax * F]; const double xr = v.x, xi = v.y;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        if (d0 + j >= dim) break;
        const double2 sc = S[(long) (d0 + j) * C + c];       // wave-uniform
        fr[j] += sc.x * xr - sc.y * xi; fi[j] += sc.x * xi + sc.y * xr;
      }
    }
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (d0 + j >= dim) break;
      const double2 wd = w[d0 + j];                          // conj(w) F
      yr += wd.x * fr[j] + wd.y * fi[j]; yi += wd.x * fi[j] - wd.y * fr[j];
      if (fo) fo[d0 + j] = make_float2((float) fr[j], (float) fi[j]);
    }
  }
  Y[((long) u * Tmax + t) * F + f] = make_float2((float) yr, (float) yi);
}

// the fused SRP: see the file header.  Sp [DT][KS][64] (S as the A operand), Wp [F][NT][DT][4][64] (conj w in stage 2's K order)
template <int TG, int DT>
__global__ __launch_bounds__(256) void k_sph_srp(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ Sp,
                                                 const double2* __restrict__ Wp, int C, int Tmax, int F, int M2, int fbinMin, int fbinMax, int nUnits,
                                                 int NT, int KS, int BC, double* __restrict__ rpOut, float* __restrict__ energy, float2* __restrict__ Y)
{
  extern __shared__ float2 xs[];                             // [C][FB][pitch]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int th0 = blockIdx.x * TG, t0 = blockIdx.y * FB, u = blockIdx.z;
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  if (t0 >= N) return;                                       // workgroup-uniform
  const int BP = bin_pitch(BC), tw = t0 + wave * 16 + i;
  const float2* Xu = X + (long) u * C * Tmax * F;
  const bool doEnergy = blockIdx.x == 0 && threadIdx.x < FB;
  const int lastTile = (nUnits - 1) >> 4, lastRow = (nUnits - 1) & 15;
  d4 rp[TG];
#pragma unroll
  for (int g = 0; g < TG; g++) rp[g] = (d4){0.0, 0.0, 0.0, 0.0};
  float e = 0.0f;
  for (int f0 = fbinMin; f0 <= fbinMax; f0 += BC) {
    const int nb = fbinMax - f0 + 1 < BC ? fbinMax - f0 + 1 : BC;
    srp_stage_chunk(xs, Xu, C, Tmax, F, BC, BP, t0, N, f0, nb);
    if (doEnergy) e = srp_energy_chunk(xs, C, FB, BP, threadIdx.x, f0, nb, M2, e);   // calcEnergy (beamformer.cc:3043-3074)
    for (int b = 0; b < nb; b++) {
      const int f = f0 + b;
      const double g = f < M2 ? 2.0 : 1.0;
      d4 Fr[DT], Fi[DT];                                     // stage 1: the 16 frames' eigenbeams, rows 16 dt + kq + 4 q
      const float2* xb = xs + (kq * FB + wave * 16 + i) * BP + b;   // + 4 ks FB BP: channel 4 ks + kq
#pragma unroll
      for (int dt = 0; dt < DT; dt++) {
        d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
        const double2* sp = Sp + (long) dt * KS * 64 + lane;
        int ks = 0;
        for (; ks + 2 <= KS; ks += 2) {
          double2 a[2]; float2 x[2];
#pragma unroll
          for (int j = 0; j < 2; j++) { a[j] = sp[(ks + j) * 64]; x[j] = ks * 4 + 4 * j + kq < C ? xb[(ks + j) * 4 * FB * BP] : make_float2(0.f, 0.f); }
#pragma unroll
          for (int j = 0; j < 2; j++) cmfma(a[j].x, a[j].y, (double) x[j].x, (double) x[j].y, cr, ci);
        }
        for (; ks < KS; ks++) {
          const double2 a = sp[ks * 64];
          const float2 x = ks * 4 + kq < C ? xb[ks * 4 * FB * BP] : make_float2(0.f, 0.f);
          cmfma(a.x, a.y, (double) x.x, (double) x.y, cr, ci);
        }
        Fr[dt] = cr; Fi[dt] = ci;
      }
#pragma unroll
      for (int tg = 0; tg < TG; tg++) {                      // stage 2: 16 units a tile, K = dim in the permuted order
        const int th = th0 + tg;
        if (th >= NT) break;                                 // uniform
        d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
        const double2* wp = Wp + ((long) f * NT + th) * DT * 256 + lane;
#pragma unroll
        for (int dt = 0; dt < DT; dt++) {
          double2 a[4];
#pragma unroll
          for (int q = 0; q < 4; q++) a[q] = wp[(dt * 4 + q) * 64];
#pragma unroll
          for (int q = 0; q < 4; q++) cmfma(a[q].x, a[q].y, Fr[dt][q], Fi[dt][q], cr, ci);
        }
        srp_accumulate(rp[tg], cr, ci, g, Y, th == lastTile, lastRow, kq, tw < N, (long) u * Tmax + tw, F, f);
      }
    }
  }
  srp_write_rp(rp, th0, NT, kq, nUnits, tw < N, (long) u * Tmax + tw, fbinMin, fbinMax, rpOut);
  if (doEnergy && t0 + (int) threadIdx.x < N) energy[(long) u * Tmax + t0 + threadIdx.x] = srp_energy_final(e, M2, C);
}

// true when (r, k) ranks before (br, bk): rp descending, unit ascending
__device__ __forceinline__ bool ahead(double r, int k, double br, int bk) { return r > br || (r == br && k < bk); }

// per frame, one wave: gate + N-best of the frame (next :892-947); nbIdx -1 = an empty rank (rp -10e10, DOA (-pi, -pi))
__global__ __launch_bounds__(256) void k_sph_frame(const double* __restrict__ rp, const float* __restrict__ energy, const int* __restrict__ nframes, int U,
                                                   int Tmax, int nUnits, int nBest, float thr, double* __restrict__ nbRp, int* __restrict__ nbIdx,
                                                   int* __restrict__ gated)
{
  const long k = (long) blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= (long) U * Tmax) return;                          // wave-uniform
  const int u = (int) (k / Tmax), t = (int) (k - (long) u * Tmax);
  int N = nframes[u]; if (N > Tmax) N = Tmax;
  if (t >= N) return;
  const bool gate = energy[k] < thr;
  if (gated && lane == 0) gated[k] = gate ? 1 : 0;
  const double* r = rp + k * nUnits;
  double pr = INFINITY; int pk = -1; bool done = gate;
  for (int n = 0; n < nBest; n++) {
    double br = -INFINITY; int bk = 0x7fffffff;
    if (!done) {
      for (int j = lane; j < nUnits; j += 64) {
        const double v = r[j];
        if (ahead(pr, pk, v, j) && ahead(v, j, br, bk)) { br = v; bk = j; }   // after the previous rank, before the best so far
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double orr = __shfl_xor(br, o); const int ok = __shfl_xor(bk, o);
        if (ahead(orr, ok, br, bk)) { br = orr; bk = ok; }
      }
      if (bk == 0x7fffffff) done = true;
    }
    if (lane == 0) { nbRp[k * nBest + n] = done ? -10e10 : br; nbIdx[k * nBest + n] = done ? -1 : bk; }
    pr = br; pk = bk;
  }
}

// Y[u][b][t][f] = sum_c Vc[c][b][f] X[u][c][t][f] for NB beams (Vc = conj v, [C][NB][F]); one thread per E elements k = t F + f of a channel's
// contiguous (t, f) plane, so the float2 loads are coalesced whatever F is.  sv: conj(v) of CC channels at a time, [CC][NB][F].  Rows from
// nframes[u] on are written as zeros.
template <int NB, int E>
__global__ __launch_bounds__(256) void k_sph_beams_valu(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ Vc,
                                                        int C, int Tmax, int F, int CC, int nbOut, float2* __restrict__ Y)
{
  extern __shared__ double2 sv[];
  const int u = blockIdx.y, tid = threadIdx.x;
  int N = nframes[u]; if (N > Tmax) N = Tmax; if (N < 0) N = 0;
  const long TF = (long) Tmax * F, live = (long) N * F, base = (long) blockIdx.x * (256 * E);
  double yr[E][NB], yi[E][NB]; int fe[E]; long ke[E];
#pragma unroll
  for (int e = 0; e < E; e++) {
    ke[e] = base + e * 256 + tid; fe[e] = (int) (ke[e] % F);
#pragma unroll
    for (int b = 0; b < NB; b++) { yr[e][b] = 0.0; yi[e][b] = 0.0; }
  }
  if (base < live) {                                         // workgroup-uniform
    const float2* Xu = X + (long) u * C * TF;
    for (int c0 = 0; c0 < C; c0 += CC) {
      const int nc = C - c0 < CC ? C - c0 : CC;
      __syncthreads();
      for (int idx = tid; idx < nc * NB * F; idx += 256) sv[idx] = Vc[(long) c0 * NB * F + idx];
      __syncthreads();
      for (int cc = 0; cc < nc; cc++) {
        float2 x[E];
#pragma unroll
        for (int e = 0; e < E; e++) x[e] = ke[e] < live ? Xu[(long) (c0 + cc) * TF + ke[e]] : make_float2(0.f, 0.f);
#pragma unroll
        for (int e = 0; e < E; e++) {
          const double xr = x[e].x, xi = x[e].y;
#pragma unroll
          for (int b = 0; b < NB; b++) {
            const double2 v = sv[(cc * NB + b) * F + fe[e]];
            yr[e][b] += v.x * xr - v.y * xi; yi[e][b] += v.x * xi + v.y * xr;
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < E; e++) {
    if (ke[e] >= TF) continue;
#pragma unroll
    for (int b = 0; b < NB; b++)
      if (b < nbOut) Y[((long) u * nbOut + b) * TF + ke[e]] = make_float2((float) yr[e][b], (float) yi[e][b]);
  }
}

// the same as one complex GEMM per bin on v_mfma_f64_16x16x4_f64: the staging and operand layout of k_doa_srp with one row tile (the beams, zero
// padded to 16), Vp [F][KS][64] = conj v as the A operand; result register q of lane l is beam (l >> 4) + 4 q of frame l & 15.  A chunk's results
// are kept as float2 and stored a beam row at a time (consecutive bins of one frame).  Frames from nframes[u] on are staged as zeros.
template <int BCT>
__global__ __launch_bounds__(256) void k_sph_beams_mfma(const float2* __restrict__ X, const int* __restrict__ nframes, const double2* __restrict__ Vp,
                                                        int C, int Tmax, int F, int NB, int KS, float2* __restrict__ Y)
{
  extern __shared__ float2 xs[];                             // [C][FB][pitch]
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, kq = lane >> 4;
  const int t0 = blockIdx.x * FB, u = blockIdx.y;
  int N = nframes[u]; if (N > Tmax) N = Tmax; if (N < 0) N = 0;
  const int BP = bin_pitch(BCT), tw = t0 + wave * 16 + i;
  const float2* Xu = X + (long) u * C * Tmax * F;
  if (t0 >= N) {                                             // workgroup-uniform: nothing to read, the rows are zero
    const int nt = Tmax - t0 < FB ? Tmax - t0 : FB;
    for (int b = 0; b < NB; b++)
      for (int idx = threadIdx.x; idx < nt * F; idx += 256) Y[(((long) u * NB + b) * Tmax + t0) * F + idx] = make_float2(0.f, 0.f);
    return;
  }
  for (int f0 = 0; f0 < F; f0 += BCT) {
    const int nb = F - f0 < BCT ? F - f0 : BCT;
    srp_stage_chunk(xs, Xu, C, Tmax, F, BCT, BP, t0, N, f0, nb);
    float2 out[BCT][4];
#pragma unroll
    for (int b = 0; b < BCT; b++) {
      d4 cr = {0.0, 0.0, 0.0, 0.0}, ci = {0.0, 0.0, 0.0, 0.0};
      if (b < nb) {                                          // uniform
        const double2* vp = Vp + (long) (f0 + b) * KS * 64 + lane;   // lane: conj(v[beam = l & 15][c = 4 ks + (l >> 4)])
        const float2* xb = xs + (kq * FB + wave * 16 + i) * BP + b;  // + 4 ks FB BP: channel 4 ks + (l >> 4)
        int ks = 0;
        for (; ks + 4 <= KS; ks += 4) {
          double2 a[4]; float2 x[4];
#pragma unroll
          for (int j = 0; j < 4; j++) { a[j] = vp[(ks + j) * 64]; x[j] = ks * 4 + 4 * j + kq < C ? xb[(ks + j) * 4 * FB * BP] : make_float2(0.f, 0.f); }
#pragma unroll
          for (int j = 0; j < 4; j++) cmfma(a[j].x, a[j].y, (double) x[j].x, (double) x[j].y, cr, ci);
        }
        for (; ks < KS; ks++) {
          const double2 a = vp[ks * 64];
          const float2 x = ks * 4 + kq < C ? xb[ks * 4 * FB * BP] : make_float2(0.f, 0.f);
          cmfma(a.x, a.y, (double) x.x, (double) x.y, cr, ci);
        }
      }
#pragma unroll
      for (int q = 0; q < 4; q++) out[b][q] = make_float2((float) cr[q], (float) ci[q]);
    }
    if (tw < Tmax) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int beam = kq + 4 * q;
        if (beam >= NB) continue;
        float2* y = Y + (((long) u * NB + beam) * Tmax + tw) * F + f0;
#pragma unroll
        for (int b = 0; b < BCT; b++) if (b < nb) y[b] = out[b][q];
      }
    }
  }
}

int beams_bin_chunk(int C)                                   // the staged chunk's bins: the power of two <= 8 whose rows fit (srp_common.h: bin_chunk)
{
  const int BC = bin_chunk(C);
  return BC > 8 ? 8 : BC;
}

constexpr size_t BEAMS_LDS = 48 * 1024;                      // the VALU kernel's staged conj(v): CC channels x NBT beams x F bins

int valu_chunk(int NBT, int F, int C)                        // CC: the channels whose staged conj(v) (NBT rows x F bins each) fit BEAMS_LDS at a time
{
  int CC = (int) (BEAMS_LDS / ((size_t) NBT * F * sizeof(double2))); if (CC > C) CC = C;
  if (CC < 1) throw Error(DSR_E_DIMENSION, "%d beams x %d bins do not fit the kernel's %zu bytes of LDS", NBT, F, BEAMS_LDS);
  return CC;
}
size_t valu_lds_bytes(int NBT, int F, int CC) { return (size_t) CC * NBT * F * sizeof(double2); }

template <int NBT, int E>
void launch_beams_valu(const dsr_sph& s, const float* X, const int* nf, int U, int Tmax, int NB, float* Y, hipStream_t st)
{
  const int F = s.M / 2 + 1, CC = valu_chunk(NBT, F, s.C);
  launch(k_sph_beams_valu<NBT, E>, dim3(cdiv((long) Tmax * F, 256 * E), U), dim3(256), valu_lds_bytes(NBT, F, CC), st, (const float2*) X, nf, s.dV.p,
                     s.C, Tmax, F, CC, NB, (float2*) Y);
}

template <int BCT>
void launch_beams_mfma(const dsr_sph& s, const float* X, const int* nf, int U, int Tmax, int NB, float* Y, hipStream_t st)
{
  launch(k_sph_beams_mfma<BCT>, dim3((Tmax + FB - 1) / FB, U), dim3(256), srp_lds_bytes(s.C, BCT), st, (const float2*) X, nf, s.dV.p, s.C, Tmax,
                     s.M / 2 + 1, NB, srp_ksteps(s.C), (float2*) Y);
}

int valu_rows(int NB) { return NB <= 4 ? NB : NB <= 8 ? 8 : 16; }   // the VALU kernel's instantiations: 1..4 exact, above that zero-padded rows

void upload_beams(dsr_sph& s, int NB, int path, hipStream_t st)   // conj(v): layout 0 [F][KS][64] (MFMA A operand), n > 0 [C][n][F] (VALU, n rows)
{
  const int layout = path == 1 ? 0 : valu_rows(NB);
  if (!s.dVDirty && s.dVLayout == layout) return;
  const int F = s.M / 2 + 1, C = s.C, KS = srp_ksteps(C);
  std::vector<double2> h;
  if (layout == 0) {
    h.assign((size_t) F * KS * 64, make_double2(0.0, 0.0));
    for (int f = 0; f < F; f++)
      for (int ks = 0; ks < KS; ks++)
        for (int l = 0; l < 64; l++) {
          const int b = l & 15, c = ks * 4 + (l >> 4);
          if (b >= NB || c >= C) continue;
          const zc v = s.V[((size_t) b * F + f) * C + c];
          h[((size_t) f * KS + ks) * 64 + l] = make_double2(v.real(), -v.imag());
        }
  } else {
    h.assign((size_t) C * layout * F, make_double2(0.0, 0.0));
    for (int c = 0; c < C; c++)
      for (int b = 0; b < NB; b++)
        for (int f = 0; f < F; f++) {
          const zc v = s.V[((size_t) b * F + f) * C + c];
          h[((size_t) c * layout + b) * F + f] = make_double2(v.real(), -v.imag());
        }
  }
  s.dV.upload(h, st); s.dVLayout = layout; s.dVDirty = false;
}

int fused_dim_tiles(int dim) { return dim <= 16 ? 1 : dim <= 32 ? 2 : 4; }           // DT: the fused kernel's 16-row eigenbeam tiles (rows past dim zero)
int fused_tile_group(int NT) { return NT >= 8 ? 8 : NT >= 4 ? 4 : NT >= 2 ? 2 : 1; }   // TG: its unit tiles per workgroup

const char* forced_path()
{
  const char* e = getenv("DSR_SPH_SRP_PATH");
  return e && *e ? e : nullptr;
}

void upload_s(dsr_sph& s, hipStream_t st)                    // S [dim][C] (apply) and Sp [DT][KS][64] (the fused kernel's A operand)
{
  if (!s.dSDirty) return;
  const int D = s.dim, C = s.C; s.DT = fused_dim_tiles(D); s.KS = srp_ksteps(C);
  std::vector<double2> h((size_t) D * C), hp((size_t) s.DT * s.KS * 64, make_double2(0.0, 0.0));
  for (int d = 0; d < D; d++)
    for (int c = 0; c < C; c++) h[(size_t) d * C + c] = make_double2(s.SH[(size_t) d * C + c].real(), s.SH[(size_t) d * C + c].imag());
  for (int dt = 0; dt < s.DT; dt++)
    for (int ks = 0; ks < s.KS; ks++)
      for (int l = 0; l < 64; l++) {
        const int d = dt * 16 + (l & 15), c = ks * 4 + (l >> 4);
        if (d < D && c < C) hp[((size_t) dt * s.KS + ks) * 64 + l] = h[(size_t) d * C + c];
      }
  s.dS.upload(h, st); s.dSp.upload(hp, st); s.dSDirty = false;
}

void upload_fused_table(dsr_sph& s, hipStream_t st)
{
  if (!s.dWDirty) return;
  const int F = s.M / 2 + 1, D = s.dim, nU = units(s); s.NT = srp_tiles(nU);
  const int DT4 = s.DT;
  std::vector<double2> h((size_t) F * s.NT * DT4 * 256, make_double2(0.0, 0.0));
  for (int f = 0; f <= s.tblFbinMax; f++)
    for (int th = 0; th < s.NT; th++)
      for (int dt = 0; dt < DT4; dt++)
        for (int q = 0; q < 4; q++)
          for (int l = 0; l < 64; l++) {
            const int k = th * 16 + (l & 15), d = dt * 16 + (l >> 4) + 4 * q;
            if (k >= nU || d >= D) continue;
            const zc w = s.W[((size_t) f * nU + k) * D + d];
            h[((((size_t) f * s.NT + th) * DT4 + dt) * 4 + q) * 64 + l] = make_double2(w.real(), -w.imag());
          }
  s.dWp.upload(h, st); s.dWDirty = false;
}

template <int TG, int DT>
void launch_fused(const dsr_sph& s, const SphSrpCell& c, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st)
{
  const int F = s.M / 2 + 1;
  dim3 grid((s.NT + TG - 1) / TG, (Tmax + FB - 1) / FB, U);
  launch(k_sph_srp<TG, DT>, grid, dim3(256), c.ldsBytes, st, (const float2*) X, nf, s.dSp.p, s.dWp.p, s.C, Tmax, F, s.M / 2, s.fbinMin, s.fbinMax,
                     units(s), s.NT, c.KS, c.BC, rp, en, (float2*) Y);
}

template <int DT>
void launch_fused_tg(const dsr_sph& s, const SphSrpCell& c, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st)
{
  if (c.TG == 8) launch_fused<8, DT>(s, c, X, nf, U, Tmax, rp, en, Y, st);
  else if (c.TG == 4) launch_fused<4, DT>(s, c, X, nf, U, Tmax, rp, en, Y, st);
  else if (c.TG == 2) launch_fused<2, DT>(s, c, X, nf, U, Tmax, rp, en, Y, st);
  else launch_fused<1, DT>(s, c, X, nf, U, Tmax, rp, en, Y, st);
}

}  // namespace

namespace dsr {

int sph_beams_path(int NB)                                   // 0 VALU (NB <= 4), 1 MFMA; DSR_SPH_BEAMS_PATH=valu|mfma forces one (measurements)
{
  const char* e = getenv("DSR_SPH_BEAMS_PATH");
  if (e && *e) {
    if (!strcmp(e, "valu")) return 0;
    if (!strcmp(e, "mfma")) return 1;
    throw Error(DSR_E_PARAMETER, "DSR_SPH_BEAMS_PATH=%s: valu or mfma", e);
  }
  return NB <= 4 ? 0 : 1;
}

// the kernel of one call: sph_beams_path, but where one channel of the VALU kernel's staged table (rows x F bins) is more than its LDS holds -- rows F
// > 3072: fftLen 2048 with 3 or 4 beams, fftLen >= 6144 with one -- the MFMA kernel, which stages snapshots and has no such limit, takes the call
// (a forced DSR_SPH_BEAMS_PATH=valu is left to fail with DSR_E_DIMENSION: it is for measurements)
int sph_beams_path_for(int NB, int F)
{
  const int path = sph_beams_path(NB);
  if (path == 0 && (size_t) valu_rows(NB) * F * sizeof(double2) > BEAMS_LDS && !getenv("DSR_SPH_BEAMS_PATH")) return 1;
  return path;
}

int sph_srp_path(const dsr_sph& s)                           // 0 fused, 1 folded: folded when dim (C + units) >= C units
{
  if (const char* e = forced_path()) {
    if (!strcmp(e, "fused")) return 0;
    if (!strcmp(e, "folded")) return 1;
    throw Error(DSR_E_PARAMETER, "DSR_SPH_SRP_PATH=%s: fused or folded", e);
  }
  const long nU = units(s);
  return (long) s.dim * (s.C + nU) >= (long) s.C * nU ? 1 : 0;
}

SphSrpCell sph_fused_cell(const dsr_sph& s)                  // the fused launch of s's table: what sph_srp_fused switches on and dsr_sph_srp_cell reports
{
  const int BC = bin_chunk(s.C);
  return SphSrpCell{0, fused_tile_group(srp_tiles(units(s))), fused_dim_tiles(s.dim), BC, srp_ksteps(s.C), srp_lds_bytes(s.C, BC)};
}

SphBeamsCell sph_beams_cell(int NB, int C, int F)            // the launch of one dsr_sph_beams call: what sph_beams switches on and dsr_sph_beams_cell reports
{
  SphBeamsCell c{sph_beams_path_for(NB, F), 0, 0, 0, 0, 0};
  if (c.kernel == 1) { c.BCT = beams_bin_chunk(C); c.KS = srp_ksteps(C); c.ldsBytes = srp_lds_bytes(C, c.BCT); }
  else { c.rows = valu_rows(NB); c.CC = valu_chunk(c.rows, F, C); c.ldsBytes = valu_lds_bytes(c.rows, F, c.CC); }
  return c;
}

void sph_apply(dsr_sph& s, const float* X, const int* nf, int U, int Tmax, float* Y, float* Fo, hipStream_t st)
{
  upload_s(s, st);
  const int F = s.M / 2 + 1;
  if ((long) Tmax * F > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "Tmax %d x %d bins", Tmax, F);
  launch(k_sph_apply, dim3(cdiv((long) Tmax * F, 256), U), dim3(256), 0, st, (const float2*) X, nf, s.dS.p, s.dLook.p,
                     s.C, Tmax, F, s.dim, (float2*) Y, (float2*) Fo);
}

void sph_beams(dsr_sph& s, const float* X, const int* nf, int U, int Tmax, int NB, int path, float* Y, hipStream_t st)
{
  upload_beams(s, NB, path, st);
  if (path == 1) {
    const int BC = sph_beams_cell(NB, s.C, s.M / 2 + 1).BCT;
    if (BC == 8) launch_beams_mfma<8>(s, X, nf, U, Tmax, NB, Y, st);
    else if (BC == 4) launch_beams_mfma<4>(s, X, nf, U, Tmax, NB, Y, st);
    else if (BC == 2) launch_beams_mfma<2>(s, X, nf, U, Tmax, NB, Y, st);
    else launch_beams_mfma<1>(s, X, nf, U, Tmax, NB, Y, st);
  } else {
    switch (sph_beams_cell(NB, s.C, s.M / 2 + 1).rows) {
    case 1: launch_beams_valu<1, 4>(s, X, nf, U, Tmax, NB, Y, st); break;
    case 2: launch_beams_valu<2, 4>(s, X, nf, U, Tmax, NB, Y, st); break;
    case 3: launch_beams_valu<3, 4>(s, X, nf, U, Tmax, NB, Y, st); break;
    case 4: launch_beams_valu<4, 4>(s, X, nf, U, Tmax, NB, Y, st); break;
    case 8: launch_beams_valu<8, 2>(s, X, nf, U, Tmax, NB, Y, st); break;
    default: launch_beams_valu<16, 1>(s, X, nf, U, Tmax, NB, Y, st); break;
    }
  }
}

void sph_srp_fused(dsr_sph& s, const float* X, const int* nf, int U, int Tmax, double* rp, float* en, float* Y, hipStream_t st)
{
  upload_s(s, st); upload_fused_table(s, st);
  const SphSrpCell c = sph_fused_cell(s);                    // c.DT is the s.DT the tables above were laid out for
  if (c.DT == 1) launch_fused_tg<1>(s, c, X, nf, U, Tmax, rp, en, Y, st);
  else if (c.DT == 2) launch_fused_tg<2>(s, c, X, nf, U, Tmax, rp, en, Y, st);
  else launch_fused_tg<4>(s, c, X, nf, U, Tmax, rp, en, Y, st);
}

void sph_frame(const dsr_sph& s, const double* rp, const float* en, const int* nf, int U, int Tmax, double* nbRp, int* nbIdx, int* gated, hipStream_t st)
{
  launch(k_sph_frame, dim3(cdiv((long) U * Tmax, 4)), dim3(256), 0, st, rp, en, nf, U, Tmax, units(s), s.nBest, s.threshold, nbRp, nbIdx, gated);
}

}  // namespace dsr
