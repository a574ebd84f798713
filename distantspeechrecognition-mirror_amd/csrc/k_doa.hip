// csrc/k_doa.hip -- steered-response-power direction-of-arrival estimation for a linear array:
// DOAEstimatorSRPDSBLA (btk/beamformer/beamformer.h:462-560, beamformer.cc:2920-3283).
//
// Host side (set-up work, as in the reference): the theta grid, the look delays and the steering table
// (_calcSteeringUnitTable :3105-3152, setLookDirection :3257-3271, calcMainlobe :531-594), the final N-best from the accumulators
// (_getNBestHypothesesFromACCRP :2986-3025).  No HIP call is made there, so the table can be inspected without a GPU.
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
#include <algorithm>
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

int theta_n(const dsr_doa& s) { return (int) (unsigned) ((s.maxTheta - s.minTheta) / s.widthTheta + 0.5); }    // :3113

void look_delays(const dsr_doa& s, double theta, double* d)   // setLookDirection (:3257-3271): |x_c - x_0| cos(theta), x only, no speed of sound
{
  if (s.pos.empty()) throw Error(DSR_E_ERROR, "set the array geometry first (setArrayGeometry)");
  if ((int) s.pos.size() < s.C) throw Error(DSR_E_DIMENSION, "the array geometry has %d positions, the estimator %d channels", (int) s.pos.size(), s.C);
  const double ref = s.pos[0];
  d[0] = 0.0;
  for (int c = 1; c < s.C; c++) { double dist = s.pos[c] - ref; if (dist < 0) dist = -dist; d[c] = dist * cos(theta); }
}

void build_table(dsr_doa& s)                                 // _calcSteeringUnitTable (:3105-3152)
{
  if (s.tbl) return;
  check_range(s.fbinMin, s.fbinMax, s.M, s.M / 2);
  const int nT = theta_n(s), C = s.C, M = s.M, M2 = M / 2;
  if (nT < 1 || nT > 65536) throw Error(DSR_E_PARAMETER, "search grid of %d directions (minTheta %g, maxTheta %g, widthTheta %g)", nT, s.minTheta, s.maxTheta, s.widthTheta);
  std::vector<double> d(C);
  look_delays(s, s.minTheta, d.data());                      // geometry errors before anything changes
  s.thetas.assign(nT, 0.0); s.W.assign((size_t) (s.fbinMax + 1) * nT * C, zc(0, 0));
  const double fs = (double) s.sampleRate;
  double theta = s.minTheta;
  for (int k = 0; k < nT; k++, theta += s.widthTheta) {      // theta accumulated in double, as the reference's loop does
    s.thetas[k] = theta;
    look_delays(s, theta, d.data());
    for (int c = 0; c < C; c++) s.W[(size_t) k * C + c] = zc(1, 0);             // bin 0: (1, 0) unless the range starts at 0
    for (int f = s.fbinMin; f <= s.fbinMax; f++)                                // wq_f of calcMainlobe (:557-581)
      for (int c = 0; c < C; c++) {
        zc w;
        if (f == 0) w = std::polar(1.0, 0.0) / (double) C;
        else if (f < M2) { const double val = -2.0 * M_PI * f * d[c] * fs / M; w = std::polar(1.0, val) / (double) C; }
        else { const double val = -M_PI * fs * d[c]; w = std::polar(1.0, val) / (double) C; }
        s.W[((size_t) f * nT + k) * C + c] = w;
      }
  }
  s.nTheta = nT; s.tblFbinMax = s.fbinMax; s.tbl = true; s.tableGen++; s.dDirty = true;
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

void doa_launch_acc(const double* rp, const float* en, const int* nf, int U, int Tmax, int nUnits, float thr, double* acc, hipStream_t st)
{
  launch(k_doa_acc, dim3(cdiv((long) U * nUnits, 256)), dim3(256), 0, st, rp, en, nf, U, Tmax, nUnits, thr, acc);
}

}  // namespace dsr

extern "C" {

dsr_status dsr_doa_create(int nBest, int sampleRate, int fftLen, int chanN, dsr_doa** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (nBest < 1) throw Error(DSR_E_PARAMETER, "nBest %d < 1", nBest);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_PARAMETER, "fftLen %d", fftLen);
    if (chanN < 1 || chanN > 128) throw Error(DSR_E_DIMENSION, "%d channels (1..128 supported)", chanN);
    if (sampleRate <= 0) throw Error(DSR_E_PARAMETER, "sampleRate %d", sampleRate);
    dsr_doa* s = new dsr_doa(); s->nBest = nBest; s->sampleRate = (unsigned) sampleRate; s->M = fftLen; s->C = chanN; s->fbinMax = fftLen / 2;
    *out = s;
  });
}
void dsr_doa_destroy(dsr_doa* s) { delete s; }
int dsr_doa_nbest(const dsr_doa* s) { return s ? s->nBest : 0; }
int dsr_doa_chan_n(const dsr_doa* s) { return s ? s->C : 0; }
int dsr_doa_fft_len(const dsr_doa* s) { return s ? s->M : 0; }
unsigned dsr_doa_table_generation(const dsr_doa* s) { return s ? s->tableGen : 0u; }
int dsr_doa_has_table(const dsr_doa* s) { return s && s->tbl ? 1 : 0; }

dsr_status dsr_doa_set_array_geometry(dsr_doa* s, const double* positions, int n)
{
  return guard([&] {
    if (!s || !positions || n < 1) throw Error(DSR_E_PARAMETER, "null argument");
    s->pos.assign(positions, positions + n);                 // the table is not rebuilt (the reference neither)
  });
}
dsr_status dsr_doa_set_search_param(dsr_doa* s, double minTheta, double maxTheta, double widthTheta)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!(widthTheta > 0.0)) throw Error(DSR_E_PARAMETER, "widthTheta %g must be positive", widthTheta);
    if (minTheta > maxTheta) { fprintf(stderr, "Invalid argument\n"); std::swap(minTheta, maxTheta); }   // beamformer.h:531-537
    s->minTheta = minTheta; s->maxTheta = maxTheta; s->widthTheta = widthTheta;
    s->tbl = false; s->thetas.clear(); s->W.clear(); s->nTheta = 0;     // clearTable (:2962-2984)
  });
}
dsr_status dsr_doa_set_frequency_range(dsr_doa* s, int fbinMin, int fbinMax)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (fbinMin < 0 || fbinMin > fbinMax || fbinMax > s->M / 2) throw Error(DSR_E_DIMENSION, "frequency range [%d, %d] outside [0, %d]", fbinMin, fbinMax, s->M / 2);
    s->fbinMin = fbinMin; s->fbinMax = fbinMax;
  });
}
dsr_status dsr_doa_frequency_range(const dsr_doa* s, int* fbinMin, int* fbinMax)
{ return guard([&] { if (!s || !fbinMin || !fbinMax) throw Error(DSR_E_PARAMETER, "null argument"); *fbinMin = s->fbinMin; *fbinMax = s->fbinMax; }); }
dsr_status dsr_doa_set_energy_threshold(dsr_doa* s, float threshold)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->threshold = threshold; }); }
float dsr_doa_energy_threshold(const dsr_doa* s) { return s ? s->threshold : 0.0f; }

dsr_status dsr_doa_theta_n(dsr_doa* s, int* n)
{
  return guard([&] {
    if (!s || !n) throw Error(DSR_E_PARAMETER, "null argument");
    *n = s->tbl ? s->nTheta : theta_n(*s);
  });
}
dsr_status dsr_doa_thetas(dsr_doa* s, double* out, int n)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    const int nT = s->tbl ? s->nTheta : theta_n(*s);
    if (n < nT) throw Error(DSR_E_DIMENSION, "room for %d directions, the grid has %d", n, nT);
    double theta = s->minTheta;
    for (int k = 0; k < nT; k++, theta += s->widthTheta) out[k] = theta;
  });
}
dsr_status dsr_doa_look_delays(dsr_doa* s, double theta, double* delays)
{ return guard([&] { if (!s || !delays) throw Error(DSR_E_PARAMETER, "null argument"); look_delays(*s, theta, delays); }); }
dsr_status dsr_doa_build_table(dsr_doa* s)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); build_table(*s); }); }
dsr_status dsr_doa_srp_cell(dsr_doa* s, int cell[3], int64_t* ldsBytes)
{
  return guard([&] {
    if (!s || !cell) throw Error(DSR_E_PARAMETER, "null argument");
    build_table(*s);
    const SrpCell c = doa_srp_cell(s->nTheta, s->C);
    cell[0] = c.TG; cell[1] = c.BC; cell[2] = c.KS;
    if (ldsBytes) *ldsBytes = (int64_t) c.ldsBytes;
  });
}
dsr_status dsr_doa_steering(dsr_doa* s, int thetaX, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    build_table(*s);
    if (thetaX < 0 || thetaX >= s->nTheta) throw Error(DSR_E_INDEX, "direction %d of %d", thetaX, s->nTheta);
    const int F = s->M / 2 + 1, C = s->C;
    if (outDoubles < (size_t) F * C * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %d needed", outDoubles, F * C * 2);
    for (int f = 0; f < F; f++)
      for (int c = 0; c < C; c++) {
        const zc w = f <= s->tblFbinMax ? s->W[((size_t) f * s->nTheta + thetaX) * C + c] : zc(0, 0);
        out[((size_t) f * C + c) * 2] = w.real(); out[((size_t) f * C + c) * 2 + 1] = w.imag();
      }
  });
}

dsr_status dsr_doa_srp(dsr_doa* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* energy_dev, double* rp_dev,
                       double* nbest_rp_dev, int32_t* nbest_idx_dev, double* acc_dev, float* Y_dev, int32_t* gated_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !nframes_dev || !energy_dev || !nbest_rp_dev || !nbest_idx_dev || !acc_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "U %d, Tmax %d", U, Tmax);
    build_table(*s);
    check_range(s->fbinMin, s->fbinMax, s->M, s->tblFbinMax);
    require_device();
    if (U == 0 || Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    double* rp = rp_dev;
    if (!rp) { DevBuf<double>& w = s->ws.at(st); w.reserve((size_t) U * Tmax * s->nTheta); rp = w.p; }
    doa_launch_rp(*s, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
    const long nfT = (long) U * Tmax;
    launch(k_doa_frame, dim3(cdiv(nfT, 256)), dim3(256), 0, st, rp, energy_dev, nframes_dev, U, Tmax, s->nTheta, s->nBest, s->threshold,
                       nbest_rp_dev, nbest_idx_dev, gated_dev);
    doa_launch_acc(rp, energy_dev, nframes_dev, U, Tmax, s->nTheta, s->threshold, acc_dev, st);
  });
}

dsr_status dsr_doa_final_nbest(dsr_doa* s, const double* acc, int U, double* nbest_rp, int32_t* nbest_idx)
{
  return guard([&] {
    if (!s || !acc || !nbest_rp || !nbest_idx) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->tbl) throw Error(DSR_E_ERROR, "no steering table: run the estimator after construction / setSearchParam first");
    final_nbest(acc, U, s->nTheta, s->nBest, nbest_rp, nbest_idx);      // _getNBestHypothesesFromACCRP (:2986-3025)
  });
}

}  // extern "C"
