// csrc/k_mcc.hip -- multichannel cross-correlation source localisation, include/dsr.h section 2f.
//
// Restates SearchGridBuilder / SGB4LinearArray / SGB4CircularArray, MCCLocalizer and MCCCalculator of btk/localization
// (MCCLocalizer.h:55-301, MCCLocalizer.cc:10-576; the delay functions localization.cc:110-142).  The grid code is host-only and keeps the
// reference's float arithmetic; the covariance, its log-determinant and the eigenvalues are fp64 on the device.
//
// Kernels:
//   k_mcc_cost   a workgroup of four waves owns one (utterance, block) and a range of grid points.  The block's channels go through LDS
//                as fp32 in time tiles of K samples plus the D samples of margin on either side that the shifts reach (wrapped to the
//                block's own tail below zero, as the reference's sample holder does); a tile is staged once for four candidates, one a wave.
//                A wave gathers its candidate's shifted rows, four samples a step, converts them to fp64 and accumulates the lower
//                16x16 tiles of X X^T with v_mfma_f64_16x16x4_f64 (the operand a wave loads for tile row I is also tile column I).  Then the
//                sample tile's LDS is reused for the four C x C matrices: scale by 1/(L-D), Cholesky, cost = 2 sum log L_ii - sum log R_ii.
//   k_mcc_nbest  a workgroup per (utterance, block): maxSource rounds of an arg-min over (cost, grid index), which is the order the
//                reference's insertion with strict `<` produces; writes index, cost, tau and position of the kept entries.
//   k_mcc_eig    a wave per kept entry: its R once more through the same Gram code, cyclic Jacobi in LDS, eigenvalues ascending.
// LDS: a channel's row of the sample tile has a stride S = 2 (mod 32) floats, so the 32 lanes that ds_read_b32 serves in one cycle
// (16 channels x 2 consecutive samples) fall on 32 banks when the shifts are equal; unequal shifts conflict as the data dictates.  The
// matrices have a row stride of 16 ceil(C/16) + 1 doubles: a lane per row, and 32 lanes fall on 64 banks of ds_read_b64.
#include "launch.h"
#include "dev_math.h"
#include "mfma64.h"
#include <cmath>

using namespace dsr;

struct dsr_sgb {
  int kind, C, farField; unsigned fs; float maxTimeDelay = -1.0f, constV = 0.0f;
  std::vector<double> mpos, delays; double hypo[3] = {0.0, 0.0, 0.0};
};

struct dsr_mcc {
  int C, G, D, S; unsigned fs;
  std::vector<int> tau; std::vector<double> pos;      // [G][C], [G][3]
  DevBuf<int> d_tau, d_tau1; DevBuf<double> d_pos, d_pos1; bool uploaded = false;
  bool timed = false; hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  ~dsr_mcc() { for (hipEvent_t e : ev) if (e) (void) hipEventDestroy(e); }
};

namespace {

constexpr double SSPEED = 343740.0, TPI = 6.28318530717958647692;
constexpr int MAX_GRID = 65536, MCC_WAVES = 4, MIN_TILE = 64;
constexpr double EMPTY_COST = 100000.0;                     // SourceCandidate's initial cost (MCCLocalizer.h:174)

// ---- the search grids (host, float arithmetic as in the reference) ------------------------------------------------------------------------
void sgb_need_geometry(const dsr_sgb& g)
{
  if (!(g.maxTimeDelay >= 0.0f)) throw Error(DSR_E_INITIALIZATION, "set the geometry of the array before the search grid is used");
}
// nextSearchGridFF of the two builders; false = the walk is over
bool sgb_step(const dsr_sgb& g, double* hypo)
{
  if (!g.farField) { fprintf(stderr, "need to be implemented\n"); return false; }                       // nextSearchGridNF hands out NULL
  if (g.kind == DSR_SGB_LINEAR) {                                                                        // MCCLocalizer.cc:114-143
    const float azimuth = (float) hypo[1], oldSin = sinf(azimuth); float newAzimuth, newSin;
    if (azimuth < M_PI_2) {
      newSin = oldSin + g.constV;
      newAzimuth = newSin >= 1 ? (float) M_PI_2 : asinf(newSin);
    } else if (azimuth < (3 * M_PI_2)) {
      newAzimuth = (float) (3 * M_PI_2);
    } else {
      newSin = oldSin + g.constV;
      if ((newSin + g.constV / 2.0) >= 0) return false;
      newAzimuth = (float) (TPI + asinf(newSin));
    }
    hypo[1] = newAzimuth;
    return true;
  }
  // MCCLocalizer.cc:202-237 with the two stated deviations: |sin|, |cos| in the polar step, and the walk ends when the azimuth reaches 2 pi
  const float azimuth = (float) hypo[1], polarAngle = (float) hypo[2]; float newAzimuth, newPolarAngle, val1, val2;
  if (azimuth >= TPI) return false;
  if ((azimuth >= M_PI_4 && azimuth < (3 * M_PI_4)) || (azimuth >= (5 * M_PI_4) && azimuth < (7 * M_PI_4))) val1 = g.constV / fabsf(sinf(azimuth));
  else val1 = g.constV / fabsf(cosf(azimuth));
  newPolarAngle = (val1 < 1) ? asinf(val1) : (float) M_PI_2;
  if ((newPolarAngle + polarAngle) < M_PI) {
    newPolarAngle += polarAngle; newAzimuth = azimuth;
  } else {
    val2 = g.constV / sinf(newPolarAngle);
    newAzimuth = (val2 < 1) ? (float) acos((double) (g.constV / val2)) : (float) M_PI;
    newAzimuth += azimuth;
  }
  if (newAzimuth >= TPI) return false;
  hypo[1] = newAzimuth; hypo[2] = newPolarAngle;
  return true;
}
void sgb_delays(const dsr_sgb& g, const double* hypo, double* delays)
{
  const int C = g.C;
  if (g.kind == DSR_SGB_LINEAR) {                                                                        // localization.cc:110-121
    const float azimuth = (float) hypo[1];
    delays[0] = 0.0;
    for (int i = 1; i < C; i++) {
      const float dist = (float) fabs(g.mpos[3 * i + 1] - g.mpos[1]);
      delays[i] = -dist * sin((double) azimuth) / SSPEED;
    }
    return;
  }
  const float azimuth = (float) hypo[1], polarAngle = (float) hypo[2], sspeed = (float) SSPEED;            // localization.cc:130-142
  for (int i = 0; i < C; i++) {
    const float cx = -sinf(polarAngle) * cosf(azimuth), cy = -sinf(polarAngle) * sinf(azimuth), cz = -cosf(polarAngle);
    const float delay = (float) ((cx * g.mpos[3 * i] + cy * g.mpos[3 * i + 1] + cz * g.mpos[3 * i + 2]) / sspeed);
    delays[i] = (double) delay;
  }
}
inline int tau_of(unsigned fs, double delay) { const float tau_l = (float) (fs * delay); return (int) tau_l; }   // MCCLocalizer.cc:330-331
inline int sgb_max_sample_delay(const dsr_sgb& g) { return (int) (size_t) (g.fs * g.maxTimeDelay); }            // :268
// the whole walk from (0, 0, 0); any of the outputs may be null
int sgb_enumerate(const dsr_sgb& g, int maxG, double* positions, double* delays, int32_t* tau)
{
  sgb_need_geometry(g);
  if (!g.farField) { fprintf(stderr, "need to be implemented\n"); throw Error(DSR_E_INITIALIZATION, "need to be implemented"); }
  double hypo[3] = {0.0, 0.0, 0.0}; std::vector<double> d(g.C); int G = 0;
  do {
    if (G >= MAX_GRID) throw Error(DSR_E_DIMENSION, "the search grid has more than %d points", MAX_GRID);
    if (G < maxG) {
      sgb_delays(g, hypo, d.data());
      if (positions) for (int k = 0; k < 3; k++) positions[(size_t) G * 3 + k] = hypo[k];
      if (delays) for (int c = 0; c < g.C; c++) delays[(size_t) G * g.C + c] = d[c];
      if (tau) for (int c = 0; c < g.C; c++) tau[(size_t) G * g.C + c] = tau_of(g.fs, d[c]);
    }
    G++;
  } while (sgb_step(g, hypo));
  return G;
}

// ---- device ---------------------------------------------------------------------------------------------------------------------------------
struct MPar { int U, B, C, N, L, D, G, S, K, maxSource, normalize; };

__device__ __forceinline__ bool block_valid(const int* ns, int u, int b, const MPar& p) { const int n = ns ? ns[u] : p.N; return (long) (b + 1) * p.L <= (long) (n < p.N ? n : p.N); }

// The Gram matrices of the workgroup's waves, one candidate a wave (tauW null: the wave idles, it still stages and keeps the barriers).
// xb: channel 0 of the block, channels N floats apart.  acc[t], t = I (I + 1) / 2 + J, J <= I: register q of lane l holds the sum for the channels
// (16 I + (l >> 4) + 4 q, 16 J + (l & 15)) (mfma64.h).
template <int CT> __device__ void mcc_gram(const float* __restrict__ xb, const MPar& p, const int* __restrict__ tauW, float* tile, d4* acc)
{
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6, i = lane & 15, k = lane >> 4;
  const int nS = p.L - p.D, W = p.K + 2 * p.D;
  int off[CT]; bool live[CT];
#pragma unroll
  for (int I = 0; I < CT; I++) {
    const int c = 16 * I + i; live[I] = tauW != nullptr && c < p.C;
    off[I] = live[I] ? c * p.S + p.D + tauW[c] + k : 0;
  }
#pragma unroll
  for (int t = 0; t < CT * (CT + 1) / 2; t++) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  for (int n0 = 0; n0 < nS; n0 += p.K) {
    __syncthreads();
    for (int c = wave; c < p.C; c += waves)
      for (int j = lane; j < W; j += 64) {
        int idx = n0 - p.D + j; if (idx < 0) idx += p.L;                                                 // the holder's samples: the block's own tail
        tile[c * p.S + j] = idx < p.L ? xb[(size_t) c * p.N + idx] : 0.0f;
      }
    __syncthreads();
    if (tauW == nullptr) continue;
    const int kn = nS - n0 < p.K ? nS - n0 : p.K;
    for (int n = 0; n < kn; n += 4) {
      double a[CT];
      const bool in = n + k < kn;
#pragma unroll
      for (int I = 0; I < CT; I++) a[I] = (live[I] && in) ? (double) tile[off[I] + n] : 0.0;
      int t = 0;
#pragma unroll
      for (int I = 0; I < CT; I++)
#pragma unroll
        for (int J = 0; J <= I; J++, t++) acc[t] = mfma64(a[I], a[J], acc[t]);
    }
  }
}

// the wave's matrix R = acc / (L - D) into LDS (both triangles), and on request the lower triangle to global memory
template <int CT> __device__ void mcc_store(const d4* acc, const MPar& p, double* Rw, int RS, double* Rout)
{
  const int lane = threadIdx.x & 63, rr = lane >> 4, cc0 = lane & 15; const double scale = 1.0 / (double) (p.L - p.D);
  int t = 0;
#pragma unroll
  for (int I = 0; I < CT; I++)
#pragma unroll
    for (int J = 0; J <= I; J++, t++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = 16 * I + rr + 4 * q, c = 16 * J + cc0; const double v = acc[t][q] * scale;
        Rw[r * RS + c] = v; if (I != J) Rw[c * RS + r] = v;
        if (Rout && r < p.C && c <= r) Rout[(size_t) r * p.C + c] = v;
      }
}


// dynamic LDS: max(sample tile C x S floats, MCC_WAVES matrices of CP x (CP + 1) doubles)
template <int CT> __global__ __launch_bounds__(64 * MCC_WAVES) void k_mcc_cost(const float* __restrict__ x, const int* __restrict__ ns, const int* __restrict__ tau, MPar p,
                                                                              int gPer, double* __restrict__ cost, double* __restrict__ Rlast)
{
  extern __shared__ double lds[];
  constexpr int CP = 16 * CT, RS = CP + 1, NT = CT * (CT + 1) / 2;
  const int ub = blockIdx.x, u = ub / p.B, b = ub % p.B, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g0 = blockIdx.y * gPer, g1 = g0 + gPer < p.G ? g0 + gPer : p.G;
  if (!block_valid(ns, u, b, p)) {
    for (int g = g0 + threadIdx.x; g < g1; g += blockDim.x) cost[(size_t) ub * p.G + g] = 0.0;
    return;
  }
  const float* xb = x + (size_t) u * p.C * p.N + (size_t) b * p.L;
  float* tile = (float*) lds; double* Rw = lds + (size_t) wave * CP * RS;
  for (int gg = g0; gg < g1; gg += MCC_WAVES) {
    const int g = gg + wave; const bool mine = g < g1;
    d4 acc[NT];
    mcc_gram<CT>(xb, p, mine ? tau + (size_t) g * p.C : nullptr, tile, acc);
    __syncthreads();                                                                                   // the sample tile is free: the matrices take its place
    double lnrm = 0.0, ldet = 0.0; bool bad = false;
    if (mine) {
      mcc_store<CT>(acc, p, Rw, RS, (Rlast && g == p.G - 1) ? Rlast + (size_t) ub * p.C * p.C : nullptr);
    }
    __syncthreads();
    if (mine) {
      const double d = lane < p.C ? Rw[lane * RS + lane] : 1.0;
      bad = __any(!(d > 0.0)) != 0;
      lnrm = wave_sum(lane < p.C && d > 0.0 ? log(d) : 0.0);
    }
    for (int j = 0; j < p.C; j++) {                                                                     // right-looking Cholesky, a lane per row
      double lij = 0.0;
      if (mine) {
        const double piv = Rw[j * RS + j]; const bool okp = piv > 0.0; if (!okp) bad = true;
        const double l = okp ? sqrt(piv) : 1.0;
        ldet += 2.0 * log(l);
        if (lane > j && lane < p.C) { lij = Rw[lane * RS + j] / l; Rw[lane * RS + j] = lij; }
      }
      __syncthreads();
      if (mine)
        for (int k = j + 1; k < p.C; k++) if (lane >= k && lane < p.C) Rw[lane * RS + k] -= lij * Rw[k * RS + j];
      __syncthreads();
    }
    if (mine && lane == 0) {
      double c = ldet - (p.normalize ? lnrm : 0.0);
      if (bad || !(fabs(c) <= 1.7976931348623157e308)) c = 0.0;                                        // a zero or negative pivot, as an exactly zero eigenvalue there
      cost[(size_t) ub * p.G + g] = c;
    }
  }
}

// the maxSource smallest of a block's costs in the order (cost, grid index); entries the grid cannot fill keep index -1 and the initial cost
__global__ __launch_bounds__(256) void k_mcc_nbest(const double* __restrict__ cost, const int* __restrict__ ns, const int* __restrict__ tau, const double* __restrict__ pos,
                                                   MPar p, int* __restrict__ valid, int* __restrict__ index, double* __restrict__ best, int* __restrict__ tauOut,
                                                   double* __restrict__ posOut)
{
  __shared__ double rv[256]; __shared__ int ri[256];
  const int ub = blockIdx.x, u = ub / p.B, b = ub % p.B, tid = threadIdx.x, S = p.maxSource;
  const bool ok = block_valid(ns, u, b, p);
  if (tid == 0) valid[ub] = ok;
  double lastC = -INFINITY; int lastI = -1;
  for (int r = 0; r < S; r++) {
    double bc = INFINITY; int bi = 0x7fffffff;
    if (ok)
      for (int g = tid; g < p.G; g += 256) {
        const double c = cost[(size_t) ub * p.G + g];
        if (!(c < EMPTY_COST) || !(c > lastC || (c == lastC && g > lastI))) continue;
        if (c < bc || (c == bc && g < bi)) { bc = c; bi = g; }
      }
    rv[tid] = bc; ri[tid] = bi;
    for (int o = 128; o >= 1; o >>= 1) {
      __syncthreads();
      if (tid < o) { const double c2 = rv[tid + o]; const int i2 = ri[tid + o]; if (c2 < rv[tid] || (c2 == rv[tid] && i2 < ri[tid])) { rv[tid] = c2; ri[tid] = i2; } }
    }
    __syncthreads();
    const int gi = ri[0]; const double gc = rv[0]; const bool have = gi != 0x7fffffff;
    __syncthreads();
    const size_t e = (size_t) ub * S + r;
    if (tid == 0) { index[e] = ok ? (have ? gi : -1) : 0; best[e] = ok ? (have ? gc : EMPTY_COST) : 0.0; }
    for (int c = tid; c < p.C; c += 256) tauOut[e * p.C + c] = have ? tau[(size_t) gi * p.C + c] : 0;
    if (tid < 3) posOut[e * 3 + tid] = have ? pos[(size_t) gi * 3 + tid] : 0.0;
    if (have) { lastC = gc; lastI = gi; } else { lastC = INFINITY; }
  }
}

// dynamic LDS: the sample tile (C x S floats), then one matrix of CP x (CP + 1) doubles
template <int CT> __global__ __launch_bounds__(64) void k_mcc_eig(const float* __restrict__ x, const int* __restrict__ ns, const int* __restrict__ tau, MPar p,
                                                                  const int* __restrict__ index, double* __restrict__ eig, size_t tileDoubles)
{
  extern __shared__ double lds[];
  constexpr int CP = 16 * CT, RS = CP + 1, NT = CT * (CT + 1) / 2;
  const int e = blockIdx.x, ub = e / p.maxSource, u = ub / p.B, b = ub % p.B, lane = threadIdx.x, C = p.C;
  const int g = index[e];
  if (!block_valid(ns, u, b, p) || g < 0) { if (lane < C) eig[(size_t) e * C + lane] = 0.0; return; }
  float* tile = (float*) lds; double* A = lds + tileDoubles;
  d4 acc[NT];
  mcc_gram<CT>(x + (size_t) u * C * p.N + (size_t) b * p.L, p, tau + (size_t) g * C, tile, acc);
  mcc_store<CT>(acc, p, A, RS, nullptr);
  __syncthreads();
  // cyclic Jacobi by rows: lane i owns A[i][p], A[i][q] and their mirrors in the rotation of (p, q)
  for (int sweep = 0; sweep < 40; sweep++) {
    int rotated = 0;
    for (int pp = 0; pp < C - 1; pp++)
      for (int qq = pp + 1; qq < C; qq++) {
        const double app = A[pp * RS + pp], aqq = A[qq * RS + qq], apq = A[pp * RS + qq];
        if (apq == 0.0 || fabs(apq) <= 1e-17 * sqrt(fabs(app) * fabs(aqq))) continue;                  // uniform over the wave
        rotated = 1;
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
        double aip = 0.0, aiq = 0.0;
        if (lane < C && lane != pp && lane != qq) { aip = A[lane * RS + pp]; aiq = A[lane * RS + qq]; }
        __syncthreads();
        if (lane < C && lane != pp && lane != qq) {
          const double np = cs * aip - sn * aiq, nq = sn * aip + cs * aiq;
          A[lane * RS + pp] = np; A[pp * RS + lane] = np; A[lane * RS + qq] = nq; A[qq * RS + lane] = nq;
        }
        if (lane == pp) { A[pp * RS + pp] = app - t * apq; A[pp * RS + qq] = 0.0; A[qq * RS + pp] = 0.0; }
        if (lane == qq) A[qq * RS + qq] = aqq + t * apq;
        __syncthreads();
      }
    if (!rotated) break;
  }
  // negative values negated as calcObjectiveFunction does (MCCLocalizer.cc:376-381), then ascending
  double* ev = A + (size_t) CP * RS;
  double v = lane < C ? fabs(A[lane * RS + lane]) : 0.0;
  if (lane < C) ev[lane] = v;
  __syncthreads();
  if (lane < C) {
    int rank = 0;
    for (int j = 0; j < C; j++) { const double w = ev[j]; if (w < v || (w == v && j < lane)) rank++; }
    eig[(size_t) e * C + rank] = v;
  }
}

struct MLaunch { int S, K; size_t lds; };
// the sample tile of a kernel: S floats a channel (S = 2 mod 32), K samples a tile; budget = bytes the tile may take
MLaunch mcc_tile(int C, int L, int D, size_t budget)
{
  const int nS = L - D, need = ((nS + 3) & ~3) + 2 * D;
  int S = ((need + 29) / 32) * 32 + 2;                                                                   // smallest S >= need with S = 2 (mod 32)
  const int fit = (int) (budget / (4 * (size_t) C)); int Sfit = fit < 34 ? 0 : ((fit - 2) / 32) * 32 + 2;
  if (S > Sfit) S = Sfit;
  const int K = S >= 2 * D + 4 ? (S - 2 * D) & ~3 : 0;
  return MLaunch{S, K, (size_t) C * S * 4};
}

struct MScratch { DevBuf<double> cost, eig, best, pos; DevBuf<int> valid, index, tau; };
PerStream<MScratch> m_scratch;

void mcc_check_block(int D, int L, int N)
{
  if (L < 1 || N < L) throw Error(DSR_E_DIMENSION, "block length %d, %d samples a channel", L, N);
  if (L < 2 * D) { fprintf(stderr, "Data samples are insufficient. It must be more than %d\n", 2 * D); throw Error(DSR_E_ERROR, "Data samples are insufficient"); }
}

struct MOut { int32_t* valid; int32_t* index; double* cost; int32_t* tau; double* pos; double* eig; double* costMap; double* R; };

// the three kernels over [U][B] blocks with a grid of G candidates (the localiser's table, or the calculator's single row)
void mcc_launch(dsr_mcc* m, const float* x, const int32_t* ns, int U, int N, int L, int G, const int* d_tau, const double* d_pos, int maxSource, int normalize,
                MOut o, hipStream_t st)
{
  const int C = m->C, D = m->D, B = N / L, CT = (C + 15) / 16, CP = 16 * CT;
  const long UB = (long) U * B;
  MScratch& sc = m_scratch.at(st);
  if (!o.costMap) { sc.cost.reserve((size_t) UB * G); o.costMap = sc.cost.p; }
  if (!o.valid) { sc.valid.reserve(UB); o.valid = sc.valid.p; }
  if (!o.index) { sc.index.reserve((size_t) UB * maxSource); o.index = sc.index.p; }
  if (!o.cost) { sc.best.reserve((size_t) UB * maxSource); o.cost = sc.best.p; }
  if (!o.tau) { sc.tau.reserve((size_t) UB * maxSource * C); o.tau = sc.tau.p; }
  if (!o.pos) { sc.pos.reserve((size_t) UB * maxSource * 3); o.pos = sc.pos.p; }
  const size_t matBytes = (size_t) CP * (CP + 1) * 8;
  // k_mcc_cost: the matrices overlay the tile, 4 x 33 280 bytes at C = 64; the tile may take as much, and at least 64 KB
  const size_t costArea = MCC_WAVES * matBytes > 65536 ? MCC_WAVES * matBytes : 65536;
  const MLaunch lc = mcc_tile(C, L, D, costArea), le = mcc_tile(C, L, D, 96 * 1024);
  if (lc.K < MIN_TILE && lc.K < ((L - D + 3) & ~3))
    throw Error(DSR_E_DIMENSION, "a maximum sample delay of %d with %d channels leaves a tile of %d samples in LDS, %d are needed", D, C, lc.K, MIN_TILE);
  if (o.eig && le.K < MIN_TILE && le.K < ((L - D + 3) & ~3))
    throw Error(DSR_E_DIMENSION, "a maximum sample delay of %d with %d channels leaves a tile of %d samples in LDS, %d are needed", D, C, le.K, MIN_TILE);
  MPar p{U, B, C, N, L, D, G, lc.S, lc.K, maxSource, normalize};
  const size_t ldsCost = lc.lds > MCC_WAVES * matBytes ? lc.lds : MCC_WAVES * matBytes;
  int split = (int) (1024 / UB); const int groups = cdiv(G, MCC_WAVES);
  if (split < 1) split = 1; if (split > groups) split = groups;
  const int gPer = cdiv(groups, split) * MCC_WAVES; split = cdiv(G, gPer);
  if (o.R) DSR_HIP(hipMemsetAsync(o.R, 0, (size_t) UB * C * C * 8, st));
  if (m->timed) DSR_HIP(hipEventRecord(m->ev[0], st));
  using MccCt = ints<1, 2, 3, 4>;                                  // channel tiles of 16 the two MFMA kernels are instantiated for; any other count runs the widest
  const int ct = has_value(MccCt{}, CT) ? CT : 4;
  for_value(MccCt{}, ct, [&](auto t) {
    launch(k_mcc_cost<t()>, dim3((unsigned) UB, split), dim3(64 * MCC_WAVES), ldsCost, st, x, ns, d_tau, p, gPer, o.costMap, o.R); });
  if (m->timed) DSR_HIP(hipEventRecord(m->ev[1], st));
  launch(k_mcc_nbest, dim3((unsigned) UB), dim3(256), 0, st, o.costMap, ns, d_tau, d_pos, p, o.valid, o.index, o.cost, o.tau, o.pos);
  if (m->timed) DSR_HIP(hipEventRecord(m->ev[2], st));
  if (o.eig) {
    MPar pe = p; pe.S = le.S; pe.K = le.K;
    const size_t tileDoubles = (le.lds + 7) / 8, ldsEig = tileDoubles * 8 + matBytes + (size_t) CP * 8;
    for_value(MccCt{}, ct, [&](auto t) {
      launch(k_mcc_eig<t()>, dim3((unsigned) (UB * maxSource)), dim3(64), ldsEig, st, x, ns, d_tau, pe, o.index, o.eig, tileDoubles); });
  }
  if (m->timed) DSR_HIP(hipEventRecord(m->ev[3], st));
}

void mcc_validate(const dsr_sgb* g, int maxSource, int* Gout, int* Dout, std::vector<int>* tau, std::vector<double>* pos)
{
  if (!g) throw Error(DSR_E_PARAMETER, "null argument");
  if (maxSource < 1 || maxSource > 64) throw Error(DSR_E_DIMENSION, "maxSource %d outside [1, 64]", maxSource);
  if (g->C < 2 || g->C > 64) throw Error(DSR_E_DIMENSION, "%d channels: 2 to 64 are supported", g->C);
  sgb_need_geometry(*g);                                                                                 // the reference casts maxTimeDelay = -1 to size_t
  const int G = sgb_enumerate(*g, 0, nullptr, nullptr, nullptr), D = sgb_max_sample_delay(*g);
  std::vector<int> t((size_t) G * g->C); std::vector<double> ps((size_t) G * 3);
  sgb_enumerate(*g, G, ps.data(), nullptr, t.data());
  for (size_t i = 0; i < t.size(); i++)
    if (t[i] > D || t[i] < -D) throw Error(DSR_E_DIMENSION, "grid point %zu shifts channel %zu by %d samples, more than the maximum sample delay %d", i / g->C, i % g->C, t[i], D);
  if (Gout) *Gout = G; if (Dout) *Dout = D;
  if (tau) tau->swap(t); if (pos) pos->swap(ps);
}

}  // namespace

extern "C" {

dsr_status dsr_sgb_create(int kind, int nChan, int isFarField, unsigned samplingFreq, dsr_sgb** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind != DSR_SGB_LINEAR && kind != DSR_SGB_CIRCULAR) throw Error(DSR_E_PARAMETER, "unknown search grid kind %d", kind);
    if (nChan < 1 || samplingFreq < 1) throw Error(DSR_E_DIMENSION, "%d channels at %u Hz", nChan, samplingFreq);
    dsr_sgb* g = new dsr_sgb(); g->kind = kind; g->C = nChan; g->farField = isFarField != 0; g->fs = samplingFreq;
    g->mpos.assign((size_t) nChan * 3, 0.0); g->delays.assign(nChan, 0.0);
    *out = g;
  });
}
void dsr_sgb_destroy(dsr_sgb* g) { delete g; }

dsr_status dsr_sgb_set_distance(dsr_sgb* g, float distance)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null argument");
    if (g->kind != DSR_SGB_LINEAR) throw Error(DSR_E_PARAMETER, "setDistanceBtwMicrophones belongs to the linear array");
    const size_t nMic = (size_t) g->C;
    for (size_t micX = 0; micX < nMic; micX++) { g->mpos[3 * micX] = 0.0; g->mpos[3 * micX + 1] = micX * distance; g->mpos[3 * micX + 2] = 0.0; }
    g->constV = (float) (0.99 * SSPEED / ((nMic - 1) * distance * g->fs));
    g->maxTimeDelay = (float) ((nMic - 1) * distance / SSPEED);
  });
}
dsr_status dsr_sgb_set_positions(dsr_sgb* g, const double* mpos, int rows)
{
  return guard([&] {
    if (!g || !mpos) throw Error(DSR_E_PARAMETER, "null argument");
    if (g->kind != DSR_SGB_LINEAR) throw Error(DSR_E_PARAMETER, "setPositionsOfMicrophones belongs to the linear array");
    if (rows != g->C) throw Error(DSR_E_DIMENSION, "The size of the matrix for the geometry of the array should be %d x %d", g->C, 3);
    float maxDist = -1; const float pos0[3] = {(float) mpos[0], (float) mpos[1], (float) mpos[2]};
    for (int micX = 0; micX < rows; micX++) {                                                            // every row, distances from microphone 0
      for (int k = 0; k < 3; k++) g->mpos[3 * micX + k] = mpos[3 * micX + k];
      if (micX > 0) {
        const float dx = pos0[0] - (float) mpos[3 * micX], dy = pos0[1] - (float) mpos[3 * micX + 1], dz = pos0[2] - (float) mpos[3 * micX + 2];
        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        if (dist > maxDist) maxDist = dist;
      }
    }
    g->constV = (float) (0.99 * SSPEED / (maxDist * g->fs));
    g->maxTimeDelay = (float) (maxDist / SSPEED);
  });
}
dsr_status dsr_sgb_set_radius(dsr_sgb* g, float radius, float height)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null argument");
    if (g->kind != DSR_SGB_CIRCULAR) throw Error(DSR_E_PARAMETER, "setRadius belongs to the circular array");
    const size_t nMic = (size_t) g->C; const float bias = (float) (TPI / (float) nMic);
    for (size_t micX = 0; micX < nMic; micX++) {
      g->mpos[3 * micX] = radius * cosf(micX * bias); g->mpos[3 * micX + 1] = radius * sinf(micX * bias); g->mpos[3 * micX + 2] = height;
    }
    g->constV = (float) (SSPEED / (2 * radius * g->fs));
    g->maxTimeDelay = (float) (2 * radius / SSPEED);
  });
}
dsr_status dsr_sgb_reset(dsr_sgb* g) { return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->hypo[0] = g->hypo[1] = g->hypo[2] = 0.0; }); }
dsr_status dsr_sgb_next(dsr_sgb* g, int32_t* more)
{
  return guard([&] {
    if (!g || !more) throw Error(DSR_E_PARAMETER, "null argument");
    sgb_need_geometry(*g);
    *more = sgb_step(*g, g->hypo) ? 1 : 0;
  });
}
dsr_status dsr_sgb_position(const dsr_sgb* g, double* pos3)
{ return guard([&] { if (!g || !pos3) throw Error(DSR_E_PARAMETER, "null argument"); for (int k = 0; k < 3; k++) pos3[k] = g->hypo[k]; }); }
dsr_status dsr_sgb_time_delays(dsr_sgb* g, double* delays)
{
  return guard([&] {
    if (!g || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    sgb_need_geometry(*g);
    sgb_delays(*g, g->hypo, g->delays.data());
    for (int c = 0; c < g->C; c++) delays[c] = g->delays[c];
  });
}
double dsr_sgb_max_time_delay(const dsr_sgb* g) { return g ? (double) g->maxTimeDelay : -1.0; }
int dsr_sgb_chan_n(const dsr_sgb* g) { return g ? g->C : 0; }
int dsr_sgb_sampling_frequency(const dsr_sgb* g) { return g ? (int) g->fs : 0; }
dsr_status dsr_sgb_microphone_positions(const dsr_sgb* g, double* mpos)
{ return guard([&] { if (!g || !mpos) throw Error(DSR_E_PARAMETER, "null argument"); for (size_t i = 0; i < g->mpos.size(); i++) mpos[i] = g->mpos[i]; }); }
dsr_status dsr_sgb_enumerate(const dsr_sgb* g, int maxG, int32_t* G, double* positions, double* delays, int32_t* tau)
{
  return guard([&] {
    if (!g || !G) throw Error(DSR_E_PARAMETER, "null argument");
    *G = sgb_enumerate(*g, maxG < 0 ? 0 : maxG, positions, delays, tau);
  });
}

dsr_status dsr_mcc_check(const dsr_sgb* g, int maxSource, int blockLen)
{
  return guard([&] {
    int G = 0, D = 0; mcc_validate(g, maxSource, &G, &D, nullptr, nullptr);
    if (blockLen > 0) mcc_check_block(D, blockLen, blockLen);
  });
}
dsr_status dsr_mcc_create(const dsr_sgb* g, int maxSource, dsr_mcc** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    std::unique_ptr<dsr_mcc> m(new dsr_mcc());
    mcc_validate(g, maxSource, &m->G, &m->D, &m->tau, &m->pos);
    m->C = g->C; m->fs = g->fs; m->S = maxSource;
    require_device();
    *out = m.release();
  });
}
void dsr_mcc_destroy(dsr_mcc* m) { delete m; }
dsr_status dsr_mcc_check_block(const dsr_mcc* m, int blockLen)
{ return guard([&] { if (!m) throw Error(DSR_E_PARAMETER, "null argument"); mcc_check_block(m->D, blockLen, blockLen); }); }
int dsr_mcc_grid_n(const dsr_mcc* m) { return m ? m->G : 0; }
int dsr_mcc_chan_n(const dsr_mcc* m) { return m ? m->C : 0; }
int dsr_mcc_max_source(const dsr_mcc* m) { return m ? m->S : 0; }
int dsr_mcc_max_sample_delay(const dsr_mcc* m) { return m ? m->D : 0; }
dsr_status dsr_mcc_set_timing(dsr_mcc* m, int on)
{
  return guard([&] {
    if (!m) throw Error(DSR_E_PARAMETER, "null argument");
    if (on) { require_device(); for (hipEvent_t& e : m->ev) if (!e) DSR_HIP(hipEventCreate(&e)); }
    m->timed = on != 0;
  });
}
dsr_status dsr_mcc_kernel_ms(const dsr_mcc* m, double* ms3)
{
  return guard([&] {
    if (!m || !ms3 || !m->timed) throw Error(DSR_E_PARAMETER, "timing is off");
    DSR_HIP(hipEventSynchronize(m->ev[3]));
    for (int k = 0; k < 3; k++) { float a = 0; DSR_HIP(hipEventElapsedTime(&a, m->ev[k], m->ev[k + 1])); ms3[k] = a; }
  });
}

dsr_status dsr_mcc_run(dsr_mcc* m, const float* x_dev, const int32_t* nsamples_dev, int U, int N, int blockLen, int32_t* valid_dev, int32_t* index_dev, double* cost_dev,
                       int32_t* tau_dev, double* position_dev, double* eig_dev, double* costmap_dev, double* R_dev, void* stream)
{
  return guard([&] {
    if (!m || !x_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 1) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d", U);
    mcc_check_block(m->D, blockLen, N);
    require_device();
    hipStream_t st = (hipStream_t) stream;
    if (!m->uploaded) { m->d_tau.upload(m->tau); m->d_pos.upload(m->pos); m->uploaded = true; }
    mcc_launch(m, x_dev, nsamples_dev, U, N, blockLen, m->G, m->d_tau.p, m->d_pos.p, m->S, 1,
               MOut{valid_dev, index_dev, cost_dev, tau_dev, position_dev, eig_dev, costmap_dev, R_dev}, st);
  });
}

dsr_status dsr_mcc_calc(dsr_mcc* m, const float* x_dev, const int32_t* nsamples_dev, int U, int N, int blockLen, const double* delays, int normalizeVariance,
                        int32_t* valid_dev, double* cost_dev, int32_t* tau_host, double* eig_dev, double* R_dev, void* stream)
{
  return guard([&] {
    if (!m || !x_dev || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 1) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d", U);
    mcc_check_block(m->D, blockLen, N);
    std::vector<int> t(m->C);
    for (int c = 0; c < m->C; c++) {
      t[c] = tau_of(m->fs, delays[c]);
      if (t[c] > m->D || t[c] < -m->D) throw Error(DSR_E_INDEX, "channel %d is shifted by %d samples, more than the maximum sample delay %d", c, t[c], m->D);
      if (tau_host) tau_host[c] = t[c];
    }
    require_device();
    hipStream_t st = (hipStream_t) stream;
    const std::vector<double> zero(3, 0.0);
    m->d_tau1.upload(t, st); m->d_pos1.upload(zero, st);
    mcc_launch(m, x_dev, nsamples_dev, U, N, blockLen, 1, m->d_tau1.p, m->d_pos1.p, 1, normalizeVariance != 0,
               MOut{valid_dev, nullptr, cost_dev, nullptr, nullptr, eig_dev, nullptr, R_dev}, st);
    DSR_HIP(hipStreamSynchronize(st));                                                                  // the one-row table may be rewritten by the next call
  });
}

dsr_status dsr_mcc_channel_delays(const dsr_mcc* m, const int32_t* tau, double* delays)
{
  return guard([&] {
    if (!m || !tau || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    for (int c = 0; c < m->C; c++) delays[c] = (double) tau[c] / (double) m->fs;
  });
}

}  // extern "C"
