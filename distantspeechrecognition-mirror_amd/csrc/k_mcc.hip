// csrc/k_mcc.hip -- multichannel cross-correlation source localisation, include/dsr.h section 2f.
//
// Restates MCCLocalizer and MCCCalculator of btk/localization (MCCLocalizer.h:55-301, MCCLocalizer.cc:10-576): the covariance, its
// log-determinant and the eigenvalues are fp64 on the device.  Host side (the search grids, the dsr_sgb_* / dsr_mcc_* entries): csrc/mcc.cpp;
// what the two share: csrc/mcc.h.
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
#include "mcc.h"
#include <cmath>

using namespace dsr;

namespace {

constexpr int MCC_WAVES = 4, MIN_TILE = 64;
constexpr double EMPTY_COST = 100000.0;                     // SourceCandidate's initial cost (MCCLocalizer.h:174)

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

}  // namespace

namespace dsr {

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
  m->tm.mark(0, st);
  using MccCt = ints<1, 2, 3, 4>;                                  // channel tiles of 16 the two MFMA kernels are instantiated for; any other count runs the widest
  const int ct = has_value(MccCt{}, CT) ? CT : 4;
  for_value(MccCt{}, ct, [&](auto t) {
    launch(k_mcc_cost<t()>, dim3((unsigned) UB, split), dim3(64 * MCC_WAVES), ldsCost, st, x, ns, d_tau, p, gPer, o.costMap, o.R); });
  m->tm.mark(1, st);
  launch(k_mcc_nbest, dim3((unsigned) UB), dim3(256), 0, st, o.costMap, ns, d_tau, d_pos, p, o.valid, o.index, o.cost, o.tau, o.pos);
  m->tm.mark(2, st);
  if (o.eig) {
    MPar pe = p; pe.S = le.S; pe.K = le.K;
    const size_t tileDoubles = (le.lds + 7) / 8, ldsEig = tileDoubles * 8 + matBytes + (size_t) CP * 8;
    for_value(MccCt{}, ct, [&](auto t) {
      launch(k_mcc_eig<t()>, dim3((unsigned) (UB * maxSource)), dim3(64), ldsEig, st, x, ns, d_tau, pe, o.index, o.eig, tileDoubles); });
  }
  m->tm.mark(3, st);
}

}  // namespace dsr
