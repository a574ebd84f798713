// csrc/sat_kernels.hip -- speaker-adaptive training (ML-SAT): the mean and variance accumulators over a batch of speaker slots, and the
// mean solve, on the device.
//
// Replaces SATMean::accumulate / _solve / _auxFunc / update (asr/sat/sat.cc:171-218, 257-342, "sat"), SATVariance::accumulate (sat:704-729),
// SATBase::MeanAcc::accumulate and VarianceAcc::accumulate (sat:999-1008, 1222-1231), which work on one speaker and one Gaussian at a time,
// with MLLRTransformer::transform (asr/adapt/transform.cc:1770-1785, "tr") and APTTransformerBase::transform (tr:1295-1337) inside the
// variance accumulator.
//
//   k_sat_mean_acc  per (tile of 16 Gaussians of one class, group of 256 columns, block nb): with K = (slot s, row m) and the Gaussians as
//                   rows, the contraction   mat_g[p][q] += (c_sg iv_gm) (A_s[m][p] A_s[m][q])  (p <= q, one column per pair)   and
//                   vec_g[p] += (iv_gm (sumO_sgm - c_sg b_sm)) A_s[m][p]   on v_mfma_f64_16x16x4_f64 (sat:192-207).  c iv is exact (24 + 24
//                   bits); the B operand is the same for every Gaussian of the class and is formed from the slot's block matrix in LDS.
//                   scalar (sat:210-213) is a plain fp64 sum, occ (sat:217, 1007) the sequential double sum in slot order.  A slot whose
//                   float count is 0 contributes nothing (sat:180).  Every accumulator entry is read, added to and written by one lane:
//                   no floating-point atomics, the same calls twice give the same bits.
//   k_sat_var_acc   thread per (Gaussian, component): the slots in order; the transformed mean in the transform's own types, then
//                   vec += sumOsq - 2 trn sumO + c trn^2 and occ += c as the reference writes them (sat:713-726): bit for bit.
//   k_sat_solve     workgroup per (Gaussian, block): auxOld at the current mean, the cyclic Jacobi of mllr_jacobi.h to M = V diag(l) V^T,
//                   x = V diag(1 / l_k if |l_k| / max |l| >= 1e-7 else 0) V^T vec (sat:257-274 for a symmetric matrix), auxNew, the
//                   decision of sat:322 and the float mean; one record per (Gaussian, block), and the solution in double.
// This translation unit is compiled with -ffp-contract=off.
#include "launch.h"
#include "sat.h"
#include "mfma64.h"
#include "sat_dev.h"
#include <cmath>

namespace dsr {

static constexpr int kSolveThreads = 128;
static constexpr int kTilesPerWave = kSatColGroup / 64;

// tile[3 t] = { class index, first sorted Gaussian, Gaussians }; pq[col] = p | q << 16 of a mat column, p of a vec column, -1 of padding.
// kVec false is FastSAT::accumulate (sat:501-528): mat and occ only -- no vec columns (NCp == PZ), no scalar pass, sumO never read
template <bool kVec>
__global__ __launch_bounds__(256) void k_sat_mean_acc(int nSlots, int NC, int nB, int bl, int D, int G, int PZ, int NCp, const float* __restrict__ ivar,
                                                      const double* __restrict__ cnt, const double* __restrict__ sumO, const double* __restrict__ Atab,
                                                      const double* __restrict__ btab, const int* __restrict__ gidx, const int* __restrict__ tile,
                                                      const int* __restrict__ pq, double* macc, double* mocc, int* has)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int sg[kSatTileG];
  const int blp = (bl + 3) & ~3, tid = threadIdx.x;
  double* As = reinterpret_cast<double*>(smem);           // [blp][bl]: the slot's block matrix, rows bl .. blp - 1 zero
  double* bs = As + blp * bl;                             // [blp]
  double* part = bs + blp;                                // [16][16]
  float* ivs = reinterpret_cast<float*>(part + 256);      // [16][blp]
  const int t = blockIdx.x, cg = blockIdx.y, nb = blockIdx.z, off = nb * bl;
  const int cls = tile[3 * t], i0 = tile[3 * t + 1], n = tile[3 * t + 2];
  const long stride = (long) bl * bl + bl + 1;
  if (tid < kSatTileG) sg[tid] = tid < n ? gidx[i0 + tid] : -1;
  __syncthreads();
  for (int e = tid; e < kSatTileG * blp; e += blockDim.x) { const int j = e / blp, m = e - j * blp; ivs[e] = (j < n && m < bl) ? ivar[(long) sg[j] * D + off + m] : 0.0f; }
  const int lane = tid & 63, wave = tid >> 6, lo = lane & 15, hi = lane >> 4;
  const int gl = sg[lo];                                  // the Gaussian of this lane's A row
  int code[kTilesPerWave]; bool isZ[kTilesPerWave], active[kTilesPerWave], anyZ = false;
#pragma unroll
  for (int u = 0; u < kTilesPerWave; u++) {
    const int c0 = ((cg * 4 + wave) * kTilesPerWave + u) * 16;
    active[u] = c0 < NCp; isZ[u] = c0 >= PZ; code[u] = active[u] ? pq[c0 + lo] : -1; anyZ = anyZ || (active[u] && isZ[u]);
  }
  d4 acc[kTilesPerWave];
#pragma unroll
  for (int u = 0; u < kTilesPerWave; u++) acc[u] = d4{0.0, 0.0, 0.0, 0.0};
  for (int s = 0; s < nSlots; s++) {
    __syncthreads();
    const double* A = Atab + (((long) s * NC + cls) * nB + nb) * bl * bl;
    for (int e = tid; e < blp * bl; e += blockDim.x) As[e] = e < bl * bl ? A[e] : 0.0;
    for (int e = tid; e < blp; e += blockDim.x) bs[e] = e < bl ? btab[((long) s * NC + cls) * D + off + e] : 0.0;
    __syncthreads();
    const float cf = gl >= 0 ? (float) cnt[(long) s * G + gl] : 0.0f;       // float c_k = postProb(), sat:1003
    const double cd = (double) cf;
    const double* so = sumO + ((long) s * G + (gl >= 0 ? gl : 0)) * D + off;
    for (int ks = 0; ks < blp / 4; ks++) {
      const int m = 4 * ks + hi;
      double aG = 0.0, aZ = 0.0;
      if (cf != 0.0f && m < bl) {                         // sat:180
        const double iv = (double) ivs[lo * blp + m];
        aG = __dmul_rn(cd, iv);                           // exact
        if (kVec && anyZ) aZ = __dmul_rn(iv, __dsub_rn(so[m], __dmul_rn(cd, bs[m])));
      }
#pragma unroll
      for (int u = 0; u < kTilesPerWave; u++) {
        if (!active[u]) continue;                         // uniform per wave
        double b = 0.0;
        if (code[u] >= 0) { b = As[m * bl + (code[u] & 0xffff)]; if (!isZ[u]) b = __dmul_rn(b, As[m * bl + (code[u] >> 16)]); }
        acc[u] = mfma64(isZ[u] ? aZ : aG, b, acc[u]);
      }
    }
  }
#pragma unroll
  for (int u = 0; u < kTilesPerWave; u++) {
    if (!active[u] || code[u] < 0) continue;
    const int p = code[u] & 0xffff, q = code[u] >> 16;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = hi + 4 * r;
      if (row >= n) continue;
      double* base = macc + ((long) sg[row] * nB + nb) * stride;
      if (isZ[u]) base[bl * bl + p] = __dadd_rn(base[bl * bl + p], acc[u][r]);
      else { const double v = __dadd_rn(base[p * bl + q], acc[u][r]); base[p * bl + q] = v; base[q * bl + p] = v; }
    }
  }
  if (cg != 0) return;
  // scalar: 16 lanes a Gaussian, lane l the rows m = l, l + 16, .. of every slot in order; the 16 partial sums added in lane order
  const int j = tid >> 4, l = tid & 15;
  double sum = 0.0;
  if (kVec && j < n) {
    const int g = sg[j];
    for (int s = 0; s < nSlots; s++) {
      const float cf = (float) cnt[(long) s * G + g]; if (cf == 0.0f) continue;
      const double cd = (double) cf;
      const double* so = sumO + ((long) s * G + g) * D + off; const double* b = btab + ((long) s * NC + cls) * D + off;
      for (int m = l; m < bl; m += 16) {
        const double v1 = __dsub_rn(so[m], __dmul_rn(cd, b[m]));
        sum = __dadd_rn(sum, __ddiv_rn(__dmul_rn(__dmul_rn((double) ivar[(long) g * D + off + m], v1), v1), cd));
      }
    }
  }
  __syncthreads();
  part[tid] = sum;
  __syncthreads();
  if (j < n && l == 0) {
    const int g = sg[j];
    double tot = 0.0;
    for (int k = 0; k < 16; k++) tot = __dadd_rn(tot, part[j * 16 + k]);
    double* base = macc + ((long) g * nB + nb) * stride;
    if (kVec) base[bl * bl + bl] = __dadd_rn(base[bl * bl + bl], tot);
    if (nb == 0) {
      double occ = mocc[g]; int seen = has[g];
      for (int s = 0; s < nSlots; s++) { const float cf = (float) cnt[(long) s * G + g]; if (cf == 0.0f) continue; occ = __dadd_rn(occ, (double) cf); seen = 1; }
      mocc[g] = occ; has[g] = seen;
    }
  }
}

// cls[g]: the class index of Gaussian g; tables [slot][class]; trn (or NULL) [slot][G][D] receives the transformed means
__global__ __launch_bounds__(256) void k_sat_var_acc(int nSlots, int NC, int nB, int bl, int D, int G, int g0, int g1, const float* __restrict__ mean,
                                                     const double* __restrict__ cnt, const double* __restrict__ sumO, const double* __restrict__ sumOsq,
                                                     const double* __restrict__ Atab, const double* __restrict__ btab, const int* __restrict__ kind,
                                                     const int* __restrict__ bsz, const int* __restrict__ cls, double* __restrict__ vvec,
                                                     double* __restrict__ vocc, float* __restrict__ trn)
{
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long) (g1 - g0) * D) return;
  const int g = g0 + (int) (idx / D), k = (int) (idx - (long) (g - g0) * D), nb = k / bl, n = k - nb * bl;
  const float* mu = mean + (long) g * D + nb * bl;
  double vec = vvec[(long) g * D + k], occ = k == 0 ? vocc[g] : 0.0;                  // only the thread that writes occ back reads it
  for (int s = 0; s < nSlots; s++) {
    const float cf = (float) cnt[(long) s * G + g]; if (cf == 0.0f) continue;        // sat:713
    const double cd = (double) cf;
    const long tab = (long) s * NC + cls[g];
    const double* a = Atab + ((tab * nB + nb) * bl + n) * bl;
    const float comp = sat_transform_comp(kind[tab], k < bsz[tab], btab[tab * D + k], a, mu, bl);
    if (trn) trn[((long) s * G + g) * D + k] = comp;
    const long e = ((long) s * G + g) * D + k;
    vec = sat_var_term(vec, sumOsq[e], sumO[e], (double) comp, cd);                    // sat:723-724
    occ = __dadd_rn(occ, cd);
  }
  vvec[(long) g * D + k] = vec;
  if (k == 0) vocc[g] = occ;
}

// solve[k]: the Gaussian; one workgroup per (k, block)
__global__ __launch_bounds__(kSolveThreads) void k_sat_solve(int nB, int bl, int D, const int* __restrict__ solve, const double* __restrict__ macc,
                                                             const float* __restrict__ mean, float* __restrict__ newMean, double* __restrict__ sol,
                                                             SatRecord* __restrict__ rec)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double sh[2]; __shared__ int shKept;
  const int n = bl, m = (n + 1) & ~1, nt = blockDim.x, tid = threadIdx.x;
  double* a = reinterpret_cast<double*>(smem);            // [n][n]
  double* v = a + n * n;                                  // [n][n]
  double* z = v + n * n;                                  // [n] vec
  double* t = z + n;                                      // [n]
  double* x = t + n;                                      // [n] the mean, then the solution
  double* cs = x + n;                                     // [m]
  double* sq = cs + m;                                    // [2 nt]
  const int g = solve[blockIdx.x / nB], nb = blockIdx.x % nB;
  const long stride = (long) n * n + n + 1;
  const double* src = macc + ((long) g * nB + nb) * stride;
  const double scalar = src[n * n + n];
  for (int e = tid; e < n * n; e += nt) { a[e] = src[e]; v[e] = (e / n == e % n) ? 1.0 : 0.0; }
  for (int e = tid; e < n; e += nt) { z[e] = src[n * n + e]; x[e] = (double) mean[(long) g * D + nb * n + e]; }
  __syncthreads();
  sat_rows_times(a, x, t, n, tid, nt);                   // _auxFunc (sat:276-286) at the current mean
  __syncthreads();
  if (tid == 0) sh[0] = sat_aux_value(t, x, z, scalar, n);
  __syncthreads();
  bool ok = sat_jacobi(a, v, n, m, cs, sq, tid, nt);
  for (int e = tid; e < n; e += nt) if (!(fabs(z[e]) <= 1.7E308)) ok = false;
  if (!(fabs(scalar) <= 1.7E308)) ok = false;
  ok = __syncthreads_and(ok);
  SatRecord* out = rec + (long) g * nB + nb;
  if (!ok) { if (tid == 0) { out->kept = 0; out->decision = kSatFlagged; out->auxOld = sh[0]; out->auxNew = 0.0; } return; }
  double lmax = 0.0;
  for (int e = 0; e < n; e++) { const double l = fabs(a[e * n + e]); if (l > lmax) lmax = l; }
  for (int e = tid; e < n; e += nt) {
    double sum = 0.0;
    for (int j = 0; j < n; j++) sum = __dadd_rn(sum, __dmul_rn(v[j * n + e], z[j]));
    const double l = a[e * n + e];
    t[e] = (fabs(l) / lmax >= 1.0e-07) ? sum / l : 0.0;   // MaxSingularValueRatio, sat:255, 265-269
  }
  if (tid == 0) { int kept = 0; for (int e = 0; e < n; e++) if (fabs(a[e * n + e]) / lmax >= 1.0e-07) kept++; shKept = kept; }
  __syncthreads();
  for (int e = tid; e < n; e += nt) {
    double sum = 0.0;
    for (int j = 0; j < n; j++) sum = __dadd_rn(sum, __dmul_rn(v[e * n + j], t[j]));
    x[e] = sum; sol[(long) g * D + nb * n + e] = sum;
  }
  __syncthreads();
  sat_rows_times(src, x, t, n, tid, nt);
  __syncthreads();
  if (tid == 0) {
    const double auxOld = sh[0], auxNew = sat_aux_value(t, x, z, scalar, n);
    int decision = kSatUpdated;
    if (auxOld < auxNew) decision = kSatKeptOld;          // sat:322
    else for (int e = 0; e < n; e++) if (x[e] != x[e]) decision = kSatNaN;             // sat:330
    out->kept = shKept; out->decision = decision; out->auxOld = auxOld; out->auxNew = auxNew;
    sh[1] = (double) decision;
  }
  __syncthreads();
  if ((int) sh[1] == kSatUpdated) for (int e = tid; e < n; e += nt) newMean[(long) g * D + nb * n + e] = (float) x[e];
}

void sat_mean_acc(SatHandle& h, const SatCall& c, bool matOnly, hipStream_t st)
{
  const int blp = (c.bl + 3) & ~3;
  const size_t lds = ((size_t) blp * c.bl + blp + 256) * sizeof(double) + (size_t) kSatTileG * blp * sizeof(float);
  ScopedTimer tm(h.timing, st);
  launch(matOnly ? k_sat_mean_acc<false> : k_sat_mean_acc<true>, dim3(c.nTiles, cdiv(c.NCp, kSatColGroup), c.nB), dim3(256), lds, st, c.nSlots, c.NC, c.nB, c.bl, h.D, h.G, c.PZ, c.NCp, h.d_ivar.p,
         h.d_c.p, h.d_sumO.p, h.d_A.p, h.d_b.p, h.d_gidx.p, h.d_tile.p, h.d_pq.p, h.d_macc.p, h.d_mocc.p, h.d_has.p);
  h.ms[0] = tm.stop();
}

void sat_var_acc(SatHandle& h, const SatCall& c, hipStream_t st)
{
  ScopedTimer tm(h.timing, st);
  launch(k_sat_var_acc, dim3(cdiv((long) (c.g1 - c.g0) * h.D, 256)), dim3(256), 0, st, c.nSlots, c.NC, c.nB, c.bl, h.D, h.G, c.g0, c.g1, h.d_mean.p, h.d_c.p,
         h.d_sumO.p, h.d_sumOsq.p, h.d_A.p, h.d_b.p, h.d_kind.p, h.d_bsz.p, h.d_cls.p, h.d_vvec.p, h.d_vocc.p, h.keepTrn ? h.d_trn.p : nullptr);
  h.ms[1] = tm.stop();
}

void sat_solve(SatHandle& h, int nSolve, hipStream_t st)
{
  const int n = h.bl, m = (n + 1) & ~1;
  const size_t lds = ((size_t) 2 * n * n + 3 * n + m + 2 * kSolveThreads) * sizeof(double);
  ScopedTimer tm(h.timing, st);
  launch(k_sat_solve, dim3(nSolve * h.nBlocks), dim3(kSolveThreads), lds, st, h.nBlocks, n, h.D, h.d_solve.p, h.d_macc.p, h.d_mean.p, h.d_newMean.p, h.d_sol.p, h.d_rec.p);
  h.ms[2] = tm.stop();
}

}  // namespace dsr
