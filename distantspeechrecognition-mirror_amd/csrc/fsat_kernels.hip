// csrc/fsat_kernels.hip -- fast speaker-adaptive training on the device: the fold of a batch of speaker slots into the speaker-independent
// fast accumulators, their addition into the SAT sums, and the MDL mean solve with the joint variance update.
//
// Replaces GaussDensity::normFastAccu (asr/sat/codebookFastSAT.cc:346-418, "cfs"), FastSAT::addFastAcc (asr/sat/sat.cc:530-550, "sat"),
// FastAcc::update / FastSAT::update / _updateVariance (sat:1079-1099, 552-587) and MDLSATMean::update / _solve (sat:395-493), which work on
// one speaker and one Gaussian at a time.  FastSAT::accumulate (sat:501-528) is the kVec = false instantiation of k_sat_mean_acc.
//
//   k_fsat_norm   per (tile of 16 Gaussians of one class, block nb): the slots in order, a slot's block matrix staged once in LDS (row stride
//                 bl | 1: a lane reads a column for the mat-vec and a row for transform(origMean), both without bank conflicts).  Per slot the
//                 workgroup forms v = sumO - ck b and the scalar terms iv v v / ck of its 16 x bl entries in LDS (sumO is read once); then
//                 every output -- fastMean[p], fastVar[p], scalar, the two counts -- belongs to one lane, which keeps its running value in
//                 registers over the slots and writes it once.  fastMean[p] += sum_m v[m] (A[m][p] iv[m]) in m order from 0.0, rows with
//                 v[m] == 0 skipped, as gsl_matrix_set(temp1 ..) + gsl_blas_dgemv(CblasTrans) do; fastVar with the code k_sat_var_acc uses
//                 (sat_dev.h).  Sequential fp64 in the reference's order: bit for bit, no atomics.
//   k_fsat_add    thread per (Gaussian, component): vec += fastMean, varVec += fastVar, scalar += fastScalar; the blocks count as allocated.
//   k_fsat_solve  workgroup per (Gaussian, block): the variances first (varVec / occ, a NaN keeps 1 / var; 1 / var under meanOnly), then
//                 auxOld = aux(mean) + thr descLen, the Jacobi of mllr_jacobi.h to M = V diag(l) V^T, t = V^T vec, lmax over the signed l from
//                 0.0 (sat:474-477), component k kept when 0.5 t_k^2 / l_k > thr and l_k / lmax >= 1e-7, x = V t', auxNew = aux(x) + thr kept
//                 with mat re-read from memory, the decision of sat:439; one record and one description length per (Gaussian, block).
// This translation unit is compiled with -ffp-contract=off.
#include "launch.h"
#include "fsat.h"
#include "sat_dev.h"
#include "train.h"
#include <cmath>

namespace dsr {

static constexpr int kSolveThreads = 128;

// num / den: numProb and denProb of a trainer's accumulator rows [sumO (D) | sumOsq (D) | count | denCount | ..]
__global__ __launch_bounds__(256) void k_fsat_take(const double* __restrict__ acc, int G, int D, double* __restrict__ num, double* __restrict__ den)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  const double* row = acc + (long) g * (2 * D + 4);
  num[g] = row[2 * D]; den[g] = row[2 * D + 1];
}

// tile[3 t] = { class index, first sorted Gaussian, Gaussians }; tables [slot][class]; cnt = num - den as the slot holds it
__global__ __launch_bounds__(256) void k_fsat_norm(int nSlots, int NC, int nB, int bl, int D, int G, const float* __restrict__ mean, const float* __restrict__ ivar,
                                                   const double* __restrict__ cnt, const double* __restrict__ num, const double* __restrict__ den,
                                                   const double* __restrict__ sumO, const double* __restrict__ sumOsq, const double* __restrict__ Atab,
                                                   const double* __restrict__ btab, const int* __restrict__ kind, const int* __restrict__ bsz,
                                                   const int* __restrict__ gidx, const int* __restrict__ tile, double* fcount, double* fden, double* fmean,
                                                   double* fvar, double* fscalar, int* flag)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ int sg[kSatTileG], live[kSatTileG]; __shared__ double cks[kSatTileG], nums[kSatTileG], dens[kSatTileG];
  const int lda = bl | 1, tid = threadIdx.x, nt = blockDim.x, W = bl + 2, nE = kSatTileG * bl;
  double* As = reinterpret_cast<double*>(smem);           // [bl][lda]: the slot's block matrix
  double* bs = As + bl * lda;                             // [bl]: its offsets
  double* vs = bs + bl;                                   // [16][bl]: sumO - ck b
  double* ts = vs + nE;                                   // [16][bl]: iv v v / ck
  double* sos = ts + nE;                                  // [16][bl]: sumO
  float* ivs = reinterpret_cast<float*>(sos + nE);        // [16][bl]
  float* mus = ivs + nE;                                  // [16][bl]
  const int t = blockIdx.x, nb = blockIdx.y, off = nb * bl;
  const int cls = tile[3 * t], i0 = tile[3 * t + 1], n = tile[3 * t + 2];
  if (tid < kSatTileG) sg[tid] = tid < n ? gidx[i0 + tid] : -1;
  __syncthreads();
  for (int e = tid; e < nE; e += nt) {
    const int j = e / bl, m = e - j * bl, g = sg[j];
    ivs[e] = g >= 0 ? ivar[(long) g * D + off + m] : 0.0f; mus[e] = g >= 0 ? mean[(long) g * D + off + m] : 0.0f;
  }
  // job e = (Gaussian j, p): p < bl fastMean and fastVar of component off + p; p == bl the scalar of the block; p == bl + 1 the two counts
  double accM[kFsatJobs], accV[kFsatJobs];
#pragma unroll
  for (int i = 0; i < kFsatJobs; i++) {
    const int e = tid + i * 256; accM[i] = 0.0; accV[i] = 0.0;
    if (e >= kSatTileG * W) continue;
    const int j = e / W, p = e - j * W, g = sg[j];
    if (g < 0) continue;
    if (p < bl) { accM[i] = fmean[(long) g * D + off + p]; accV[i] = fvar[(long) g * D + off + p]; }
    else if (p == bl) accM[i] = fscalar[(long) g * nB + nb];
    else if (nb == 0) { accM[i] = fcount[g]; accV[i] = fden[g]; }
  }
  for (int s = 0; s < nSlots; s++) {
    __syncthreads();
    const long tab = (long) s * NC + cls;
    const double* A = Atab + (tab * nB + nb) * bl * bl;
    for (int e = tid; e < bl * bl; e += nt) { const int r = e / bl; As[r * lda + (e - r * bl)] = A[e]; }
    for (int e = tid; e < bl; e += nt) bs[e] = btab[tab * D + off + e];
    if (tid < kSatTileG) {
      const int g = sg[tid]; double ck = 0.0, nm = 0.0, dn = 0.0; int lv = 0;
      if (g >= 0) {
        nm = num[(long) s * G + g]; dn = den[(long) s * G + g]; ck = cnt[(long) s * G + g];
        if (!(nm == 0.0 && dn == 0.0)) lv = fabs(ck) < kFsatSmallCk ? 1 : 2;             // cfs:348, 368
      }
      cks[tid] = ck; nums[tid] = nm; dens[tid] = dn; live[tid] = lv;
    }
    __syncthreads();
    for (int e = tid; e < nE; e += nt) {
      const int j = e / bl, m = e - j * bl;
      double v = 0.0, so = 0.0, term = 0.0;
      if (live[j] == 2) {
        so = sumO[((long) s * G + sg[j]) * D + off + m];
        v = __dsub_rn(so, __dmul_rn(cks[j], bs[m]));                                      // cfs:391-393
        term = __ddiv_rn(__dmul_rn(__dmul_rn((double) ivs[e], v), v), cks[j]);            // cfs:404-405
      }
      vs[e] = v; sos[e] = so; ts[e] = term;
    }
    __syncthreads();
    const int kd = kind[tab], bz = bsz[tab];
#pragma unroll
    for (int i = 0; i < kFsatJobs; i++) {
      const int e = tid + i * 256;
      if (e >= kSatTileG * W) continue;
      const int j = e / W, p = e - j * W, g = sg[j];
      if (g < 0 || live[j] == 0) continue;
      if (p == bl + 1) { accM[i] = __dadd_rn(accM[i], nums[j]); accV[i] = __dadd_rn(accV[i], dens[j]); continue; }   // cfs:365-366
      if (live[j] != 2) continue;
      if (p == bl) { for (int m = 0; m < bl; m++) accM[i] = __dadd_rn(accM[i], ts[j * bl + m]); continue; }
      double y = 0.0;                                     // dgemv(CblasTrans), beta = 0: cfs:383-394
      for (int m = 0; m < bl; m++) {
        const double v = vs[j * bl + m];
        if (v != 0.0) y = __dadd_rn(y, __dmul_rn(v, __dmul_rn(As[m * lda + p], (double) ivs[j * bl + m])));
      }
      accM[i] = __dadd_rn(accM[i], y);                    // cfs:397-399
      const float comp = sat_transform_comp(kd, off + p < bz, bs[p], As + p * lda, mus + j * bl, bl);
      accV[i] = sat_var_term(accV[i], sumOsq[((long) s * G + g) * D + off + p], sos[j * bl + p], (double) comp, cks[j]);   // cfs:410-414
    }
  }
#pragma unroll
  for (int i = 0; i < kFsatJobs; i++) {
    const int e = tid + i * 256;
    if (e >= kSatTileG * W) continue;
    const int j = e / W, p = e - j * W, g = sg[j];
    if (g < 0) continue;
    if (p < bl) { fmean[(long) g * D + off + p] = accM[i]; fvar[(long) g * D + off + p] = accV[i]; }
    else if (p == bl) { fscalar[(long) g * nB + nb] = accM[i]; if (accM[i] != accM[i]) flag[0] = 1; }
    else if (nb == 0) { fcount[g] = accM[i]; fden[g] = accV[i]; }
  }
}

// FastSAT::addFastAcc (sat:530-550) of the Gaussians [g0, g1)
__global__ __launch_bounds__(256) void k_fsat_add(int nB, int bl, int D, int g0, int g1, const double* __restrict__ fmean, const double* __restrict__ fvar,
                                                  const double* __restrict__ fscalar, double* __restrict__ macc, double* __restrict__ vvec,
                                                  int* __restrict__ has, int* __restrict__ flag)
{
  const long idx = (long) blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long) (g1 - g0) * D) return;
  const int g = g0 + (int) (idx / D), k = (int) (idx - (long) (g - g0) * D), nb = k / bl, n = k - nb * bl;
  double* base = macc + ((long) g * nB + nb) * ((long) bl * bl + bl + 1);
  base[bl * bl + n] = __dadd_rn(base[bl * bl + n], fmean[(long) g * D + k]);
  vvec[(long) g * D + k] = __dadd_rn(vvec[(long) g * D + k], fvar[(long) g * D + k]);
  if (n == 0) { const double sc = __dadd_rn(base[bl * bl + bl], fscalar[(long) g * nB + nb]); base[bl * bl + bl] = sc; if (sc != sc) flag[0] = 1; }
  if (k == 0) has[g] = 1;
}

// solve[k]: the Gaussian; one workgroup per (k, block).  ivar: the covariance slot as it stands (inverse variances); desc [G][nB]
__global__ __launch_bounds__(kSolveThreads) void k_fsat_solve(int nB, int bl, int D, double thr, int meanOnly, const int* __restrict__ solve,
                                                              const double* __restrict__ macc, const double* __restrict__ mocc, const double* __restrict__ vvec,
                                                              const float* __restrict__ mean, const float* __restrict__ ivar, const int* __restrict__ desc,
                                                              float* __restrict__ newMean, float* __restrict__ newVar, double* __restrict__ sol,
                                                              SatRecord* __restrict__ rec, int* __restrict__ newDesc)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ double sh[2]; __shared__ int shKept;
  const int n = bl, m = (n + 1) & ~1, nt = blockDim.x, tid = threadIdx.x;
  double* a = reinterpret_cast<double*>(smem);            // [n][n]
  double* v = a + n * n;                                  // [n][n]
  double* z = v + n * n;                                  // [n] vec
  double* t = z + n;                                      // [n]
  double* x = t + n;                                      // [n] the mean, then the solution
  double* cs = x + n;                                     // [m]: the rotations, then which components are kept
  double* sq = cs + m;                                    // [2 nt]
  const int g = solve[blockIdx.x / nB], nb = blockIdx.x % nB;
  const long stride = (long) n * n + n + 1;
  const double* src = macc + ((long) g * nB + nb) * stride;
  const double scalar = src[n * n + n], occ = mocc[g];
  const int dl = desc[(long) g * nB + nb];
  for (int e = tid; e < n * n; e += nt) { a[e] = src[e]; v[e] = (e / n == e % n) ? 1.0 : 0.0; }
  for (int e = tid; e < n; e += nt) {
    const long k = (long) g * D + nb * n + e;
    z[e] = src[n * n + e]; x[e] = (double) mean[k];
    const double cur = (double) ivar[k]; double nv = __ddiv_rn(1.0, cur);                  // sat:555-558, 581
    if (!meanOnly) { const double var = __ddiv_rn(vvec[k], occ); if (var == var) nv = var; }      // sat:577-584
    newVar[k] = (float) nv;
  }
  __syncthreads();
  sat_rows_times(a, x, t, n, tid, nt);
  __syncthreads();
  if (tid == 0) sh[0] = __dadd_rn(sat_aux_value(t, x, z, scalar, n), __dmul_rn(thr, (double) dl));     // sat:424-426
  __syncthreads();
  bool ok = sat_jacobi(a, v, n, m, cs, sq, tid, nt);
  for (int e = tid; e < n; e += nt) if (!(fabs(z[e]) <= 1.7E308)) ok = false;
  if (!(fabs(scalar) <= 1.7E308)) ok = false;
  ok = __syncthreads_and(ok);
  SatRecord* out = rec + (long) g * nB + nb;
  if (!ok) { if (tid == 0) { out->kept = 0; out->decision = kSatFlagged; out->auxOld = sh[0]; out->auxNew = 0.0; newDesc[(long) g * nB + nb] = dl; } return; }
  double lmax = 0.0;                                      // sat:474-477: the largest eigenvalue, from 0.0
  for (int e = 0; e < n; e++) { const double l = a[e * n + e]; if (l > lmax) lmax = l; }
  for (int e = tid; e < n; e += nt) {
    double sum = 0.0;
    for (int j = 0; j < n; j++) sum = __dadd_rn(sum, __dmul_rn(v[j * n + e], z[j]));
    const double l = a[e * n + e];
    const double contrib = __dmul_rn(0.5, __ddiv_rn(__dmul_rn(sum, sum), l));              // sat:482
    const bool keep = contrib > thr && __ddiv_rn(l, lmax) >= 1.0e-07;                      // sat:483
    t[e] = keep ? __ddiv_rn(sum, l) : 0.0; cs[e] = keep ? 1.0 : 0.0;
  }
  __syncthreads();
  if (tid == 0) { int kept = 0; for (int e = 0; e < n; e++) if (cs[e] != 0.0) kept++; shKept = kept; }
  for (int e = tid; e < n; e += nt) {
    double sum = 0.0;
    for (int j = 0; j < n; j++) sum = __dadd_rn(sum, __dmul_rn(v[e * n + j], t[j]));
    x[e] = sum; sol[(long) g * D + nb * n + e] = sum;
  }
  __syncthreads();
  sat_rows_times(src, x, t, n, tid, nt);                  // mat again, from memory: a holds its eigenvalues now
  __syncthreads();
  if (tid == 0) {
    const double auxOld = sh[0], auxNew = __dadd_rn(sat_aux_value(t, x, z, scalar, n), __dmul_rn(thr, (double) shKept));   // sat:430-432
    int decision = kSatUpdated;
    if (auxOld < auxNew) decision = kSatKeptOld;          // sat:439
    else for (int e = 0; e < n; e++) if (x[e] != x[e]) decision = kSatNaN;             // sat:449
    out->kept = shKept; out->decision = decision; out->auxOld = auxOld; out->auxNew = auxNew;
    newDesc[(long) g * nB + nb] = decision == kSatUpdated ? shKept : dl;                   // sat:445-446
    sh[1] = (double) decision;
  }
  __syncthreads();
  if ((int) sh[1] == kSatUpdated) for (int e = tid; e < n; e += nt) newMean[(long) g * D + nb * n + e] = (float) x[e];
}

void fsat_take_counts(FsatHandle& f, int s, const dsr_train& t)
{
  if (t.G != f.G || t.D != f.D) throw Error(DSR_E_DIMENSION, "accumulators of %d Gaussians x %d for a model of %d x %d", t.G, t.D, f.G, f.D);
  launch(k_fsat_take, dim3(cdiv(f.G, 256)), dim3(256), 0, nullptr, t.d_acc.p, f.G, f.D, f.d_num.p + (size_t) s * f.G, f.d_den.p + (size_t) s * f.G);
  DSR_HIP(hipDeviceSynchronize());
}

void fsat_norm(FsatHandle& f, const SatCall& c, hipStream_t st)
{
  SatHandle& h = *f.sat; const int bl = c.bl, lda = bl | 1;
  const size_t lds = ((size_t) bl * lda + bl + 3 * (size_t) kSatTileG * bl) * sizeof(double) + 2 * (size_t) kSatTileG * bl * sizeof(float);
  ScopedTimer tm(h.timing, st);
  launch(k_fsat_norm, dim3(c.nTiles, c.nB), dim3(256), lds, st, c.nSlots, c.NC, c.nB, bl, h.D, h.G, h.d_mean.p, h.d_ivar.p, h.d_c.p, f.d_num.p, f.d_den.p,
         h.d_sumO.p, h.d_sumOsq.p, h.d_A.p, h.d_b.p, h.d_kind.p, h.d_bsz.p, h.d_gidx.p, h.d_tile.p, f.d_fcount.p, f.d_fden.p, f.d_fmean.p, f.d_fvar.p,
         f.d_fscalar.p, f.d_flag.p);
  f.ms[0] = tm.stop();
}

void fsat_add(FsatHandle& f, hipStream_t st)
{
  SatHandle& h = *f.sat; int g0, g1; sat_part_gaussians(h, g0, g1);
  if (g0 == g1) return;
  launch(k_fsat_add, dim3(cdiv((long) (g1 - g0) * h.D, 256)), dim3(256), 0, st, h.nBlocks, h.bl, h.D, g0, g1, f.d_fmean.p, f.d_fvar.p, f.d_fscalar.p, h.d_macc.p,
         h.d_vvec.p, h.d_has.p, f.d_flag.p);
}

void fsat_solve(FsatHandle& f, int nSolve, hipStream_t st)
{
  SatHandle& h = *f.sat; const int n = h.bl, m = (n + 1) & ~1;
  const size_t lds = ((size_t) 2 * n * n + 3 * n + m + 2 * kSolveThreads) * sizeof(double);          // the LDS of k_sat_solve
  ScopedTimer tm(h.timing, st);
  launch(k_fsat_solve, dim3(nSolve * h.nBlocks), dim3(kSolveThreads), lds, st, h.nBlocks, n, h.D, f.lhoodThreshold, f.meanOnly ? 1 : 0, h.d_solve.p, h.d_macc.p,
         h.d_mocc.p, h.d_vvec.p, h.d_mean.p, h.d_ivar.p, f.d_desc.p, h.d_newMean.p, f.d_newVar.p, h.d_sol.p, h.d_rec.p, f.d_newDesc.p);
  f.ms[2] = tm.stop();
}

}  // namespace dsr
