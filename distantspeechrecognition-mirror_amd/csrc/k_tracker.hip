// csrc/k_tracker.hip -- the spherical-array speaker trackers of btk/beamformer/tracker.{h,cc}: ModalDecomposition, SpatialDecomposition,
// ModalSphericalArrayTracker, SpatialSphericalArrayTracker (an iterated extended Kalman filter in square-root form on (theta, phi)) and
// PlaneWaveSimulator.  Line numbers are tracker.cc's.
//
// Host side (the set-up work, the dsr_trk_* / dsr_pws_* entries): csrc/tracker.cpp; what the two share: csrc/tracker.h.
//
// Device side, a batch X [U][32][Tmax][M/2+1] complex64 (the layout dsr_fb_analysis writes):
//   k_trk_run   one workgroup per utterance, the frames in order (the filter is sequential in time); within a frame the work is spread over
//               bins, modes / channels and the rows of the realified observation.  All arithmetic fp64, built without FMA contraction.
//               Per local iteration: the harmonics and their derivatives at the current angles, g and its derivatives per bin, B per bin
//               (estimateBkl), the useSubbandsN bins of largest |B| (ties: lower bin first), linearize / predictedObservation / residual,
//               then _update: the Givens sweep of _lowerTriangularize (:1185-1250) streamed one A11 column at a time.  Column j of the
//               prearray's first block column is touched only at step j of the sweep, where it mixes with the two A12 columns over the rows
//               >= j; it is then final and the column-oriented forward substitution uses it at once, so the dense (2N+2) x (2N+4) array
//               never exists: LDS holds the two A12 columns and the innovation, a thread holds the working column's entries of its rows,
//               and a step costs one barrier (the pivot row's owner computes both rotations and A11^-1 r's entry and broadcasts them).
//               The rotation order and every operand are the reference's.
//   k_pws_apply PlaneWaveSimulator::next (:1474-1488) element-wise: coefficient x source spectrum, optionally the conjugate mirror.
#include "launch.h"
#include "tracker.h"
#include "dev_math.h"
#include <algorithm>

using namespace dsr;

namespace {

constexpr int NT = 256;
constexpr size_t LDS_BUDGET = 160 * 1024;                    // per workgroup on gfx950
constexpr double EPSILON = 0.01, TOLERANCE = 1.0e-04;        // _Epsilon, _Tolerance (:878-879)

// the kernel's LDS in doubles: per-mode tables 8 modesN, the spatial kind's per-(sensor, order) sums 6 x 32 x (orderN+1), the reduction
// scratch NT, 32 of pivots and scalars, the selected bins (K ints), then three columns of 2N+2 rows (two of A12 | A22, the innovation)
size_t lds_fixed_doubles(int modesN, int orderN, int spatial, int K) { return 8 * (size_t) modesN + (spatial ? 6 * CHAN * (size_t) (orderN + 1) : 0) + NT + 32 + (size_t) (K + 1) / 2 + 1; }

struct TrkP {
  int spatial, orderN, modesN, F, L, K, N, maxLocalN, Tmax, hasV;
  double su, sv;
  const double2* bn; const double2* sc; const double* norm; const double* absbn; const double* Vt;
};

__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }

// the sum of every thread's v in a fixed tree (the same for every launch shape); all threads get it
__device__ double block_sum(double v, double* red)
{
  const int tid = threadIdx.x;
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = NT / 2; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
  return red[0];
}

// _calcGivensRotation (:1044-1059); false where the norm is zero (the reference throws)
__device__ __forceinline__ bool givens(double v1, double v2, double& c, double& s, double& norm)
{
  norm = sqrt(v1 * v1 + v2 * v2);
  if (norm == 0.0) return false;
  c = v1 / norm; s = v2 / norm;
  return true;
}

__global__ __launch_bounds__(NT) void k_trk_init(double* state, int U, double th, double ph, double k0, int keepK)
{
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= U) return;
  double* s = state + (size_t) u * STATE_DOUBLES;
  s[0] = th; s[1] = ph;
  if (!keepK) { s[2] = k0; s[3] = 0.0; s[4] = 0.0; s[5] = k0; s[6] = 0.0; s[7] = 0.0; }
}

__global__ __launch_bounds__(NT) void k_trk_run(TrkP p, const float2* __restrict__ X, const int* __restrict__ nframes, double* state,
                                                double* ws, size_t wsStride, float* __restrict__ pos, double* __restrict__ pos64,
                                                int* __restrict__ info)
{
  extern __shared__ double lds[];
  const int tid = threadIdx.x, u = blockIdx.x;
  const int F = p.F, L = p.L, K = p.K, N = p.N, n2 = 2 * N, R = n2 + 2, modesN = p.modesN, O1 = p.orderN + 1;
  // LDS
  double* mY = lds;                                          // [modesN] x (Y, dY/dtheta, dY/dphi) complex, P, dP
  double* mS = mY + 8 * modesN;                              // spatial: [3][32][O1] complex
  double* red = mS + (p.spatial ? 6 * CHAN * O1 : 0);
  double* misc = red + NT;                                   // [0..11] the two pivot slots, [12..] scalars
  int* sel = reinterpret_cast<int*>(misc + 32);
  double* a0 = misc + 32 + (K + 1) / 2 + 1;
  double* a1 = a0 + R;
  double* rr = a1 + R;
  // global work space of this utterance
  double2* Vobs = reinterpret_cast<double2*>(ws + (size_t) u * wsStride);   // [F][L] the observation of every bin
  double2* G = Vobs + (size_t) F * L;                                       // [3][F][L] g, dg/dtheta, dg/dphi
  double2* Bk = G + 3 * (size_t) F * L;                                     // [3][F] B, dB/dtheta, dB/dphi
  double* absB = reinterpret_cast<double*>(Bk + 3 * (size_t) F);            // [F]
  double* st = state + (size_t) u * STATE_DOUBLES;
  const int nf = min(max(nframes[u], 0), p.Tmax);

  double th = st[0], ph = st[1], K00 = st[2], K01 = st[3], K10 = st[4], K11 = st[5], count = st[6];
  bool dead = st[7] != 0.0;

  auto tables = [&](double theta, double phi) {              // the harmonics of every mode at (theta, phi); the spatial kind's sums over m
    __syncthreads();
    const double ct = cos(theta), sn = sin(theta);
    if (tid < modesN) {
      int n = 0; while ((n + 1) * (n + 1) <= tid) n++;
      const Harm h = trk_harm(n, tid - n * n - n, ct, sn, phi, p.norm[tid]);
      double* q = mY + 8 * tid;
      q[0] = h.yr; q[1] = h.yi; q[2] = h.tr; q[3] = h.ti; q[4] = h.pr; q[5] = h.pi; q[6] = h.P; q[7] = h.dP;
    }
    __syncthreads();
    if (p.spatial) {
      for (int i = tid; i < CHAN * O1; i += NT) {            // :846-861: sum_m conj(Y_s) Y, m = -n..n in order
        const int s = i / O1, n = i % O1;
        double2 a = make_double2(0, 0), b = a, c = a;
        for (int idx = n * n; idx < (n + 1) * (n + 1); idx++) {
          const double2 ys = p.sc[idx * CHAN + s]; const double* q = mY + 8 * idx;
          a = cadd(a, cmul(ys, make_double2(q[0], q[1]))); b = cadd(b, cmul(ys, make_double2(q[2], q[3]))); c = cadd(c, cmul(ys, make_double2(q[4], q[5])));
        }
        double2* S = reinterpret_cast<double2*>(mS);
        S[i] = a; S[CHAN * O1 + i] = b; S[2 * CHAN * O1 + i] = c;
      }
      __syncthreads();
    }
  };
  auto gkl = [&](int f, int i, double2& g, double2& gt, double2& gp) {   // calculate_gkl (:750-767 / :838-870) from the tables
    if (!p.spatial) {
      int n = 0; while ((n + 1) * (n + 1) <= i) n++;
      const double2 b = p.bn[f * O1 + n]; const double* q = mY + 8 * i;
      g = cmul(b, make_double2(q[0], q[1])); gt = cmul(b, make_double2(q[2], q[3])); gp = cmul(b, make_double2(q[4], q[5]));
    } else {
      const double2* S = reinterpret_cast<const double2*>(mS);
      g = gt = gp = make_double2(0, 0);
      for (int n = 0; n < O1; n++) {
        const double2 b = p.bn[f * O1 + n];
        g = cadd(g, cmul(b, S[i * O1 + n])); gt = cadd(gt, cmul(b, S[CHAN * O1 + i * O1 + n])); gp = cadd(gp, cmul(b, S[2 * CHAN * O1 + i * O1 + n]));
      }
    }
  };

  for (int t = 0; t < p.Tmax; t++) {
    const size_t o = (size_t) u * p.Tmax + t;
    if (t >= nf || dead) {                                   // beyond the utterance: zeros; after an error: the last position, the error flag
      if (tid == 0) {
        const bool z = t >= nf;
        pos64[2 * o] = z ? 0.0 : th; pos64[2 * o + 1] = z ? 0.0 : ph; pos[2 * o] = z ? 0.f : (float) th; pos[2 * o + 1] = z ? 0.f : (float) ph;
        info[o] = z ? 0 : (1 << 9);
      }
      continue;
    }
    // the frame's observations: the snapshot itself, or its transform by the stored conjugate harmonics (:680-691); they do not depend on the state
    __syncthreads();
    for (int i = tid; i < F * L; i += NT) {
      const int f = i / L, l = i % L;
      double2 v;
      if (p.spatial) { const float2 x = X[(((size_t) u * CHAN + l) * p.Tmax + t) * F + f]; v = make_double2(x.x, x.y); }
      else {
        v = make_double2(0, 0);
        for (int s = 0; s < CHAN; s++) { const float2 x = X[(((size_t) u * CHAN + s) * p.Tmax + t) * F + f]; v = cadd(v, conj_mul(p.sc[l * CHAN + s], make_double2(x.x, x.y))); }
      }
      Vobs[i] = v;
    }
    double e0 = th, e1 = ph;                                 // _eta_i
    double P00 = 0, P01 = 0, P10 = 0, P11 = 0;               // the A22 block of the last postarray
    int iters = 0; bool clamped = false, failed = false;
    for (int localX = 0; localX < p.maxLocalN; localX++) {
      tables(e0, e1);
      for (int i = tid; i < F * L; i += NT) {
        double2 g, gt, gp; gkl(i / L, i % L, g, gt, gp);
        G[i] = g; G[(size_t) F * L + i] = gt; G[2 * (size_t) F * L + i] = gp;
      }
      __syncthreads();
      const double sn = sin(e0);
      for (int f = tid; f < F; f += NT) {                    // estimateBkl (:636-678 / :775-791)
        double2 eta = make_double2(0, 0), dt = eta, dp = eta; double delta = 0.0;
        for (int l = 0; l < L; l++) {
          const double2 g = G[(size_t) f * L + l], v = Vobs[(size_t) f * L + l];
          eta = cadd(eta, conj_mul(g, v)); delta += g.x * g.x + g.y * g.y;
          if (!p.spatial) { dt = cadd(dt, conj_mul(G[(size_t) F * L + (size_t) f * L + l], v)); dp = cadd(dp, conj_mul(G[2 * (size_t) F * L + (size_t) f * L + l], v)); }
        }
        const double2 B = make_double2(eta.x / delta, eta.y / delta);
        Bk[f] = B; absB[f] = hypot(B.x, B.y);
        if (!p.spatial) {
          double dd = 0.0;                                   // :656-667
          for (int idx = 0; idx < modesN; idx++) {
            int n = 0; while ((n + 1) * (n + 1) <= idx) n++;
            const double norm2 = M_PI * p.norm[idx] * p.absbn[f * O1 + n];
            dd += -32.0 * norm2 * norm2 * mY[8 * idx + 6] * mY[8 * idx + 7] * sn;
          }
          const double d2 = delta * delta;
          Bk[F + f] = make_double2((dt.x * delta - eta.x * dd) / d2, (dt.y * delta - eta.y * dd) / d2);
          Bk[2 * F + f] = make_double2(dp.x / delta, dp.y / delta);
        }
      }
      __syncthreads();
      for (int f = tid; f < F; f += NT) {                    // SubbandList: |B| descending, ties to the lower bin; the first K are kept
        const double af = absB[f]; int rank = 0;
        for (int g = 0; g < F; g++) { const double ag = absB[g]; rank += (ag > af || (ag == af && g < f)) ? 1 : 0; }
        if (rank < K) sel[rank] = f;
      }
      __syncthreads();
      // linearize, predictedObservation, the innovation and the prearray's A12 = Hbar K (:1077-1144), residualBefore
      const double d0 = th - e0, d1 = ph - e1;
      double part = 0.0;
      for (int rc = tid; rc < N; rc += NT) {
        const int k = rc / L, i = rc % L, f = sel[k];
        const size_t gi = (size_t) f * L + i;
        const double2 B = Bk[f], g = G[gi], gt = G[(size_t) F * L + gi], gp = G[2 * (size_t) F * L + gi], v = Vobs[gi];
        double2 H0 = cmul(B, gt), H1 = cmul(B, gp);
        if (!p.spatial) { H0 = cadd(H0, cmul(g, Bk[F + f])); H1 = cadd(H1, cmul(g, Bk[2 * F + f])); }
        const double2 y = cmul(g, B);
        const double er = v.x - y.x, ei = v.y - y.y;
        part += er * er + ei * ei;
        const int nr = 2 * k * L + i, ni = nr + L;
        a0[nr] = (0.0 + H0.x * K00) + H1.x * K10; a1[nr] = (0.0 + H0.x * K01) + H1.x * K11;
        a0[ni] = (0.0 + H0.y * K00) + H1.y * K10; a1[ni] = (0.0 + H0.y * K01) + H1.y * K11;
        rr[nr] = er - ((0.0 + d0 * H0.x) + d1 * H1.x);
        rr[ni] = ei - ((0.0 + d0 * H0.y) + d1 * H1.y);
      }
      if (tid == 0) { a0[n2] = K00; a0[n2 + 1] = K10; a1[n2] = K01; a1[n2 + 1] = K11; rr[n2] = 0.0; rr[n2 + 1] = 0.0; }
      const double before = block_sum(part, red) / N;
      // _lowerTriangularize's first loop, column by column, with the forward substitution and B21 (A11^-1 r) folded in
      const int L2 = 2 * L;
      auto vinit = [&](int n, int j) -> double {             // the prearray's (n, j), n >= j: the selected bins' V blocks on the diagonal
        if (n >= n2 || n / L2 != j / L2) return 0.0;
        if (!p.hasV) return n == j ? p.sv : 0.0;
        return p.Vt[((size_t) sel[j / L2] * L2 + (j % L2)) * L2 + (n % L2)];
      };
      double corr = 0.0;                                     // of the owners of rows 2N, 2N+1: the correction's entry
      for (int j = 0; j < n2; j++) {
        double* slot = misc + 6 * (j & 1);
        if (tid == (j % NT)) {
          double c0 = 0, s0 = 0, c1 = 0, s1 = 0, nrm = 0, w = vinit(j, j);
          bool okp = givens(w, a0[j], c0, s0, nrm);
          if (okp) { w = nrm; a0[j] = 0.0; okp = givens(w, a1[j], c1, s1, nrm); }
          if (okp) { w = nrm; a1[j] = 0.0; }
          slot[0] = c0; slot[1] = s0; slot[2] = c1; slot[3] = s1; slot[4] = okp ? rr[j] / w : 0.0; slot[5] = okp ? 0.0 : 1.0;
        }
        __syncthreads();
        if (slot[5] != 0.0) { failed = true; break; }
        const double c0 = slot[0], s0 = slot[1], c1 = slot[2], s1 = slot[3], x = slot[4];
        int n = tid > j ? tid : tid + ((j - tid) / NT + 1) * NT;   // this thread's first row > j
        for (; n < R; n += NT) {
          double w = vinit(n, j);
          const double v0 = a0[n], w1 = c0 * w + s0 * v0; a0[n] = c0 * v0 - s0 * w;
          const double v1 = a1[n], w2 = c1 * w1 + s1 * v1; a1[n] = c1 * v1 - s1 * w1;
          if (n < n2) rr[n] -= w2 * x; else corr += w2 * x;
        }
      }
      __syncthreads();
      if (!failed) {
        if (tid == (n2 % NT)) misc[12] = corr;
        if (tid == ((n2 + 1) % NT)) misc[13] = corr;
      }
      __syncthreads();
      if (tid == 0 && !failed) {                             // the A22 | A23 loops (:1206-1250), the correction and _checkPhysicalConstraints
        double A[2][4] = {{a0[n2], a1[n2], p.su, 0.0}, {a0[n2 + 1], a1[n2 + 1], 0.0, p.su}};
        bool okp = true; double c, s, nrm;
        auto rot = [&](int rowX, int col) {                  // rotate column `col` into column rowX from row rowX on
          if (!okp) return;
          okp = givens(A[rowX][rowX], A[rowX][col], c, s, nrm);
          if (!okp) return;
          A[rowX][rowX] = nrm; A[rowX][col] = 0.0;
          for (int n = rowX + 1; n < 2; n++) { const double v1 = A[n][rowX], v2 = A[n][col]; A[n][rowX] = c * v1 + s * v2; A[n][col] = c * v2 - s * v1; }
        };
        rot(0, 1);
        rot(0, 2); rot(0, 3); rot(1, 2); rot(1, 3);
        double t0 = e0 + misc[12], t1 = e1 + misc[13], cl = 0.0;
        if (t0 < EPSILON) { t0 = EPSILON; cl = 1.0; } else if (t0 > M_PI - EPSILON) { t0 = M_PI - EPSILON; cl = 1.0; }
        misc[14] = t0; misc[15] = t1; misc[16] = cl; misc[17] = okp ? 0.0 : 1.0;
        misc[18] = A[0][0]; misc[19] = A[0][1]; misc[20] = A[1][0]; misc[21] = A[1][1];
      }
      __syncthreads();
      if (failed || misc[17] != 0.0) { failed = true; break; }
      e0 = misc[14]; e1 = misc[15]; clamped = clamped || misc[16] != 0.0;
      P00 = misc[18]; P01 = misc[19]; P10 = misc[20]; P11 = misc[21];
      iters = localX + 1;
      // residualAfter: the old B with the harmonics (modal, :725-747) / the recomputed g of the selected bins (spatial, :1402-1410) at the new angles
      tables(e0, e1);
      part = 0.0;
      for (int rc = tid; rc < N; rc += NT) {
        const int k = rc / L, i = rc % L, f = sel[k];
        double2 g, gt, gp; gkl(f, i, g, gt, gp);
        const double2 y = cmul(g, Bk[f]), v = Vobs[(size_t) f * L + i];
        const double er = v.x - y.x, ei = v.y - y.y;
        part += er * er + ei * ei;
      }
      const double after = block_sum(part, red) / N;
      if ((before - after) / (before + after) < TOLERANCE) break;
    }
    if (failed) { dead = true; t--; continue; }              // frozen: this frame and the rest report the last position
    th = e0; ph = e1; K00 = P00; K01 = P01; K10 = P10; K11 = P11; count += 1.0;
    if (tid == 0) {
      pos64[2 * o] = th; pos64[2 * o + 1] = ph; pos[2 * o] = (float) th; pos[2 * o + 1] = (float) ph;
      info[o] = iters | (clamped ? 1 << 8 : 0);
    }
  }
  if (tid == 0) { st[0] = th; st[1] = ph; st[2] = K00; st[3] = K01; st[4] = K10; st[5] = K11; st[6] = count; st[7] = dead ? 1.0 : 0.0; }
}

// PlaneWaveSimulator::next (:1474-1488): out = coefficient x source, bins 0..M/2; full: rows of M bins with bin M-k = conj(bin k), 0 < k < M/2
__global__ __launch_bounds__(NT) void k_pws_apply(const double2* __restrict__ coef, int C, const float2* __restrict__ src, const int* __restrict__ nframes,
                                                  int U, int Tmax, int M, int full, float2* __restrict__ out)
{
  const int F = M / 2 + 1, W = full ? M : F;
  const size_t total = (size_t) U * C * Tmax * F;
  for (size_t i = (size_t) blockIdx.x * NT + threadIdx.x; i < total; i += (size_t) gridDim.x * NT) {
    const int f = (int) (i % F); size_t q = i / F;
    const int t = (int) (q % Tmax); q /= Tmax;
    const int c = (int) (q % C), u = (int) (q / C);
    float2 y = make_float2(0.f, 0.f);
    if (t < nframes[u]) {
      const float2 s = src[((size_t) u * Tmax + t) * F + f];
      const double2 v = cmul(coef[(size_t) c * F + f], make_double2(s.x, s.y));
      y = make_float2((float) v.x, (float) v.y);
    }
    float2* row = out + (((size_t) u * C + c) * Tmax + t) * W;
    row[f] = y;
    if (full && f != 0 && f != M / 2) row[M - f] = make_float2(y.x, -y.y);
  }
}

void upload_tables(dsr_trk& s, hipStream_t st)
{
  if (!s.tablesUp) {
    s.dBn.upload(reinterpret_cast<const double2*>(s.bn.data()), s.bn.size(), st);
    s.dSc.upload(reinterpret_cast<const double2*>(s.sc.data()), s.sc.size(), st);
    s.dNorm.upload(s.norm, st); s.dAbs.upload(s.absbn, st);
    s.tablesUp = true;
  }
  if (!s.V.empty() && s.vDirty) {                            // the blocks transposed: a column's rows are contiguous
    const int L2 = 2 * s.L; std::vector<double> Vt(s.V.size());
    for (int f = 0; f < s.F; f++)
      for (int m = 0; m < L2; m++)
        for (int n = 0; n < L2; n++) Vt[((size_t) f * L2 + n) * L2 + m] = s.V[((size_t) f * L2 + m) * L2 + n];
    s.dVt.upload(Vt, st); s.vDirty = false;
  }
}

}  // namespace

namespace dsr {

long trk_max_rows(int modesN, int orderN, int spatial, int K)
{
  return ((long) (LDS_BUDGET / 8) - (long) lds_fixed_doubles(modesN, orderN, spatial, K)) / 3 - 2;
}
size_t trk_lds_bytes(const dsr_trk& s) { return 8 * (lds_fixed_doubles(s.modesN, s.orderN, s.spatial, s.K) + 3 * (size_t) (2 * s.N + 2)); }

void trk_launch_init(double* state, int U, double th, double ph, double k0, int keepK, hipStream_t st)
{
  launch(k_trk_init, dim3(cdiv(U, NT)), dim3(NT), 0, st, state, U, th, ph, k0, keepK);
}

void trk_launch_run(dsr_trk& s, const float* X, const int32_t* nframes, int U, int Tmax, double* state, float* pos, double* pos64, int32_t* info, hipStream_t st)
{
  upload_tables(s, st);
  const size_t FL = (size_t) s.F * s.L, wsStride = (8 * FL + 7 * (size_t) s.F + 1) / 2 * 2;   // doubles, even: the complex tables stay 16-byte aligned
  DevBuf<double>& ws = s.ws.at(st); ws.reserve((size_t) U * wsStride);
  TrkP p;
  p.spatial = s.spatial; p.orderN = s.orderN; p.modesN = s.modesN; p.F = s.F; p.L = s.L; p.K = s.K; p.N = s.N; p.maxLocalN = s.maxLocalN;
  p.Tmax = Tmax; p.hasV = s.V.empty() ? 0 : 1; p.su = std::sqrt(s.s2u); p.sv = std::sqrt(s.s2v);
  p.bn = s.dBn.p; p.sc = s.dSc.p; p.norm = s.dNorm.p; p.absbn = s.dAbs.p; p.Vt = s.dVt.p;
  launch(k_trk_run, dim3(U), dim3(NT), s.lds, st, p, (const float2*) X, nframes, state, ws.p, wsStride, pos, pos64, info);
}

void pws_launch_apply(const double* coef, int C, const float* src, const int32_t* nframes, int U, int Tmax, int M, int full, float* out, hipStream_t st)
{
  const size_t total = (size_t) U * C * Tmax * (M / 2 + 1);
  const int blocks = (int) std::min<size_t>((total + NT - 1) / NT, 65535);
  launch(k_pws_apply, dim3(blocks), dim3(NT), 0, st, (const double2*) coef, C, (const float2*) src, nframes, U, Tmax, M, full, (float2*) out);
}

}  // namespace dsr
