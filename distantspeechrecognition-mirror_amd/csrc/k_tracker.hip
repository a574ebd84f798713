// csrc/k_tracker.hip -- the spherical-array speaker trackers of btk/beamformer/tracker.{h,cc}: ModalDecomposition, SpatialDecomposition,
// ModalSphericalArrayTracker, SpatialSphericalArrayTracker (an iterated extended Kalman filter in square-root form on (theta, phi)) and
// PlaneWaveSimulator.  Line numbers are tracker.cc's.
//
// Host side (set-up work, as in the reference): the EigenMike geometry (:195-297, the table of csrc/sph_math.h), _bn = 4 pi i^n b_n(ka) with
// modalCoefficient's own closed forms (:474-628), the conjugated harmonics at the sensors (:117-130), _calculateNormalization per mode, the
// per-bin observation-noise Cholesky blocks (setV :961-981) and the plane-wave coefficients (:1453-1465).
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
#include "sph_math.h"
#include "dev_math.h"
#include <algorithm>

using namespace dsr;

typedef std::complex<double> zc;

namespace {

constexpr double SSPEED = 343740.0;                          // BaseDecomposition::_SpeedOfSound (:86)
constexpr int CHAN = 32;                                     // _ChannelsN (:85)
constexpr int MAX_ORDER_N = 8;                               // 81 modes: the per-mode tables of the kernel
constexpr int STATE_DOUBLES = 8;                             // theta, phi, K (row major), frames seen, error flag
constexpr int NT = 256;
constexpr size_t LDS_BUDGET = 160 * 1024;                    // per workgroup on gfx950
constexpr double EPSILON = 0.01, TOLERANCE = 1.0e-04;        // _Epsilon, _Tolerance (:878-879)

// _calculatePnm (:421-437): the unnormalised Legendre function with the negative-degree scaling loop; x = cos(theta)
DSR_HD inline double trk_pnm(int order, int degree, double x)
{
  double result = legendre_plm(order, degree < 0 ? -degree : degree, x);
  if (degree < 0) {
    int m = -degree; double factor = 1.0;
    while (m > degree) { factor *= (order + m); m--; }
    result /= factor;
    if (((-degree) % 2) == 1) result *= -1;
  }
  return result;
}
// _calculate_dPnm_dtheta (:440-449): dP/dx in fact; the (degree - order - 1) factor is kept for negative degree, as written
DSR_HD inline double trk_dpnm(int order, int degree, double x)
{
  const double x2 = x * x;
  return ((degree - order - 1) * trk_pnm(order + 1, degree, x) + (order + 1) * x * trk_pnm(order, degree, x)) / (1.0 - x2);
}
// _calculateNormalization (:381-403)
double trk_norm(int order, int degree)
{
  double norm = std::sqrt((2 * order + 1) / (4.0 * M_PI)), factor = 1.0;
  if (degree >= 0) { int m = degree; while (m > -degree) { factor *= (order + m); m--; } norm /= std::sqrt(factor); }
  else { int m = -degree; while (m > degree) { factor *= (order + m); m--; } norm *= std::sqrt(factor); }
  return norm;
}
// harmonic (:319-339) and the two derivatives (:452-472) from cos / sin of theta and the mode's normalisation: host and device
struct Harm { double yr, yi, tr, ti, pr, pi, P, dP; };
DSR_HD inline Harm trk_harm(int n, int m, double ct, double st, double phi, double norm)
{
  Harm h;
  double p = sph_plm(n, m >= 0 ? m : -m, ct);
  if (m < 0 && ((-m) % 2) == 1) p = -p;
  const double ang = -m * phi, er = cos(ang), ei = sin(ang);
  h.yr = er * p; h.yi = ei * p;
  h.P = trk_pnm(n, m, ct); h.dP = trk_dpnm(n, m, ct);
  const double factor = -norm * h.dP * st;
  h.tr = er * factor; h.ti = ei * factor;
  const double qr = h.yr * 0.0 - h.yi * -1.0, qi = h.yr * -1.0 + h.yi * 0.0;    // gsl_complex_mul(Ynm, (0, -1))
  h.pr = qr * m; h.pi = qi * m;
  return h;
}

zc modal_coefficient(unsigned order, double ka)              // :474-628
{
  if (ka == 0.0) return zc(1.0, 0.0);
  const double c = std::cos(ka), s = std::sin(ka);
  const double ka2 = ka * ka, ka3 = ka2 * ka, ka4 = ka2 * ka2, ka5 = ka4 * ka, ka6 = ka5 * ka, ka7 = ka6 * ka, ka8 = ka7 * ka, ka9 = ka8 * ka;
  auto mul_imag = [](zc a, double y) { return zc(-y * a.imag(), y * a.real()); };
  switch (order) {
  case 0: {
    const double j0 = gsinc(ka / M_PI);
    const zc h0(j0, -c / ka);
    const double val1 = ka * c - s;
    const zc val2 = gmul(zc(ka, 1), zc(c, s));
    const zc grad = gdiv(zc(val1, 0), val2), g = gmul(grad, h0);
    return zc(j0 - g.real(), 0.0 - g.imag());
  }
  case 1: return gmulr(gdiv(zc(-c, s), zc(ka2 - 2, 2 * ka)), ka);
  case 2: return mul_imag(gdiv(zc(c, -s), zc(ka3 - 9 * ka, 4 * ka2 - 9)), ka2);
  case 3: return gmulr(gdiv(zc(c, -s), zc(ka4 - 27 * ka2 + 60, 7 * ka3 - 60 * ka)), ka3);
  case 4: return gmulr(gdiv(zc(s, c), zc(ka5 - 65 * ka3 + 525 * ka, 11 * ka4 - 240 * ka2 + 525)), ka4);
  case 5: return gmulr(gdiv(zc(c, -s), zc(ka6 - 135 * ka4 + 2625 * ka2 - 5670, 16 * ka5 - 735 * ka3 + 5670 * ka)), ka5);
  case 6: return mul_imag(gdiv(zc(c, -s), zc(ka7 - 252 * ka5 + 9765 * ka3 - 72765 * ka, 22 * ka6 - 1890 * ka4 + 34020 * ka2 - 72765)), ka6);
  case 7: return gmulr(gdiv(zc(c, -s), zc(1081080 - 509355 * ka2 + 29925 * ka4 - 434 * ka6 + ka8, -1081080 * ka + 148995 * ka3 - 4284 * ka5 + 29 * ka7)), ka7);
  case 8: return gmulr(gdiv(zc(s, c), zc(18243225 * ka - 2567565 * ka3 + 79695 * ka5 - 702 * ka7 + ka9,
                                         18243225 - 8648640 * ka2 + 530145 * ka4 - 8820 * ka6 + 37 * ka8)), ka8);
  default: {
    const double jn = sph_jl(order, ka), yn = sph_yl(order, ka);
    const double jp = sph_jl(order - 1, ka), jnn = sph_jl(order + 1, ka), yp = sph_yl(order - 1, ka), ynn = sph_yl(order + 1, ka);
    const double djn = (jp - jnn) / 2;
    const zc hn(jn, yn), hp(jp, yp), hnn(jnn, ynn);
    const zc val = gdivr(hn + gmulr(hnn, ka), ka);
    const zc dhn = gmulr(hp - val, 0.5);
    const zc grad = gdiv(zc(djn, 0), dhn), g = gmul(grad, hn);
    return zc(-g.real() + jn, -g.imag());
  }
  }
}

zc host_harmonic(int n, int m, double theta, double phi)
{
  const Harm h = trk_harm(n, m, std::cos(theta), std::sin(theta), phi, trk_norm(n, m));
  return zc(h.yr, h.yi);
}

}  // namespace

struct dsr_trk {
  int spatial = 0, orderN = 0, modesN = 1, M = 0, F = 0, K = 0, L = 0, N = 0, maxLocalN = 1;
  double a = 0, fs = 0, s2u = 10, s2v = 10, s2init = 10, th0 = 0.5, ph0 = 0.0;
  std::vector<zc> bn, sc;                                    // _bn [F][orderN+1]; _sphericalComponent [modesN][32] = conj(Y) at the sensors
  std::vector<double> norm, absbn;                           // [modesN]; |_bn| [F][orderN+1]
  std::vector<double> V; bool vDirty = true;                 // setV's blocks [F][2L][2L] (empty until the first setV: sqrt(sigma2_v) I)
  DevBuf<double2> dBn, dSc; DevBuf<double> dNorm, dAbs, dVt; bool tablesUp = false;
  PerStream<DevBuf<double>> ws;
  size_t lds = 0;
};

namespace {

// the kernel's LDS in doubles: per-mode tables 8 modesN, the spatial kind's per-(sensor, order) sums 6 x 32 x (orderN+1), the reduction
// scratch NT, 32 of pivots and scalars, the selected bins (K ints), then three columns of 2N+2 rows (two of A12 | A22, the innovation)
size_t lds_fixed_doubles(int modesN, int orderN, int spatial, int K) { return 8 * (size_t) modesN + (spatial ? 6 * CHAN * (size_t) (orderN + 1) : 0) + NT + 32 + (size_t) (K + 1) / 2 + 1; }
size_t lds_bytes(const dsr_trk& s) { return 8 * (lds_fixed_doubles(s.modesN, s.orderN, s.spatial, s.K) + 3 * (size_t) (2 * s.N + 2)); }
long max_rows(int modesN, int orderN, int spatial, int K)      // the largest 2N the LDS budget admits
{
  return ((long) (LDS_BUDGET / 8) - (long) lds_fixed_doubles(modesN, orderN, spatial, K)) / 3 - 2;
}

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

extern "C" {

dsr_status dsr_trk_create(int kind, int orderN, int fftLen, double a, double sampleRate, int useSubbandsN, double sigma2_u, double sigma2_v, double sigma2_init,
                          int maxLocalN, int chanN, dsr_trk** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_ARG, "out is null");
    *out = nullptr;
    if (chanN != CHAN) throw Error(DSR_E_ARG, "the trackers are built for the EigenMike's %d channels, not %d", CHAN, chanN);
    if (kind != DSR_TRK_MODAL && kind != DSR_TRK_SPATIAL) throw Error(DSR_E_ARG, "kind %d: DSR_TRK_MODAL or DSR_TRK_SPATIAL", kind);
    if (orderN < 0 || orderN > MAX_ORDER_N) throw Error(DSR_E_ARG, "orderN %d outside [0, %d]", orderN, MAX_ORDER_N);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_ARG, "fftLen %d: an even length >= 2", fftLen);
    const int F = fftLen / 2 + 1;
    if (useSubbandsN < 0 || useSubbandsN > F) throw Error(DSR_E_ARG, "useSubbandsN %d outside [0, %d]", useSubbandsN, F);
    if (maxLocalN < 1 || maxLocalN > 255) throw Error(DSR_E_ARG, "maxLocalN %d outside [1, 255]", maxLocalN);
    if (!(sigma2_u >= 0.0) || !(sigma2_v >= 0.0) || !(sigma2_init >= 0.0)) throw Error(DSR_E_ARG, "negative variance");
    std::unique_ptr<dsr_trk> s(new dsr_trk());
    s->spatial = kind == DSR_TRK_SPATIAL; s->orderN = orderN; s->modesN = (orderN + 1) * (orderN + 1); s->M = fftLen; s->F = F;
    s->K = useSubbandsN == 0 ? F : useSubbandsN; s->L = s->spatial ? CHAN : s->modesN; s->N = s->K * s->L; s->maxLocalN = maxLocalN;
    s->a = a; s->fs = sampleRate; s->s2u = sigma2_u; s->s2v = sigma2_v; s->s2init = sigma2_init;
    const long lim = max_rows(s->modesN, orderN, s->spatial, s->K);
    if (2L * s->N > lim) throw Error(DSR_E_ARG, "2N = 2 x %d x %d = %ld rows exceed the %ld the workgroup's LDS holds", s->K, s->L, 2L * s->N, lim);
    s->lds = lds_bytes(*s);
    const int O1 = orderN + 1;
    s->bn.resize((size_t) F * O1); s->absbn.resize((size_t) F * O1);
    static const zc IN[4] = {zc(1, 0), zc(0, 1), zc(-1, 0), zc(0, -1)};      // _calc_in (:299-312)
    for (int f = 0; f < F; f++) {
      const double ka = 2.0 * M_PI * f * a * sampleRate / (fftLen * SSPEED);
      for (int n = 0; n < O1; n++) {
        const zc b = gmul(gmul(zc(4.0 * M_PI, 0.0), IN[n % 4]), modal_coefficient(n, ka));
        s->bn[(size_t) f * O1 + n] = b; s->absbn[(size_t) f * O1 + n] = std::hypot(b.real(), b.imag());
      }
    }
    s->sc.resize((size_t) s->modesN * CHAN); s->norm.resize(s->modesN);
    int idx = 0;
    for (int n = 0; n <= orderN; n++)
      for (int m = -n; m <= n; m++, idx++) {
        s->norm[idx] = trk_norm(n, m);
        for (int c = 0; c < CHAN; c++) s->sc[(size_t) idx * CHAN + c] = std::conj(host_harmonic(n, m, EM_THETA[c] * M_PI / 180.0, EM_PHI[c] * M_PI / 180.0));
      }
    *out = s.release();
  });
}

void dsr_trk_destroy(dsr_trk* s) { delete s; }
int dsr_trk_state_doubles(const dsr_trk*) { return STATE_DOUBLES; }
int dsr_trk_modes_n(const dsr_trk* s) { return s ? s->modesN : 0; }
int dsr_trk_subband_length(const dsr_trk* s) { return s ? s->L : 0; }
int dsr_trk_use_subbands_n(const dsr_trk* s) { return s ? s->K : 0; }
int dsr_trk_fft_len(const dsr_trk* s) { return s ? s->M : 0; }
int64_t dsr_trk_max_rows(int kind, int orderN, int useSubbandsN) { return max_rows((orderN + 1) * (orderN + 1), orderN, kind == DSR_TRK_SPATIAL, useSubbandsN); }

dsr_status dsr_trk_set_v(dsr_trk* s, const double* Vk, size_t nDoubles, unsigned subbandX)
{
  return guard([&] {
    if (!s || !Vk) throw Error(DSR_E_ARG, "null argument");
    const int L = s->L, L2 = 2 * L;
    if ((int) subbandX >= s->F) throw Error(DSR_E_ARG, "subband %u outside [0, %d)", subbandX, s->F);
    if (nDoubles != (size_t) 2 * L * L) throw Error(DSR_E_ARG, "Vk: %d x %d complex values expected", L, L);
    std::vector<double> B((size_t) L2 * L2, 0.0);
    if (!s->V.empty()) std::copy(s->V.begin() + (size_t) subbandX * L2 * L2, s->V.begin() + (size_t) (subbandX + 1) * L2 * L2, B.begin());
    else for (int n = 0; n < L2; n++) B[(size_t) n * L2 + n] = std::sqrt(s->s2v);
    for (int m = 0; m < L; m++)                              // :965-974: the lower triangle only; (m + L, n) with n > m keeps its contents
      for (int n = 0; n <= m; n++) {
        const double c = Vk[2 * ((size_t) m * L + n)], sg = Vk[2 * ((size_t) m * L + n) + 1];
        B[(size_t) m * L2 + n] = c; B[(size_t) (m + L) * L2 + n + L] = c; B[(size_t) (m + L) * L2 + n] = sg;
      }
    std::vector<double> C((size_t) L2 * L2, 0.0);            // the Cholesky factor of the lower triangle, row by row; the strict upper part zero
    for (int i = 0; i < L2; i++) {
      for (int j = 0; j < i; j++) {
        double sum = 0.0; for (int k = 0; k < j; k++) sum += C[(size_t) i * L2 + k] * C[(size_t) j * L2 + k];
        C[(size_t) i * L2 + j] = (B[(size_t) i * L2 + j] - sum) / C[(size_t) j * L2 + j];
      }
      double sum = 0.0; for (int k = 0; k < i; k++) sum += C[(size_t) i * L2 + k] * C[(size_t) i * L2 + k];
      const double d = B[(size_t) i * L2 + i] - sum;
      if (!(d > 0.0)) throw Error(DSR_E_ARG, "setV: the block of subband %u is not positive definite", subbandX);
      C[(size_t) i * L2 + i] = std::sqrt(d);
    }
    if (s->V.empty()) {
      s->V.assign((size_t) s->F * L2 * L2, 0.0);
      for (int f = 0; f < s->F; f++) for (int n = 0; n < L2; n++) s->V[((size_t) f * L2 + n) * L2 + n] = std::sqrt(s->s2v);
    }
    std::copy(C.begin(), C.end(), s->V.begin() + (size_t) subbandX * L2 * L2);
    s->vDirty = true;
  });
}

dsr_status dsr_trk_get_v(const dsr_trk* s, unsigned subbandX, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_ARG, "null argument");
    const int L2 = 2 * s->L;
    if ((int) subbandX >= s->F || outDoubles != (size_t) L2 * L2) throw Error(DSR_E_ARG, "subband %u, %d x %d doubles expected", subbandX, L2, L2);
    if (s->V.empty()) { std::fill(out, out + outDoubles, 0.0); for (int n = 0; n < L2; n++) out[(size_t) n * L2 + n] = std::sqrt(s->s2v); }
    else std::copy(s->V.begin() + (size_t) subbandX * L2 * L2, s->V.begin() + (size_t) (subbandX + 1) * L2 * L2, out);
  });
}

dsr_status dsr_trk_set_initial_position(dsr_trk* s, double theta, double phi)
{ return guard([&] { if (!s) throw Error(DSR_E_ARG, "null handle"); s->th0 = theta; s->ph0 = phi; }); }
dsr_status dsr_trk_next_speaker(dsr_trk* s)
{ return guard([&] { if (!s) throw Error(DSR_E_ARG, "null handle"); s->th0 = 0.5; s->ph0 = 0.0; }); }

dsr_status dsr_trk_init_state(dsr_trk* s, double* state_dev, int U, int positionOnly, void* stream)
{
  return guard([&] {
    if (!s || !state_dev || U <= 0) throw Error(DSR_E_ARG, "null argument or U <= 0");
    require_device();
    launch(k_trk_init, dim3(cdiv(U, NT)), dim3(NT), 0, (hipStream_t) stream, state_dev, U, s->th0, s->ph0, std::sqrt(std::sqrt(s->s2init)), positionOnly);
  });
}

dsr_status dsr_trk_bn(const dsr_trk* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out || outDoubles != 2 * s->bn.size()) throw Error(DSR_E_ARG, "bn: [fftLen/2+1][orderN+1] complex128 expected");
    memcpy(out, s->bn.data(), sizeof(double) * outDoubles);
  });
}
dsr_status dsr_trk_sensor_harmonics(const dsr_trk* s, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out || outDoubles != 2 * s->sc.size()) throw Error(DSR_E_ARG, "sensor harmonics: [modesN][32] complex128 expected");
    memcpy(out, s->sc.data(), sizeof(double) * outDoubles);
  });
}
dsr_status dsr_trk_geometry(double* theta_s, double* phi_s, int n)
{
  return guard([&] {
    if (!theta_s || !phi_s || n != CHAN) throw Error(DSR_E_ARG, "the geometry has %d sensors", CHAN);
    for (int c = 0; c < CHAN; c++) { theta_s[c] = EM_THETA[c] * M_PI / 180.0; phi_s[c] = EM_PHI[c] * M_PI / 180.0; }
  });
}

dsr_status dsr_trk_harmonic(int order, int degree, double theta, double phi, double* out2)
{
  return guard([&] {
    if (!out2 || order < 0 || degree > order || -degree > order) throw Error(DSR_E_ARG, "|degree| <= order expected");
    const zc y = host_harmonic(order, degree, theta, phi); out2[0] = y.real(); out2[1] = y.imag();
  });
}
dsr_status dsr_trk_harmonic_deriv_polar(int order, int degree, double theta, double phi, double* out2)
{
  return guard([&] {
    if (!out2 || order < 0 || degree > order || -degree > order) throw Error(DSR_E_ARG, "|degree| <= order expected");
    const Harm h = trk_harm(order, degree, std::cos(theta), std::sin(theta), phi, trk_norm(order, degree)); out2[0] = h.tr; out2[1] = h.ti;
  });
}
dsr_status dsr_trk_harmonic_deriv_azimuth(int order, int degree, double theta, double phi, double* out2)
{
  return guard([&] {
    if (!out2 || order < 0 || degree > order || -degree > order) throw Error(DSR_E_ARG, "|degree| <= order expected");
    const Harm h = trk_harm(order, degree, std::cos(theta), std::sin(theta), phi, trk_norm(order, degree)); out2[0] = h.pr; out2[1] = h.pi;
  });
}
dsr_status dsr_trk_modal_coefficient(unsigned order, double ka, double* out2)
{
  return guard([&] {
    if (!out2) throw Error(DSR_E_ARG, "null argument");
    const zc b = modal_coefficient(order, ka); out2[0] = b.real(); out2[1] = b.imag();
  });
}

dsr_status dsr_trk_run(dsr_trk* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, double* state_dev, float* pos_dev, double* pos64_dev,
                       int32_t* info_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !nframes_dev || !state_dev || !pos_dev || !pos64_dev || !info_dev) throw Error(DSR_E_ARG, "null argument");
    if (U <= 0 || Tmax <= 0) throw Error(DSR_E_ARG, "U and Tmax must be positive");
    require_device();
    hipStream_t st = (hipStream_t) stream;
    upload_tables(*s, st);
    const size_t FL = (size_t) s->F * s->L, wsStride = (8 * FL + 7 * (size_t) s->F + 1) / 2 * 2;   // doubles, even: the complex tables stay 16-byte aligned
    DevBuf<double>& ws = s->ws.at(st); ws.reserve((size_t) U * wsStride);
    TrkP p;
    p.spatial = s->spatial; p.orderN = s->orderN; p.modesN = s->modesN; p.F = s->F; p.L = s->L; p.K = s->K; p.N = s->N; p.maxLocalN = s->maxLocalN;
    p.Tmax = Tmax; p.hasV = s->V.empty() ? 0 : 1; p.su = std::sqrt(s->s2u); p.sv = std::sqrt(s->s2v);
    p.bn = s->dBn.p; p.sc = s->dSc.p; p.norm = s->dNorm.p; p.absbn = s->dAbs.p; p.Vt = s->dVt.p;
    launch(k_trk_run, dim3(U), dim3(NT), s->lds, st, p, (const float2*) X_dev, nframes_dev, state_dev, ws.p, wsStride, pos_dev, pos64_dev, info_dev);
  });
}

dsr_status dsr_pws_coefficients(const dsr_trk* s, double theta, double phi, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out || outDoubles != (size_t) 2 * CHAN * s->F) throw Error(DSR_E_ARG, "coefficients: [32][fftLen/2+1] complex128 expected");
    const int O1 = s->orderN + 1;
    std::vector<zc> Y(s->modesN);
    int idx = 0;
    for (int n = 0; n <= s->orderN; n++) for (int m = -n; m <= n; m++) Y[idx++] = host_harmonic(n, m, theta, phi);
    for (int c = 0; c < CHAN; c++)
      for (int f = 0; f < s->F; f++) {                       // :1453-1465
        zc coefficient(0, 0);
        for (int n = 0; n < O1; n++) {
          zc coeff_n(0, 0);
          for (int i = n * n; i < (n + 1) * (n + 1); i++) coeff_n += gmul(s->sc[(size_t) i * CHAN + c], Y[i]);
          coefficient += gmul(s->bn[(size_t) f * O1 + n], coeff_n);
        }
        out[2 * ((size_t) c * s->F + f)] = coefficient.real(); out[2 * ((size_t) c * s->F + f) + 1] = coefficient.imag();
      }
  });
}

dsr_status dsr_pws_apply(const double* coef_dev, int chanN, const float* src_dev, const int32_t* nframes_dev, int U, int Tmax, int fftLen, int full, float* out_dev,
                         void* stream)
{
  return guard([&] {
    if (!coef_dev || !src_dev || !nframes_dev || !out_dev) throw Error(DSR_E_ARG, "null argument");
    if (chanN <= 0 || U <= 0 || Tmax <= 0 || fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_ARG, "chanN, U, Tmax positive and fftLen even expected");
    require_device();
    const size_t total = (size_t) U * chanN * Tmax * (fftLen / 2 + 1);
    const int blocks = (int) std::min<size_t>((total + NT - 1) / NT, 65535);
    launch(k_pws_apply, dim3(blocks), dim3(NT), 0, (hipStream_t) stream, (const double2*) coef_dev, chanN, (const float2*) src_dev, nframes_dev, U, Tmax,
                       fftLen, full, (float2*) out_dev);
  });
}

}  // extern "C"
