// csrc/k_conv.hip -- block convolution with an impulse response and the FIR across frames, include/dsr.h section 2g.
//
// Restates OverlapAdd and OverlapSave of btk/convolution (convolution.h:40-104, convolution.cc:43-290) and the arithmetic of FilterFeature
// (feature.cc:3206-3313).  fp64 up to the fp32 buffer add, built without FMA contraction.
//
// Kernels:
//   k_conv_fft    a workgroup per (utterance, block), grid-stride: the block's forward real transform of N points as a complex one of N/2
//                 (fft_lds.h), kept as the spectrum of the complex transform; then for each of the C responses the product with H_c in the
//                 half spectrum, the split step, the inverse transform and the scaling by 1/N.  OverlapAdd stores the first L+P-1 samples of
//                 the section in fp64 for the fold; OverlapSave stores samples P..L-1 as fp32 output.
//                 MODE 0 (N <= 4096): data, twiddles and the saved spectrum in LDS (90 KB at N = 4096).  MODE 1 (N = 8192): data and twiddles
//                 in LDS (112 KB), the saved spectrum in the workgroup's block of global memory.  MODE 2 (N > 8192): everything in the
//                 workgroup's block of global memory, as k_cctde<true>.
//   k_conv_fold   OverlapAdd's fp32 buffer recurrence, a thread per output sample: the carried value, then the sections that reach the
//                 sample, oldest block first, rounded to fp32 after every add.  One more row per (utterance, channel) is the buffer the next
//                 call starts from.
//   k_fir_frames  FilterFeature: a thread per (utterance, frame, coefficient), fp64 accumulator over the taps in ascending order.
#include "launch.h"
#include "dev_math.h"
#include "fft_lds.h"
#include <cmath>
#include <complex>

using namespace dsr;

struct dsr_conv {
  int kind, L, P, N, C, size;
  std::vector<double> H;                            // [C][N/2+1] complex: the responses' half spectra
  DevBuf<double2> dH; bool haveH = false, uploaded = false;
  EventTimes<3> tm;                                 // dsr_conv_set_timing: around k_conv_fft and k_conv_fold
};

namespace {

constexpr int CONV_FFT_MAX = 1 << 22;               // as CCTDE's limit: 4 Mi samples, 7 N/2 doubles of work space a workgroup
constexpr int CONV_LDS_ALL = 4096, CONV_LDS_MAX = 8192;
constexpr int CONV_GRID_LDS = 16384, CONV_GRID_SPEC = 1024, CONV_GRID_GLOBAL = 8;

struct CPar { int kind, U, C, T, L, P, N, S; };     // S = L+P-1, the samples of a section that the fold reads


// bin k (0 <= k <= n) of the real transform of 2n points from Z = FFT_n(x[2m] + i x[2m+1]): X[k] = E + e^{-2 pi i k / 2n} O with
// E = (Z[k] + conj Z[n-k]) / 2, O = -i (Z[k] - conj Z[n-k]) / 2; (cs, sn) = cos, sin of pi k / n
__device__ __forceinline__ double2 half_bin(const double* sr, const double* si, int k, int n, double cs, double sn)
{
  const int a = k & (n - 1), b = (n - k) & (n - 1);
  const double zr = sr[a], zi = si[a], cr = sr[b], ci = -si[b];
  const double er = 0.5 * (zr + cr), ei = 0.5 * (zi + ci), orr = 0.5 * (zi - ci), oi = -0.5 * (zr - cr);
  return make_double2(er + (orr * cs + oi * sn), ei + (oi * cs - orr * sn));
}
// the reference multiplies bins 0 and N/2 by the real part of the response alone (convolution.cc:135-143)
__device__ __forceinline__ double2 times_h(double2 x, double2 h, bool edge)
{
  if (edge) return make_double2(x.x * h.x, 0.0);
  return make_double2(x.x * h.x - x.y * h.y, x.x * h.y + x.y * h.x);                                       // gsl_complex_mul
}

template <int MODE>
__global__ __launch_bounds__(512) void k_conv_fft(const float* __restrict__ x, const int* __restrict__ nf, const double2* __restrict__ H, CPar p,
                                                  double* __restrict__ sec, float* __restrict__ y, double* work, long nItems)
{
  extern __shared__ double lds[];
  const int N = p.N, n = N / 2, logn = 31 - __clz(n), B = blockDim.x, tid = threadIdx.x, tw = fft_tw_entries(n);
  double *re, *im, *sr, *si, *twr, *twi;
  if (MODE == 2) { re = work + (size_t) blockIdx.x * ((size_t) 4 * n + 2 * (size_t) tw); im = re + n; sr = im + n; si = sr + n; twr = si + n; twi = twr + tw; }
  else {
    re = lds; im = re + n; twr = im + n; twi = twr + tw;
    if (MODE == 0) { sr = twi + tw; si = sr + n; } else { sr = work + (size_t) blockIdx.x * 2 * n; si = sr + n; }
  }
  fft_tw_init(twr, twi, n);
  const double inv = 1.0 / (double) N;
  const int outN = p.L - p.P;                                                                              // OverlapSave's size
  for (long it = blockIdx.x; it < nItems; it += gridDim.x) {
    const int u = (int) (it / p.T), t = (int) (it % p.T);
    if (t >= clampT(nf, u, p.T)) {                                                                         // uniform over the workgroup
      if (p.kind == 1)
        for (int c = 0; c < p.C; c++)
          for (int i = tid; i < outN; i += B) y[(((size_t) u * p.C + c) * p.T + t) * outN + i] = 0.0f;
      continue;                                                                                            // OverlapAdd: the fold writes the zeros
    }
    const float* xb = x + (size_t) it * p.L;
    __syncthreads();
    for (int k = tid; k < n; k += B) {
      const int i0 = 2 * k, r = brev(k, logn);
      re[r] = i0 < p.L ? (double) xb[i0] : 0.0; im[r] = i0 + 1 < p.L ? (double) xb[i0 + 1] : 0.0;
    }
    fft_run(re, im, twr, twi, n, -1.0);
    for (int k = tid; k < n; k += B) { sr[k] = re[k]; si[k] = im[k]; }
    for (int c = 0; c < p.C; c++) {
      const double2* Hc = H + (size_t) c * (n + 1);
      __syncthreads();
      for (int k = tid; k < n; k += B) {
        double sn, cs; sincospi((double) k / n, &sn, &cs);
        const double2 A = times_h(half_bin(sr, si, k, n, cs, sn), Hc[k], k == 0);
        double2 Bc = times_h(half_bin(sr, si, n - k, n, -cs, sn), Hc[n - k], k == 0);                      // pi (n-k) / n = pi - pi k / n
        Bc.y = -Bc.y;
        // split step of the inverse: Z[k] = (Y[k] + conj Y[n-k]) + i (Y[k] - conj Y[n-k]) e^{2 pi i k / N}
        const double ex = A.x + Bc.x, ey = A.y + Bc.y, dx = A.x - Bc.x, dy = A.y - Bc.y;
        const double ox = dx * cs - dy * sn, oy = dx * sn + dy * cs;
        const int r = brev(k, logn);
        re[r] = ex - oy; im[r] = ey + ox;
      }
      fft_run(re, im, twr, twi, n, 1.0);
      const size_t row = ((size_t) u * p.C + c) * p.T + t;
      if (p.kind == 0) {
        double* s = sec + row * p.S;
        for (int i = tid; i < p.S; i += B) s[i] = ((i & 1) ? im[i >> 1] : re[i >> 1]) * inv;               // gsl_fft_halfcomplex_radix2_inverse scales by 1/N
      } else {
        float* o = y + row * outN;
        for (int i = p.P + tid; i < p.L; i += B) o[i - p.P] = (float) (((i & 1) ? im[i >> 1] : re[i >> 1]) * inv);   // from P, not P-1 (convolution.cc:270)
      }
    }
  }
}

// OverlapAdd::next's buffer (convolution.cc:148-160) for sample i of block t of (utterance, channel) uc = blockIdx.x / (T+1); row T is the
// buffer after the utterance's last block: what the next call starts from.  g counts samples from the first block of this call.
__global__ __launch_bounds__(256) void k_conv_fold(const double* __restrict__ sec, const int* __restrict__ nf, CPar p, const float* __restrict__ state,
                                                   float* __restrict__ newState, float* __restrict__ y)
{
  const int i = blockIdx.y * 256 + threadIdx.x, t = (int) (blockIdx.x % (p.T + 1));
  const size_t uc = blockIdx.x / (p.T + 1);
  const int T = clampT(nf, (int) (uc / p.C), p.T), keep = p.P - 1;
  const bool stateRow = t == p.T;
  if (i >= (stateRow ? keep : p.L)) return;
  float* dst = stateRow ? newState + uc * keep + i : y + (uc * p.T + t) * p.L + i;
  if (!stateRow && t >= T) { *dst = 0.0f; return; }
  const int tt = stateRow ? T : t, last = stateRow ? T - 1 : t;
  const long g = (long) tt * p.L + i, lo = g - (p.S - 1);
  float acc = g < keep ? state[uc * keep + g] : 0.0f;
  for (int b = lo <= 0 ? 0 : (int) ((lo + p.L - 1) / p.L); b <= last; b++)
    acc = (float) ((double) acc + sec[(uc * p.T + b) * p.S + (size_t) (g - (long) b * p.L)]);
  *dst = acc;
}

__global__ void k_conv_zero(float* p, size_t n) { const size_t i = (size_t) blockIdx.x * 256 + threadIdx.x; if (i < n) p[i] = 0.0f; }

// FilterFeature::next (feature.cc:3286-3300): y[t][c] = float(sum_i a[i+o] * double(x[t-i][c])), i ascending; frames outside [0, T) are zeros
__host__ __device__ inline int fir_count(int T, int o) { return o == 0 ? T + 1 : (T < o ? 0 : T); }
__global__ __launch_bounds__(256) void k_fir_frames(const float* __restrict__ x, const int* __restrict__ nf, const double* __restrict__ a, int lenA, int U, int Tmax,
                                                    int Tout, int dim, float* __restrict__ y)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tout * dim) return;
  const int c = (int) (idx % dim), t = (int) ((idx / dim) % Tout), u = (int) (idx / ((size_t) dim * Tout));
  const int T = clampT(nf, u, Tmax), o = (lenA - 1) / 2;
  if (t >= fir_count(T, o)) { y[idx] = 0.0f; return; }
  double sum = 0.0;
  for (int i = -o; i <= o; i++) {
    const int s = t - i;
    const double v = (s >= 0 && s < T) ? (double) x[((size_t) u * Tmax + s) * dim + c] : 0.0;
    sum += a[i + o] * v;
  }
  y[idx] = (float) sum;
}

struct CScratch { DevBuf<double> sec, work, a; DevBuf<float> newState; };
PerStream<CScratch> c_scratch;

// the half spectrum of a zero-padded real sequence on the host: an iterative radix-2 transform of N complex points
void host_rfft(const double* h, int P, int N, double* out /* [N/2+1][2] */)
{
  std::vector<std::complex<double>> z(N);
  const int logn = ilog2((unsigned) N);
  for (int i = 0; i < N; i++) {
    unsigned r = 0; for (int b = 0; b < logn; b++) if (i & (1 << b)) r |= 1u << (logn - 1 - b);
    z[r] = i < P ? std::complex<double>(h[i], 0.0) : std::complex<double>(0.0, 0.0);
  }
  for (int len = 2; len <= N; len *= 2) {
    const int half = len / 2;
    std::vector<std::complex<double>> w(half);
    for (int k = 0; k < half; k++) { const double a = -2.0 * M_PI * (double) k / (double) len; w[k] = std::complex<double>(std::cos(a), std::sin(a)); }
    for (int s = 0; s < N; s += len)
      for (int k = 0; k < half; k++) {
        const std::complex<double> e = z[s + k], o = z[s + k + half] * w[k];
        z[s + k] = e + o; z[s + k + half] = e - o;
      }
  }
  for (int k = 0; k <= N / 2; k++) { out[2 * k] = z[k].real(); out[2 * k + 1] = (k == 0 || k == N / 2) ? 0.0 : z[k].imag(); }      // _halfComplexUnpack
}

int conv_mode(int N) { return N <= CONV_LDS_ALL ? 0 : (N <= CONV_LDS_MAX ? 1 : 2); }
int conv_block(int n) { const int b = n / 2; return b < 64 ? 64 : (b > 512 ? 512 : b); }

}  // namespace

extern "C" {

dsr_status dsr_conv_create(int kind, int L, int P, int fftLen, int C, dsr_conv** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind != 0 && kind != 1) throw Error(DSR_E_PARAMETER, "unknown convolution kind %d (0 OverlapAdd, 1 OverlapSave)", kind);
    if (L < 1 || P < 1 || C < 1) throw Error(DSR_E_DIMENSION, "section length %d, impulse response length %d, %d responses: at least one of each is needed", L, P, C);
    const long need = (long) L + P - 1; long N;
    if (kind == 0) {
      if (fftLen == 0) { N = 4; while (N < need && N <= CONV_FFT_MAX) N *= 2; }                             // _checkFFTLen (convolution.cc:80-102); 4 is the shortest transform here
      else {
        if (fftLen < 0 || fftLen < need)
          throw Error(DSR_E_DIMENSION, "Section (%d) and impulse response (%d) lengths inconsistent with FFT length (%d).", L, P, fftLen);
        N = fftLen;
      }
    } else {
      if (P >= L) throw Error(DSR_E_DIMENSION, "Cannot have P = %d and L = %d", P, L);                     // _checkOutputSize (convolution.cc:211-217)
      N = L;
    }
    if (N > CONV_FFT_MAX) throw Error(DSR_E_DIMENSION, "FFT length %ld is above the limit of %d", N, CONV_FFT_MAX);
    if (N < 4 || !is_pow2((unsigned) N)) throw Error(DSR_E_DIMENSION, "FFT length %ld: a power of two of at least 4 is needed", N);
    dsr_conv* q = new dsr_conv(); std::unique_ptr<dsr_conv> hold(q);
    q->kind = kind; q->L = L; q->P = P; q->N = (int) N; q->C = C; q->size = kind == 0 ? L : L - P;
    q->H.assign((size_t) C * (N / 2 + 1) * 2, 0.0);
    *out = hold.release();
  });
}
void dsr_conv_destroy(dsr_conv* q) { delete q; }
int dsr_conv_size(const dsr_conv* q) { return q ? q->size : 0; }
int dsr_conv_fft_len(const dsr_conv* q) { return q ? q->N : 0; }

dsr_status dsr_conv_set_response(dsr_conv* q, const double* h_host)
{
  return guard([&] {
    if (!q) throw Error(DSR_E_PARAMETER, "null argument");
    if (!h_host) throw Error(DSR_E_PARAMETER, "null impulse response");                                    // the reference dereferences it
    const size_t bins = (size_t) q->N / 2 + 1;
    for (int c = 0; c < q->C; c++) host_rfft(h_host + (size_t) c * q->P, q->P, q->N, q->H.data() + (size_t) c * bins * 2);
    q->haveH = true; q->uploaded = false;
  });
}

dsr_status dsr_conv_update(dsr_conv* q, int c, const double* delta_host)
{
  return guard([&] {
    if (!q || !delta_host) throw Error(DSR_E_PARAMETER, "null argument");
    if (q->kind != 1) throw Error(DSR_E_PARAMETER, "update() belongs to OverlapSave");
    if (c < 0 || c >= q->C) throw Error(DSR_E_INDEX, "response %d of %d", c, q->C);
    if (!q->haveH) throw Error(DSR_E_CONSISTENCY, "set the impulse response before update()");
    const size_t bins = (size_t) q->N / 2 + 1; double* H = q->H.data() + (size_t) c * bins * 2;
    for (size_t k = 0; k < bins; k++) { H[2 * k] += delta_host[2 * k]; H[2 * k + 1] += delta_host[2 * k + 1]; }      // the stored bins only
    q->uploaded = false;
  });
}

size_t dsr_conv_state_bytes(const dsr_conv* q, int U) { return (q && U > 0 && q->kind == 0) ? (size_t) U * q->C * (q->P - 1) * sizeof(float) : 0; }

dsr_status dsr_conv_state_init(const dsr_conv* q, void* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!q || U < 1) throw Error(DSR_E_PARAMETER, "null argument");
    const size_t n = dsr_conv_state_bytes(q, U) / sizeof(float);
    if (n == 0) return;
    if (!state_dev) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    launch(k_conv_zero, dim3(cdiv((long) n, 256)), dim3(256), 0, (hipStream_t) stream, (float*) state_dev, n);
  });
}

dsr_status dsr_conv_apply(dsr_conv* q, const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, void* state_dev, float* y_dev, void* stream)
{
  return guard([&] {
    if (!q || !x_dev || !y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 1 || Tmax < 0) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d Tmax=%d", U, Tmax);
    if (!q->haveH) throw Error(DSR_E_CONSISTENCY, "set the impulse response before apply()");
    const int keep = q->P - 1;
    if (q->kind == 0 && keep > 0 && !state_dev) throw Error(DSR_E_PARAMETER, "null state");
    if ((long) U * q->C * ((long) Tmax + 1) > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "U * C * (Tmax + 1) = %ld is above 2^31", (long) U * q->C * ((long) Tmax + 1));
    require_device();
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    if (!q->uploaded) { q->dH.upload((const double2*) q->H.data(), q->H.size() / 2, st); q->uploaded = true; }
    CScratch& sc = c_scratch.at(st);
    const int N = q->N, n = N / 2, mode = conv_mode(N), B = conv_block(n), tw = fft_tw_entries(n);
    const long items = (long) U * Tmax;
    const CPar p{q->kind, U, q->C, Tmax, q->L, q->P, N, q->L + q->P - 1};
    if (q->kind == 0) sc.sec.reserve((size_t) items * q->C * p.S);
    const int cap = mode == 0 ? CONV_GRID_LDS : (mode == 1 ? CONV_GRID_SPEC : CONV_GRID_GLOBAL);
    const int grid = (int) (items < cap ? items : cap);
    q->tm.mark(0, st);
    if (mode == 0) {
      const size_t ldsBytes = ((size_t) 4 * n + 2 * tw) * 8;
      launch(k_conv_fft<0>, dim3(grid), dim3(B), ldsBytes, st, x_dev, nframes_dev, q->dH.p, p, sc.sec.p, y_dev, (double*) nullptr, items);
    } else if (mode == 1) {
      const size_t ldsBytes = ((size_t) 2 * n + 2 * tw) * 8;
      sc.work.reserve((size_t) grid * 2 * n);
      launch(k_conv_fft<1>, dim3(grid), dim3(B), ldsBytes, st, x_dev, nframes_dev, q->dH.p, p, sc.sec.p, y_dev, sc.work.p, items);
    } else {
      sc.work.reserve((size_t) grid * ((size_t) 4 * n + 2 * (size_t) tw));
      launch(k_conv_fft<2>, dim3(grid), dim3(B), 0, st, x_dev, nframes_dev, q->dH.p, p, sc.sec.p, y_dev, sc.work.p, items);
    }
    q->tm.mark(1, st);
    if (q->kind == 0) {
      const size_t stateN = (size_t) U * q->C * keep;
      sc.newState.reserve(stateN ? stateN : 1);
      const int width = q->L > keep ? q->L : keep;
      launch(k_conv_fold, dim3((unsigned) (U * q->C * (Tmax + 1)), cdiv(width, 256)), dim3(256), 0, st, sc.sec.p, nframes_dev, p, (const float*) state_dev,
                         sc.newState.p, y_dev);
      if (stateN) DSR_HIP(hipMemcpyAsync(state_dev, sc.newState.p, stateN * sizeof(float), hipMemcpyDeviceToDevice, st));
    }
    q->tm.mark(2, st);
  });
}

dsr_status dsr_conv_set_timing(dsr_conv* q, int on)
{
  return guard([&] {
    if (!q) throw Error(DSR_E_PARAMETER, "null argument");
    q->tm.enable(on != 0);
  });
}
dsr_status dsr_conv_kernel_ms(const dsr_conv* q, double* ms2)
{
  return guard([&] {
    if (!q || !ms2 || !q->tm.on) throw Error(DSR_E_PARAMETER, "timing is off");
    q->tm.wait(2); ms2[0] = q->tm.ms(0, 1); ms2[1] = q->tm.ms(1, 2);
  });
}

int dsr_fir_frames_count(int T, int lenA) { return (T < 0 || lenA < 1) ? 0 : fir_count(T, (lenA - 1) / 2); }

dsr_status dsr_fir_frames_run(const float* x_dev, const int32_t* nframes_dev, const double* a_host, int lenA, int U, int Tmax, int dim, float* y_dev, void* stream)
{
  return guard([&] {
    if (!x_dev || !a_host || !y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (lenA < 1 || lenA % 2 != 1) throw Error(DSR_E_DIMENSION, "Length of filter (%d) is not odd.", lenA);                      // feature.cc:3219-3220
    if (U < 1 || Tmax < 0 || dim < 1) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d Tmax=%d dim=%d", U, Tmax, dim);
    require_device();
    const int Tout = Tmax + (lenA == 1 ? 1 : 0);
    if (Tout == 0) return;
    hipStream_t st = (hipStream_t) stream;
    CScratch& sc = c_scratch.at(st);
    sc.a.upload(a_host, (size_t) lenA, st);
    const size_t total = (size_t) U * Tout * dim;
    launch(k_fir_frames, dim3(cdiv((long) total, 256)), dim3(256), 0, st, x_dev, nframes_dev, sc.a.p, lenA, U, Tmax, Tout, dim, y_dev);
  });
}

}  // extern "C"
