// csrc/k_featops.hip -- the scalar feature operators of btk/feature/feature.{h,cc} (include/dsr.h section 6c): SignalPower,
// ZeroCrossingRateHamming, YINPitch, SpikeFilter, SpikeFilter2, ALog, Normalize, Threshold, Amplification, SpectralResampling, SphinxMel.
//
// Every operator keeps the reference's operation order and the float / double of every intermediate, so the file is built without FMA
// contraction and the tests compare bits.  All entry points take device arrays [U][Tmax][dim] and an optional nframes_dev [U]; frames at or
// past an utterance's count come out zero.
//
//   k_yin<LDS>      one wavefront per frame, one lane per lag, 64 lags a chunk; the wave leaves after the chunk in which the reference's
//                   predicate first holds (its early return).  d(tau) = sum_j (x[j] - x[j+tau])^2 in fp32, j ascending: x[j] is wave-uniform
//                   and comes through scalar loads, x[j+tau .. j+tau+3] is one 16-byte LDS read from the one of four copies of the frame
//                   (shifted by 0..3 samples) in which that address is aligned, so four (tau, j) pairs cost one LDS instruction beside their
//                   twelve vector ones.  The running sum over lags is a chain of 64 dependent adds a chunk.  LDS = false reads the frame from
//                   global memory (frames too long for the four copies).
//   k_spike2        SpikeFilter2's serial state machine: one workgroup of 64 per utterance, the block staged in LDS, lane 0 walks it, frames
//                   in order, (meanslope, count) carried in and out.
//   k_minmax        the running / whole-utterance minimum and maximum of ALog and Normalize: contiguous segments a lane, combined in index
//                   order with the reference's strict comparisons (the first of two equal values stays, which decides the sign of a zero).
//   the others      one thread per frame (serial fp64 / fp32 sums of SignalPower and the zero-crossing rate) or per output element.
#include "launch.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

using namespace dsr;

namespace {

// (clampT of dev_math.h in the spelling these kernels were compiled with: the other one changes their instruction schedule)
__device__ __forceinline__ int clampT(const int* nf, int u, int Tmax) { if (!nf) return Tmax; const int t = nf[u]; return t < 0 ? 0 : (t > Tmax ? Tmax : t); }

// ---- SignalPowerFeature::next (feature.cc:1360-1378): fp64 sum of squares, i ascending, / N / range, one rounding to fp32
__global__ __launch_bounds__(256) void k_signal_power(const float* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int N, double range, float* __restrict__ y)
{
  const size_t f = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t) U * Tmax) return;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[f] = 0.0f; return; }
  const float* r = x + f * N;
  double p = 0.0;
  for (int i = 0; i < N; i++) { const double v = r[i]; p += v * v; }
  y[f] = (float) (p / (double) (unsigned) N / range);
}

// ---- ZeroCrossingRateHammingFeature::next (feature.cc:3557-3577): a float sum widened, added to and rounded back at every step
__global__ __launch_bounds__(256) void k_zcr(const float* __restrict__ x, const int* __restrict__ nf, const double* __restrict__ w, int U, int Tmax, int N, float* __restrict__ y)
{
  const size_t f = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t) U * Tmax) return;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[f] = 0.0f; return; }
  const float* r = x + f * N;
  float sum = 0.0f;
  int s = r[0] >= 0 ? 1 : -1;
  for (int i = 0; i + 1 < N; i++) {
    const int sn = r[i + 1] >= 0 ? 1 : -1;
    sum = (float) ((double) sum + (double) (abs(sn - s) / 2) * w[i]);
    s = sn;
  }
  y[f] = sum / (float) (unsigned) N;
}

// ---- YINPitchFeature (feature.cc:3584-3634)
__device__ __forceinline__ float lane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

template <bool LDS>
__global__ void k_yin(const float* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int N, int NQ, unsigned sr, float tol,
                      float* __restrict__ pitch, float* __restrict__ value, int* __restrict__ chunks)
{
  extern __shared__ float4 yin_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wpb = blockDim.x >> 6;
  const long F = (long) U * Tmax;
  const long f = (long) blockIdx.x * wpb + wave;                       // wave-uniform: the frame's loads below are scalar loads
  const bool inside = f < F;
  const int u = inside ? (int) (f / Tmax) : 0, t = inside ? (int) (f % Tmax) : 0;
  const bool live = inside && t < clampT(nf, u, Tmax);
  const float* xs = x + (size_t) (inside ? f : 0) * N;
  float4* cp = yin_lds + (size_t) wave * 4 * NQ;                       // copy s, entry q: x[4q+s .. 4q+s+3], zeros past the frame
  if (LDS) {
    if (live)
      for (int q = lane; q < NQ; q += 64)
        for (int s = 0; s < 4; s++) {
          const int i = 4 * q + s;
          cp[s * NQ + q] = make_float4(i < N ? xs[i] : 0.0f, i + 1 < N ? xs[i + 1] : 0.0f, i + 2 < N ? xs[i + 2] : 0.0f, i + 3 < N ? xs[i + 3] : 0.0f);
        }
    __syncthreads();
  }
  if (!inside) return;
  const int W = N / 2;
  float outPitch = 0.0f, outVal = 1.0f;                                // yin[0] = 1
  int nchunk = 0;
  if (live) {
    float carryRun = 0.0f, carryY = 1.0f;
    for (int base = 0; base < W; base += 64) {                         // lags 64c .. 64c+63; lag 0 is y(0) = 1 and adds nothing
      nchunk++;
      const int tau = base + lane, tc = tau < W ? tau : W - 1;         // lanes past the last lag repeat it and are ignored
      float d = 0.0f;
      int j = 0;
      if (LDS) {
        const float4* c = cp + (tc & 3) * NQ + (tc >> 2);
#pragma unroll 4
        for (; j + 4 <= W; j += 4) {
          const float4 v = c[j >> 2];
          const float t0 = xs[j] - v.x;     d = d + t0 * t0;
          const float t1 = xs[j + 1] - v.y; d = d + t1 * t1;
          const float t2 = xs[j + 2] - v.z; d = d + t2 * t2;
          const float t3 = xs[j + 3] - v.w; d = d + t3 * t3;
        }
        const float* flat = reinterpret_cast<const float*>(cp);        // copy 0 is the frame itself
        for (; j < W; j++) { const float t0 = xs[j] - flat[j + tc]; d = d + t0 * t0; }
      } else {
        const float* xt = xs + tc;
#pragma unroll 4
        for (; j < W; j++) { const float t0 = xs[j] - xt[j]; d = d + t0 * t0; }
      }
      // tmp2 += d(tau), tau ascending: lane L adds the chunk's d(0..L) to the carried sum one after the other
      if (tau == 0) d = 0.0f;
      float run = carryRun;
#pragma unroll
      for (int l = 0; l < 64; l++) { const float dl = lane_f(d, l); if (lane >= l) run = run + dl; }
      const float y = tau == 0 ? 1.0f : d * (float) (unsigned) tau / run;
      float yprev = __shfl_up(y, 1, 64);
      if (lane == 0) yprev = carryY;
      const bool pred = tau >= 1 && tau < W && y < tol && yprev < y;
      const unsigned long long m = __ballot(pred);
      if (m) {
        const int first = __ffsll((long long) m) - 1, lag = base + first - 1;
        outVal = __shfl(y, first, 64);
        outPitch = lag > 0 ? (float) ((double) sr / (double) lag) : 0.0f;
        break;
      }
      carryRun = __shfl(run, 63, 64); carryY = __shfl(y, 63, 64);
      if (base + 64 >= W) outVal = __shfl(y, W - 1 - base, 64);
    }
  } else {
    outVal = 0.0f;
  }
  if (lane == 0) {
    pitch[f] = outPitch;
    if (value) value[f] = outVal;
    if (chunks) chunks[f] = nchunk;
  }
}

// ---- SpikeFilter::next (feature.cc:3656-3696): out[i] = in[i] for i < q, the median of in[i-q..i+q] for q <= i < n-2q, zeros from n-2q on
__global__ __launch_bounds__(256) void k_spike(const float* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int n, int tapN, float* __restrict__ y)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tmax * n) return;
  const int i = (int) (idx % n), t = (int) ((idx / n) % Tmax), u = (int) (idx / ((size_t) n * Tmax));
  const int q = (tapN - 1) >> 1;
  if (t >= clampT(nf, u, Tmax) || i >= n - 2 * q) { y[idx] = 0.0f; return; }
  const float* r = x + (idx - i);
  if (i < q) { y[idx] = r[i]; return; }
  // the element a stable ascending sort of the window puts at position q
  const float* w = r + i - q;
  float med = w[q];
  for (int a = 0; a < tapN; a++) {
    const float va = w[a];
    int rank = 0;
    for (int b = 0; b < tapN; b++) { const float vb = w[b]; rank += (vb < va || (vb == va && b < a)) ? 1 : 0; }
    if (rank == q) med = va;
  }
  y[idx] = med;
}

// ---- SpikeFilter2::next (feature.cc:3711-3776)
__global__ __launch_bounds__(64) void k_spike2(const float* __restrict__ x, const int* __restrict__ nf, int Tmax, int n, unsigned width, float maxslope, float thresh,
                                               float alpha, float beta, float* __restrict__ meanslope, int* __restrict__ count, float* __restrict__ y)
{
  extern __shared__ float sp_v[];
  const int u = blockIdx.x, lane = threadIdx.x;
  const int T = clampT(nf, u, Tmax);
  float ms = meanslope[u]; int cnt = count[u];
  for (int t = 0; t < Tmax; t++) {
    const size_t off = ((size_t) u * Tmax + t) * n;
    if (t >= T) { for (int i = lane; i < n; i += 64) y[off + i] = 0.0f; continue; }
    for (int i = lane; i < n; i += 64) sp_v[i] = x[off + i];
    __syncthreads();
    if (lane == 0) {
      float* v = sp_v;
      unsigned P = 0, Q = 1;
      while (Q < (unsigned) n) {
        float slope = v[Q] - v[P];
        int signB, signE = 0;
        if (slope < 0.0f) { slope = -slope; signB = -1; } else signB = 1;
        P = Q++;
        const float mx = thresh * ms;
        if (slope > mx && slope > maxslope) {
          const unsigned spikeB = P - 1; unsigned spikeN = 0;
          while (Q < (unsigned) n && spikeN < width) {
            slope = v[Q] - v[P];
            if (slope < 0.0f) { slope = -slope; signE = -1; } else signE = 1;
            P = Q++; spikeN++;
            if (signB != signE && slope > mx && slope > maxslope) break;
          }
          const int spikeE = (int) P;
          for (int sX = (int) spikeB + 1; sX < spikeE; sX++) {
            const float lambda = (float) ((unsigned) sX - spikeB) / (float) ((unsigned) spikeE - spikeB);
            const float far = lambda * v[spikeE];                      // float * float, as the reference's expression types it
            v[sX] = (float) ((1.0 - (double) lambda) * (double) v[spikeB] + (double) far);
          }
          cnt++;
        } else {
          ms = beta * ms + alpha * slope;
        }
      }
    }
    __syncthreads();
    for (int i = lane; i < n; i += 64) y[off + i] = sp_v[i];
    __syncthreads();
  }
  if (lane == 0) { meanslope[u] = ms; count[u] = cnt; }
}

// ---- _findMinMax of ALogFeature / NormalizeFeature (feature.cc:1417-1443, 1488-1514)
// runon: frame by frame from the carried state, mm[u][t] = (min, max) after frame t.  Otherwise the whole utterance from (HUGE, -HUGE).
// The final pair goes to state[u].
__global__ __launch_bounds__(64) void k_minmax(const float* __restrict__ x, const int* __restrict__ nf, int Tmax, int dim, int runon, double* __restrict__ state,
                                               double* __restrict__ mm)
{
  __shared__ double smn[64], smx[64];
  const int u = blockIdx.x, lane = threadIdx.x;
  const int T = clampT(nf, u, Tmax);
  const int frames = runon ? T : 1;
  const size_t len = runon ? (size_t) dim : (size_t) T * dim;
  const size_t seg = (len + 63) / 64;
  double mn = runon ? state[2 * u] : (double) FLT_MAX, mx = runon ? state[2 * u + 1] : -(double) FLT_MAX;     // every lane holds the carried pair
  for (int t = 0; t < frames; t++) {
    const float* r = x + ((size_t) u * Tmax + t) * dim;
    const size_t lo = (size_t) lane * seg, hi = lo + seg < len ? lo + seg : len;
    double a = (double) INFINITY, b = -(double) INFINITY;               // strict comparisons: the first of equal values stays, a NaN never enters
    for (size_t i = lo; i < hi; i++) { const double v = r[i]; if (v < a) a = v; if (v > b) b = v; }
    smn[lane] = a; smx[lane] = b;
    __syncthreads();
    for (int l = 0; l < 64; l++) { if (smn[l] < mn) mn = smn[l]; if (smx[l] > mx) mx = smx[l]; }
    __syncthreads();
    if (runon && lane == 0) { mm[2 * ((size_t) u * Tmax + t)] = mn; mm[2 * ((size_t) u * Tmax + t) + 1] = mx; }
  }
  if (lane == 0) { state[2 * u] = mn; state[2 * u + 1] = mx; }
}

__global__ void k_minmax_init(double* state, int U) { const int u = blockIdx.x * 64 + threadIdx.x; if (u < U) { state[2 * u] = (double) FLT_MAX; state[2 * u + 1] = -(double) FLT_MAX; } }

// ALogFeature::next (feature.cc:1383-1406): element 0 of every frame
__global__ __launch_bounds__(256) void k_alog(const float* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int dim, double m, double pw, int runon,
                                              const double* __restrict__ state, const double* __restrict__ mm, float* __restrict__ y)
{
  const size_t f = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (f >= (size_t) U * Tmax) return;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[f] = 0.0f; return; }
  const double mx = runon ? mm[2 * f + 1] : state[2 * u + 1];
  const float b = (float) (mx / pw);
  const float sum = b + x[f * dim];                                    // float + float, then widened
  double val = sum;
  if (val <= 0.0) val = 1.0;
  y[f] = (float) (m * log10(val));
}

// NormalizeFeature::next (feature.cc:1453-1477)
__global__ __launch_bounds__(256) void k_normalize(const float* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int dim, double ymin, double range, int runon,
                                                   const double* __restrict__ state, const double* __restrict__ mm, float* __restrict__ y)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tmax * dim) return;
  const size_t f = idx / dim;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[idx] = 0.0f; return; }
  const double xmin = runon ? mm[2 * f] : state[2 * u], xmax = runon ? mm[2 * f + 1] : state[2 * u + 1];
  const double xrange = xmax - xmin, factor = range / xrange, add = ymin - xmin * factor;
  y[idx] = (float) ((double) x[idx] * factor + add);
}

// ThresholdFeature::next (feature.cc:1534-1560) and AmplificationFeature::next (feature.cc:3927-3941); mode 2: amplify
__global__ __launch_bounds__(256) void k_thresh_amp(const float* __restrict__ x, const int* __restrict__ nf, int U, int Tmax, int dim, double value, double thresh, int mode,
                                                    float* __restrict__ y)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tmax * dim) return;
  const size_t f = idx / dim;
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[idx] = 0.0f; return; }
  double v = x[idx];
  if (mode == 2) v = v * value;
  else if (mode > 0) { if (v >= thresh) v = value; }
  else if (mode == 0) { if (v >= thresh) v = value; else if (v <= -thresh) v = -value; }
  else { if (v <= thresh) v = value; }
  y[idx] = (float) v;
}

// SpectralResamplingFeature::next (feature.cc:1579-1602) from the host's table of low indices and float weights
__global__ __launch_bounds__(256) void k_resample(const double* __restrict__ x, const int* __restrict__ nf, const int* __restrict__ low, const float* __restrict__ wgt, int U,
                                                  int Tmax, int srcN, int outN, double* __restrict__ y)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tmax * outN) return;
  const size_t f = idx / outN; const int c = (int) (idx % outN);
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[idx] = 0.0; return; }
  const double* r = x + f * srcN;
  const int lo = low[c]; const float w = wgt[c];
  const double hiV = lo + 1 < srcN ? r[lo + 1] : 0.0;                   // the weightless term one past the end
  const float coeff = (float) ((double) w * r[lo] + (1.0 - (double) w) * hiV);
  y[idx] = coeff;
}

// SphinxMelFeature::next (feature.cc:2372-2385): row-major dgemv, k ascending
__global__ __launch_bounds__(256) void k_sphinx_mel(const double* __restrict__ x, const int* __restrict__ nf, const double* __restrict__ A, int U, int Tmax, int powerN,
                                                    int filterN, double* __restrict__ y)
{
  const size_t idx = (size_t) blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t) U * Tmax * filterN) return;
  const size_t f = idx / filterN; const int i = (int) (idx % filterN);
  const int u = (int) (f / Tmax), t = (int) (f % Tmax);
  if (t >= clampT(nf, u, Tmax)) { y[idx] = 0.0; return; }
  const double* r = x + f * powerN; const double* a = A + (size_t) i * powerN;
  double temp = 0.0;
  for (int k = 0; k < powerN; k++) temp += r[k] * a[k];
  y[idx] = temp;
}

struct FScratch { DevBuf<double> w, mm, state; DevBuf<int> low; DevBuf<float> wgt; int wN = -1; };
PerStream<FScratch> f_scratch;

void batch(const void* x, const void* y, int U, int Tmax, int dim)
{
  if (!x || !y) throw Error(DSR_E_PARAMETER, "null argument");
  if (U < 1 || Tmax < 0 || dim < 1) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d Tmax=%d dim=%d", U, Tmax, dim);
  if ((double) U * (double) Tmax * (double) dim >= 4294967296.0 * 256.0) throw Error(DSR_E_DIMENSION, "batch of %d x %d x %d elements is too large", U, Tmax, dim);
  require_device();
}
dim3 grid256(size_t n) { return dim3((unsigned) ((n + 255) / 256)); }

// the (min, max) pairs of ALog / Normalize: into the caller's state, or into scratch that starts fresh
const double* minmax(FScratch& sc, const float* x, const int32_t* nf, int U, int Tmax, int dim, int runon, double*& state, hipStream_t st)
{
  if (!state) {
    sc.state.reserve((size_t) 2 * U); state = sc.state.p;
    launch(k_minmax_init, dim3(cdiv(U, 64)), dim3(64), 0, st, state, U);
  }
  sc.mm.reserve((size_t) 2 * U * (Tmax > 0 ? Tmax : 1));
  launch(k_minmax, dim3(U), dim3(64), 0, st, x, nf, Tmax, dim, runon, state, sc.mm.p);
  return sc.mm.p;
}

void resample_table(int srcN, double ratio, int len, std::vector<int>& low, std::vector<float>& wgt)
{
  if (srcN < 1 || len < 0) throw Error(DSR_E_PARAMETER, "bad sizes %d -> %d", srcN, len);
  const int outN = len == 0 ? srcN : len;
  const double r = ratio * float(srcN) / float(outN);                                                      // feature.cc:1570
  if (r > 1.0) throw Error(DSR_E_CONSISTENCY, "Must resample the spectrum to a higher rate (ratio = %10.4f < 1.0).", r);
  low.resize(outN); wgt.resize(outN);
  for (unsigned c = 0; c < (unsigned) outN; c++) {
    const float exact = c * r;
    const unsigned lo = unsigned(c * r), hi = lo + 1;
    const float w = hi - exact;
    if (lo >= (unsigned) srcN || (hi >= (unsigned) srcN && (1.0 - w) != 0.0))
      throw Error(DSR_E_DIMENSION, "Coefficient %u of %d reads element %u of a source of %d with weight %g.", c, outN, hi, srcN, 1.0 - w);
    low[c] = (int) lo; wgt[c] = w;
  }
}

}  // namespace

struct dsr_sphinx_mel { int fftN, powerN, filterN; std::vector<double> A; DevBuf<double> dA; bool up = false; };

extern "C" {

dsr_status dsr_signal_power_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    if (Tmax == 0) return;
    const double range = float(65536) * float(65536) / 4.0;                                                 // feature.h:629-634
    launch(k_signal_power, grid256((size_t) U * Tmax), dim3(256), 0, (hipStream_t) stream, x_dev, nframes_dev, U, Tmax, dim, range, y_dev);
  });
}

dsr_status dsr_zcr_hamming_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    FScratch& sc = f_scratch.at(st);
    if (sc.wN != dim) {                                                                                     // feature.cc:3549-3551
      std::vector<double> w((size_t) dim);
      const double temp = 2. * M_PI / (double) (dim - 1);
      for (int i = 0; i < dim; i++) w[i] = 0.54 - 0.46 * cos(temp * i);
      sc.wN = -1; sc.w.upload(w, st); sc.wN = dim;
    }
    launch(k_zcr, grid256((size_t) U * Tmax), dim3(256), 0, st, x_dev, nframes_dev, sc.w.p, U, Tmax, dim, y_dev);
  });
}

int dsr_yin_kernel(int dim) { return dim <= 960 ? 4 : (dim <= 4000 ? 1 : 0); }   // waves a workgroup with the frame's four copies in at most 64 KiB of LDS; 0: from global memory

dsr_status dsr_yin_pitch_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, unsigned samplerate, float threshold, float* pitch_dev,
                             float* value_dev, int32_t* chunks_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, pitch_dev, U, Tmax, dim);
    if (dim < 2) throw Error(DSR_E_DIMENSION, "YIN needs frames of at least 2 samples, got %d.", dim);    // the reference writes yin[0] of an empty vector
    if ((long) U * Tmax > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "too many frames (%d x %d)", U, Tmax);
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    const long F = (long) U * Tmax;
    const int wpb = dsr_yin_kernel(dim);
    if (wpb) {
      int NQ = dim / 4 + 2; NQ += (4 - NQ % 16 + 16) % 16;                                                   // copies 16 banks apart: the four lanes of an address group never meet
      const size_t lds = (size_t) wpb * 4 * NQ * sizeof(float4);
      launch(k_yin<true>, dim3((unsigned) ((F + wpb - 1) / wpb)), dim3(64 * wpb), lds, st, x_dev, nframes_dev, U, Tmax, dim, NQ, samplerate, threshold,
                         pitch_dev, value_dev, chunks_dev);
    } else {
      launch(k_yin<false>, dim3((unsigned) ((F + 3) / 4)), dim3(256), 0, st, x_dev, nframes_dev, U, Tmax, dim, 0, samplerate, threshold, pitch_dev,
                         value_dev, chunks_dev);
    }
  });
}

dsr_status dsr_spike_filter_check(int dim, int tapN)
{
  return guard([&] {
    if (tapN < 3) throw Error(DSR_E_DIMENSION, "tapN should be at least 3.");                                // feature.cc:3643-3647
    if (dim < tapN) throw Error(DSR_E_DIMENSION, "Cannot filter with adcN = %d and tapN = %d.", dim, tapN);
    if (tapN % 2 == 0) throw Error(DSR_E_DIMENSION, "tapN = %d is even: the window would read one sample past the block.", tapN);
  });
}

dsr_status dsr_spike_filter_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, int tapN, float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    if (dsr_spike_filter_check(dim, tapN)) throw Error(DSR_E_DIMENSION, "%s", dsr_last_error());
    if (Tmax == 0) return;
    launch(k_spike, grid256((size_t) U * Tmax * dim), dim3(256), 0, (hipStream_t) stream, x_dev, nframes_dev, U, Tmax, dim, tapN, y_dev);
  });
}

dsr_status dsr_spike_filter2_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, unsigned width, float maxslope, float thresh, float alpha,
                                 float* meanslope_dev, int32_t* count_dev, float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    if (!meanslope_dev || !count_dev) throw Error(DSR_E_PARAMETER, "null state");
    if (dim > 16000) throw Error(DSR_E_DIMENSION, "SpikeFilter2 stages a block in LDS: %d samples exceed 16000.", dim);
    if (Tmax == 0) return;
    const float beta = 1.0 - alpha;                                                                          // feature.cc:3704
    launch(k_spike2, dim3(U), dim3(64), (size_t) dim * sizeof(float), (hipStream_t) stream, x_dev, nframes_dev, Tmax, dim, width, maxslope, thresh, alpha,
                       beta, meanslope_dev, count_dev, y_dev);
  });
}

dsr_status dsr_minmax_state_init(double* state_dev, int U, void* stream)
{
  return guard([&] {
    if (!state_dev || U < 1) throw Error(DSR_E_PARAMETER, "bad argument");
    require_device();
    launch(k_minmax_init, dim3(cdiv(U, 64)), dim3(64), 0, (hipStream_t) stream, state_dev, U);
  });
}

dsr_status dsr_alog_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double m, double a, int runon, double* state_dev, float* y_dev,
                        void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    hipStream_t st = (hipStream_t) stream;
    FScratch& sc = f_scratch.at(st);
    const double* mm = minmax(sc, x_dev, nframes_dev, U, Tmax, dim, runon, state_dev, st);
    if (Tmax > 0)
      launch(k_alog, grid256((size_t) U * Tmax), dim3(256), 0, st, x_dev, nframes_dev, U, Tmax, dim, m, pow(10.0, a), runon, state_dev, mm, y_dev);
  });
}

dsr_status dsr_normalize_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double ymin, double ymax, int runon, double* state_dev,
                             float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    hipStream_t st = (hipStream_t) stream;
    FScratch& sc = f_scratch.at(st);
    const double* mm = minmax(sc, x_dev, nframes_dev, U, Tmax, dim, runon, state_dev, st);
    if (Tmax > 0)
      launch(k_normalize, grid256((size_t) U * Tmax * dim), dim3(256), 0, st, x_dev, nframes_dev, U, Tmax, dim, ymin, ymax - ymin, runon, state_dev, mm,
                         y_dev);
  });
}

dsr_status dsr_threshold_mode(const char* mode, int* compare)
{
  return guard([&] {
    if (!mode || !compare) throw Error(DSR_E_PARAMETER, "null argument");
    const std::string s(mode);
    if (s == "upper") *compare = 1; else if (s == "lower") *compare = -1; else if (s == "both") *compare = 0;
    else throw Error(DSR_E_KEY, "Mode %s is not supported", mode);                                           // feature.cc:1524-1531
  });
}

dsr_status dsr_threshold_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double value, double thresh, int compare, float* y_dev,
                             void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    if (compare < -1 || compare > 1) throw Error(DSR_E_KEY, "Mode %d is not supported", compare);
    if (Tmax == 0) return;
    launch(k_thresh_amp, grid256((size_t) U * Tmax * dim), dim3(256), 0, (hipStream_t) stream, x_dev, nframes_dev, U, Tmax, dim, value, thresh, compare, y_dev);
  });
}

dsr_status dsr_amplify_run(const float* x_dev, const int32_t* nframes_dev, int U, int Tmax, int dim, double amplify, float* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, dim);
    if (Tmax == 0) return;
    launch(k_thresh_amp, grid256((size_t) U * Tmax * dim), dim3(256), 0, (hipStream_t) stream, x_dev, nframes_dev, U, Tmax, dim, amplify, 0.0, 2, y_dev);
  });
}

dsr_status dsr_spectral_resample_size(int srcN, double ratio, int len, int* outN)
{
  return guard([&] {
    if (!outN) throw Error(DSR_E_PARAMETER, "null argument");
    std::vector<int> low; std::vector<float> wgt; resample_table(srcN, ratio, len, low, wgt); *outN = (int) low.size();
  });
}

dsr_status dsr_spectral_resample_run(const double* x_dev, const int32_t* nframes_dev, int U, int Tmax, int srcN, double ratio, int len, double* y_dev, void* stream)
{
  return guard([&] {
    batch(x_dev, y_dev, U, Tmax, srcN > 0 ? srcN : 1);
    std::vector<int> low; std::vector<float> wgt; resample_table(srcN, ratio, len, low, wgt);
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    FScratch& sc = f_scratch.at(st);
    sc.low.upload(low, st); sc.wgt.upload(wgt, st);
    const int outN = (int) low.size();
    launch(k_resample, grid256((size_t) U * Tmax * outN), dim3(256), 0, st, x_dev, nframes_dev, sc.low.p, sc.wgt.p, U, Tmax, srcN, outN, y_dev);
  });
}

dsr_status dsr_sphinx_mel_create(unsigned fftN, unsigned powerN, float sampleRate, float lowerF, float upperF, unsigned filterN, dsr_sphinx_mel** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (fftN < 1 || powerN < 1 || filterN < 1) throw Error(DSR_E_PARAMETER, "bad sizes fftN=%u powerN=%u filterN=%u", fftN, powerN, filterN);
    std::unique_ptr<dsr_sphinx_mel> q(new dsr_sphinx_mel());
    q->fftN = (int) fftN; q->powerN = (int) powerN; q->filterN = (int) filterN; q->A.assign((size_t) filterN * powerN, 0.0);
    // feature.cc:2313-2352, as written: unnormalised triangles, k from 1, the break at the first hz > right_freq
    const double _sampleRate = sampleRate;
    const double dfreq = _sampleRate / fftN;
    if (upperF > _sampleRate / 2) throw Error(DSR_E_ERROR, "Upper frequency %f exceeds Nyquist %f", upperF, sampleRate / 2.0);
    auto mel = [](double f) { return 2595.0 * log10(1.0 + (f / 700.0)); };
    auto inv = [](double m) { return 700.0 * (pow(10.0, m / 2595.0) - 1.0); };
    const double melmax = mel(upperF), melmin = mel(lowerF), dmelbw = (melmax - melmin) / (filterN + 1);
    std::vector<double> edges(filterN + 2);
    for (unsigned n = 0; n < filterN + 2; n++) edges[n] = inv(melmin + dmelbw * n);
    for (unsigned fX = 0; fX < filterN; fX++) {
      const double left = edges[fX], center = edges[fX + 1], right = edges[fX + 2];
      for (unsigned k = 1; k < powerN; k++) {
        const double hz = k * dfreq;
        if (hz < left) continue;
        if (hz > right) break;
        const double lv = (hz - left) / (center - left), rv = (right - hz) / (right - center);
        q->A[(size_t) fX * powerN + k] = std::min(lv, rv);
      }
    }
    *out = q.release();
  });
}
void dsr_sphinx_mel_destroy(dsr_sphinx_mel* q) { delete q; }
int  dsr_sphinx_mel_size(const dsr_sphinx_mel* q) { return q ? q->filterN : 0; }
int  dsr_sphinx_mel_power_n(const dsr_sphinx_mel* q) { return q ? q->powerN : 0; }
dsr_status dsr_sphinx_mel_filters(const dsr_sphinx_mel* q, double* A_host)
{
  return guard([&] { if (!q || !A_host) throw Error(DSR_E_PARAMETER, "null argument"); memcpy(A_host, q->A.data(), q->A.size() * sizeof(double)); });
}
dsr_status dsr_sphinx_mel_apply(dsr_sphinx_mel* q, const double* x_dev, const int32_t* nframes_dev, int U, int Tmax, double* y_dev, void* stream)
{
  return guard([&] {
    if (!q) throw Error(DSR_E_PARAMETER, "null argument");
    batch(x_dev, y_dev, U, Tmax, q->powerN);
    if (Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    if (!q->up) { q->dA.upload(q->A, st); q->up = true; }
    launch(k_sphinx_mel, grid256((size_t) U * Tmax * q->filterN), dim3(256), 0, st, x_dev, nframes_dev, q->dA.p, U, Tmax, q->powerN, q->filterN, y_dev);
  });
}

}  // extern "C"
