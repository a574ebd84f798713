// csrc/src.cpp -- the host side of the sample-rate converter (dsr_src_*, include/dsr.h section 6d): the ratio, the Kaiser-windowed sinc table in
// fp64 and the C entries.  Kernels and launch: csrc/src_kernels.hip, through csrc/src.h.  The operator it stands for is SamplerateConversionFeature
// (btk/feature/feature.h:794-816, feature.cc:1607-1699), a wrapper over libsamplerate; the converter itself is defined in include/dsr.h.
#include "src.h"
#include <cmath>

namespace dsr {

static const struct { const char* name; int Z; double beta, cutoff; } kSrcMethods[] = {
  {"fastest", 10, 7.0, 0.84}, {"medium", 16, 9.5, 0.90}, {"best", 32, 12.0, 0.95}, {"zoh", 0, 0, 0}, {"linear", 0, 0, 0}};

static unsigned gcd_u(unsigned a, unsigned b) { while (b) { unsigned t = a % b; a = b; b = t; } return a; }

// I0(x), the power series: every term is positive, so the sum is as good as its last term is small
static double bessel_i0(double x)
{
  const double q = x * x / 4.0; double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; k++) { term *= q / ((double) k * k); sum += term; if (term < 1e-18 * sum) break; }
  return sum;
}

// h_p[j] = s c sinc(s c d) w(d s / Z), d = p/L - j, j = -K+1 .. K, each phase divided by its sum; row q of the table is phase (q M) mod L, so that
// the outputs n, n+1, ... of neighbouring lanes read neighbouring rows
static void src_table(SrcState& s, int Z, double beta, double c)
{
  const int L = s.L, M = s.M, K = s.K, taps = 2 * K;
  const double sc = (L < M ? (double) L / M : 1.0), i0b = bessel_i0(beta);
  s.taps = taps; s.stride = taps + 1;                                  // an odd row stride: 32 neighbouring rows start on 32 different LDS banks
  s.table.assign((size_t) L * s.stride, 0.0f);
  std::vector<double> h(taps);
  for (int q = 0; q < L; q++) {
    const int p = (int) (((int64_t) q * M) % L);
    const double frac = (double) p / L; double sum = 0.0;
    for (int jj = 0; jj < taps; jj++) {
      const double d = frac - (double) (jj - K + 1), v = sc * c * d, u = d * sc / Z;
      const double sinc = v == 0.0 ? 1.0 : std::sin(M_PI * v) / (M_PI * v);
      const double w = std::fabs(u) < 1.0 ? bessel_i0(beta * std::sqrt(1.0 - u * u)) / i0b : 0.0;
      h[jj] = sc * c * sinc * w; sum += h[jj];
    }
    for (int jj = 0; jj < taps; jj++) s.table[(size_t) q * s.stride + jj] = (float) (h[jj] / sum);
  }
}

static int64_t src_out_samples(const SrcState& s, int64_t nIn) { return nIn <= 0 ? 0 : (int64_t) (((__int128) nIn * s.L) / s.M); }

}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_src_create(unsigned srcRate, unsigned dstRate, const char* method, dsr_src** out)
{
  return guard([&] {
    if (!out || !method) throw Error(DSR_E_PARAMETER, "null argument");
    int m = -1;
    for (int i = 0; i < 5; i++) if (!strcmp(method, kSrcMethods[i].name)) m = i;
    if (m < 0) throw Error(DSR_E_CONSISTENCY, "Cannot recognize type (%s) of sample rate converter.", method);               // feature.cc:1626
    if (srcRate == 0 || dstRate == 0) throw Error(DSR_E_PARAMETER, "sample rates must be positive (%u -> %u)", srcRate, dstRate);
    const unsigned g = gcd_u(srcRate, dstRate);
    const uint64_t L = dstRate / g, M = srcRate / g;
    const bool copy = srcRate == dstRate;                                                                                 // equal rates: a copy, whatever the method
    int K = (m == SRC_ZOH || copy) ? 0 : 1;
    if (m <= SRC_BEST && !copy) {
      const uint64_t Z = (uint64_t) kSrcMethods[m].Z, k = L < M ? (Z * M + L - 1) / L : Z;                                  // K = ceil(Z / s), s = min(1, L/M)
      if (k > (1u << 22) || 2 * k * L > (1u << 22))
        throw Error(DSR_E_PARAMETER, "%u -> %u Hz (%s): a table of %llu x %llu coefficients is above 2^22", srcRate, dstRate, method,
                    (unsigned long long) L, (unsigned long long) (2 * k));
      K = (int) k;
    } else if (L > (1u << 22) || M > (1u << 22))
      throw Error(DSR_E_PARAMETER, "%u -> %u Hz (%s): the ratio %llu / %llu has a term above 2^22", srcRate, dstRate, method, (unsigned long long) L,
                  (unsigned long long) M);
    std::unique_ptr<dsr_src> s(new dsr_src());
    s->srcRate = srcRate; s->dstRate = dstRate; s->method = m; s->L = (int) L; s->M = (int) M; s->K = K; s->copy = copy;
    if (m <= SRC_BEST && !copy) src_table(*s, kSrcMethods[m].Z, kSrcMethods[m].beta, kSrcMethods[m].cutoff);
    *out = s.release();
  });
}
void dsr_src_destroy(dsr_src* s) { delete s; }

dsr_status dsr_src_ratio(const dsr_src* s, int32_t ratio[3])
{
  return guard([&] {
    if (!s || !ratio) throw Error(DSR_E_PARAMETER, "null argument");
    ratio[0] = s->L; ratio[1] = s->M; ratio[2] = s->K;
  });
}
int64_t dsr_src_out_samples(const dsr_src* s, int64_t nIn) { return s ? src_out_samples(*s, nIn) : 0; }
int64_t dsr_src_block_out_bound(const dsr_src* s, int64_t nIn) { return s ? src_out_samples(*s, (nIn < 0 ? 0 : nIn) + s->K) + 1 : 0; }

dsr_status dsr_src_table(const dsr_src* s, float* table)
{
  return guard([&] {
    if (!s || !table) throw Error(DSR_E_PARAMETER, "null argument");
    if (s->method > SRC_BEST || s->copy) throw Error(DSR_E_CONSISTENCY, "the sinc methods have a table (equal rates are a copy)");
    for (int q = 0; q < s->L; q++) memcpy(table + (size_t) (((int64_t) q * s->M) % s->L) * s->taps, &s->table[(size_t) q * s->stride], (size_t) s->taps * sizeof(float));
  });
}

size_t dsr_src_state_bytes(const dsr_src* s, int U, int C)
{
  if (!s || U <= 0 || C <= 0) return 0;
  return (size_t) U * sizeof(SrcCount) + (size_t) U * C * s->hist() * sizeof(float);
}
dsr_status dsr_src_state_init(dsr_src* s, void* state_dev, int U, int C, void* stream)
{
  return guard([&] {
    if (!s || (!state_dev && U > 0 && C > 0)) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || C < 0) throw Error(DSR_E_DIMENSION, "bad batch U=%d C=%d", U, C);
    if (U > 0 && C > 0) { require_device(); DSR_HIP(hipMemsetAsync(state_dev, 0, dsr_src_state_bytes(s, U, C), (hipStream_t) stream)); }
    s->stateU = U; s->stateC = C;
  });
}

dsr_status dsr_src_apply(dsr_src* s, const float* x_dev, const int32_t* nsamp_dev, int U, int C, int64_t inStride, void* state_dev, int flush,
                         float* y_dev, int32_t* nout_dev, int64_t outStride, void* stream)
{
  return guard([&] {
    if (!s || !x_dev || !y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || C < 0 || inStride < 0 || outStride < 0) throw Error(DSR_E_DIMENSION, "bad batch U=%d C=%d inStride=%lld outStride=%lld", U, C, (long long) inStride, (long long) outStride);
    if (inStride > 0x7fffffff || outStride > 0x7fffffff) throw Error(DSR_E_DIMENSION, "a row of more than 2^31-1 samples (%lld in, %lld out)", (long long) inStride, (long long) outStride);
    if (state_dev && (s->stateU != U || s->stateC != C))
      throw Error(DSR_E_CONSISTENCY, "SampleRateConverter: the carried state holds %d x %d rows, this call has %d x %d (initialise a state of this shape first)",
                  s->stateU, s->stateC, U, C);
    const int64_t need = state_dev ? dsr_src_block_out_bound(s, inStride) : src_out_samples(*s, inStride);
    if (outStride < need && !(state_dev && s->copy && outStride >= inStride))
      throw Error(DSR_E_DIMENSION, "outStride %lld: %lld input samples a row can give %lld outputs", (long long) outStride, (long long) inStride, (long long) need);
    require_device();
    if (U == 0 || C == 0) return;
    hipStream_t st = (hipStream_t) stream;
    if (!s->uploaded && s->method <= SRC_BEST && !s->copy) { s->d_table.upload(s->table, st); s->uploaded = true; }
    s->tm.mark(0, st);
    src_launch(*s, x_dev, nsamp_dev, U, C, (long) inStride, state_dev, flush, y_dev, nout_dev, (long) outStride, st);
    s->tm.mark(1, st);
  });
}

dsr_status dsr_src_path(const dsr_src* s, int32_t path[5])
{
  return guard([&] {
    if (!s || !path) throw Error(DSR_E_PARAMETER, "null argument");
    const SrcPath r = src_path(*s);
    path[0] = r.table; path[1] = r.input; path[2] = r.run; path[3] = (int32_t) r.ldsBytes; path[4] = r.lanePitch;
  });
}

dsr_status dsr_src_set_timing(dsr_src* s, int on)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    s->tm.enable(on != 0);
  });
}
dsr_status dsr_src_kernel_ms(const dsr_src* s, double* ms)
{
  return guard([&] {
    if (!s || !ms || !s->tm.on) throw Error(DSR_E_PARAMETER, "timing is off");
    s->tm.wait(1); *ms = s->tm.ms(0, 1);
  });
}

}  // extern "C"
