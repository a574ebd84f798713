// csrc/gcc.h -- what the time-delay estimation files share: the handle dsr_gcc, the layout of the carried state, and the functions through which
// the host side (gcc.cpp: handle construction, the per-call face, the dsr_gcc_* / dsr_cctde_* entries) reaches the kernels (k_gcc.hip).
#pragma once
#include "common.h"

struct dsr_gcc {
  int kind, N, len, C, P, interpolate, noisereduction;
  double sampleRate, alpha, beta, q;
  std::vector<int> pairs, inPair;                   // [P][2], [C]
  dsr::DevBuf<int> d_pairs, d_inPair; bool uploaded = false;
  // the per-call face (dsr_gcc_calculate / dsr_gcc_peak / dsr_gcc_get): one utterance's carried state, as a GCC object of the reference keeps it
  dsr::DevBuf<double> ownState, ownX, ownTs, ownRes; dsr::DevBuf<int> ownSad, ownValid; bool ownReady = false;
  dsr::EventTimes<4> tm;                            // dsr_gcc_set_timing: around k_gcc_spectrum and k_gcc_corr
};

namespace dsr {

constexpr double HUGE_D = 3.4028234663852886e+38;   // <math.h> HUGE (FLT_MAX): findMaximum's initial maxima (localization.cc:1299-1300)
constexpr int CC_FFT_MAX = 1 << 22;                 // CCTDE's longest transform, 4 Mi samples: 184 MB of work space a workgroup

// the carried state of U utterances, offsets in doubles
struct GLayout { size_t ts, hasN, Np, hasG, hasC, Gn, S, corr, doubles; };
inline GLayout glayout(const dsr_gcc& g, int U)
{
  const size_t u = (size_t) U, C = (size_t) g.C, P = (size_t) g.P, len = (size_t) g.len; GLayout l; size_t o = 0;
  auto take = [&](size_t n) { size_t at = o; o += (n + 1) & ~(size_t) 1; return at; };          // every part starts 16-byte aligned
  l.ts = take(u * C); l.hasN = take(u * C); l.Np = take(u * C * len); l.hasG = take(u * P); l.hasC = take(u * P);
  l.Gn = take(u * P * len * 2); l.S = take(u * P * len * 2); l.corr = take(u * P * (size_t) g.N); l.doubles = o;
  return l;
}

// ---- k_gcc.hip ----
// the kernels of GCC::calculate over a batch X [U][C][Tmax][len]; active >= 0: one calculate() call -- that pair alone, bound to the channels
// (ac1, ac2).  Throws GCCGnnSub's "speech before noise" after the launches.
void gcc_launch_run(dsr_gcc* g, const void* X_dev, int xIsDouble, const int32_t* nframes_dev, const int32_t* sad_dev, const double* timestamp_dev, int smooth,
                    double minDelay, double maxDelay, int U, int Tmax, void* state_dev, double* result_dev, int32_t* valid_dev, double* corr_dev,
                    void* xspec_dev, hipStream_t st, int active, int ac1, int ac2);
// k_gcc_find_state: findMaximum over the correlation the state carries, result [U][P][3], valid [U][P]
void gcc_launch_find_maximum(const dsr_gcc& g, double minDelay, double maxDelay, int U, void* state_dev, double* result_dev, int32_t* valid_dev, hipStream_t st);
// k_gcc_state_init: n doubles of state zeroed
void gcc_launch_state_init(double* state_dev, size_t n, hipStream_t st);
// k_cctde over nItems block pairs with the Hann window of fftLen
void cctde_launch(const float* a_dev, const float* b_dev, int nItems, int blockLen, int fftLen, int nHeldMaxCC, int sampleRate, double* delays_dev,
                  int32_t* args_dev, double* values_dev, hipStream_t st);

}  // namespace dsr
