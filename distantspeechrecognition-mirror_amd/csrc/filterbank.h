// csrc/filterbank.h -- what the filter banks' two files share: the plans behind the handles dsr_fb, dsr_prfb and dsr_stft, and the launchers
// through which the host side (filterbank.cpp: plan construction, block state, the dsr_fb_* / dsr_prfb_* / dsr_stft_* entries) reaches the
// kernels (k_filterbank.hip: kernels, launch arithmetic, dispatch).
#pragma once
#include "common.h"

namespace dsr {

// OverSampledDFTAnalysisBank / SynthesisBank
struct FbPlan {
  int M, m, r, R, D, synthesis, dctype, gain, pd, laN;
  std::vector<double> proto;
  DevBuf<float> d_proto;     // [m*M] taps as fp32
  DevBuf<float2> d_tw;       // tw[k] = e^{+2 pi j k / M}
};

// per-call frame bookkeeping: a whole-utterance call uses the plan's look-ahead and tail (laN, pd) and no history; a block of a longer stream
// (dsr_fb_analysis_block / dsr_fb_synthesis_block) carries the samples / subband frames that came before it
struct FbCall { int pd, laN; const float* hist; int histN; int tsMin; };

// PerfectReconstructionFFTAnalysisBank / SynthesisBank: 2M bands; wA, wS the pre- and post-rotations e^{-+ j pi i / 2M}, V the synthesis scratch
struct PrPlan { int M, m, r, D; DevBuf<float> h; DevBuf<float2> tw, wA, wS; DevBuf<float> V; };

// NormalFFTAnalysisBank
struct StftPlan { int M, r, D, winType; DevBuf<float> win; DevBuf<float2> tw; };

// frames an analysis bank yields for nsamp samples in blocks of D: laN source blocks of look-ahead are spent, pd zero-input frames added
__host__ __device__ inline int fb_frames(int nsamp, int D, int laN, int pd)
{ const int nblk = (nsamp + D - 1) / D; return nblk < laN ? 0 : nblk - laN + pd; }

// ---- k_filterbank.hip ----
void fb_analysis(const FbPlan& p, const FbCall& k, const float* x, const int* nsamp, int U, int C, long sampStride, int Tmax, float* X, hipStream_t st);
// analysis and fixed-weight beamformer in one pass over the channel-major weights WT [C][M/2+2]; the plan is M = 256, r = 1, m 2 or 4
void fb_analysis_beamform(const FbPlan& p, const float2* WT, const float* x, const int* nsamp, int U, int C, long sampStride, int Tmax, float* Y,
                          hipStream_t st);
void fb_synthesis(const FbPlan& p, const FbCall& k, const float* Y, const int* nframes, int U, int Tmax, long outStride, float* y, hipStream_t st);
void fb_normal_fft(const StftPlan& p, const float* x, const int* nsamp, int U, int C, long sampStride, int Tmax, float* X, hipStream_t st);
void fb_pr_analysis(const PrPlan& p, const float* x, const int* nsamp, int U, int C, long sampStride, int Tmax, float* X, hipStream_t st);
void fb_pr_synthesis(PrPlan& p, const float* Y, const int* nframes, int U, int Tmax, long outStride, float* y, hipStream_t st);
// newH = the last H items (rowLen floats each) of oldH ++ the n[stream] valid items of blk, for each of `rows` rows; at most gxMax workgroups
// per row when gxMax > 0
void fb_hist_update(const float* oldH, float* newH, const float* blk, const int* n, int rows, int rowsPerStream, long blkRowStride, int H, int rowLen,
                    bool haveOld, int gxMax, hipStream_t st);

}  // namespace dsr
