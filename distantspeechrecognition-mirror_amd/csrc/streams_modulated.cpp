// csrc/streams_modulated.cpp -- the filter banks of btk/modulated as streams (see stream_op.h).
#include "stream_op.h"

namespace {
// what the filter-bank operators' create functions share: the operator (order unchecked, `bins` bins a frame on the bank's side) owns the plan
// that `plan` creates into it, and is handed out on top of `up` only when that succeeded
template <class Op, class Plan> void bank_create(dsr_stream* up, const char* name, const char* dflt, int size, int type, int bins, dsr_stream** out, Plan plan)
{
  auto s = new_op<Op>(out, name, dflt, size, type); s->bins = bins; s->checkOrder = false;
  ok(plan(*s));
  hand_out(out, std::move(s), {up});
}
// The block-fed analysis banks.  The upstream delivers blocks of D samples (blockLen = shiftLen = D, padZeros): concatenate them again, run the
// bank into `bins` complex64 bins a frame, widen to the size_ complex128 subbands of a frame.
struct BlockAnalysisOp : dsr_stream {
  int bins = 0; bool skipEmpty = false; DevBuf<float> x; DevBuf<float2> X; DevBuf<int> ns;
  virtual int frames(int n) = 0;       // frames for n samples
  virtual dsr_status run(int n, int T) = 0;                  // x [n] (ns = n) -> X [T][bins]
  void compute() override {
    dsr_stream* u = ups[0]; const int n = u->nFrames * u->size_;
    const int T = frames(n); alloc(T);
    x.reserve(n > 0 ? n : 1); if (n > 0) DSR_HIP(hipMemcpy(x.p, u->dev.p, (size_t) n * sizeof(float), hipMemcpyDeviceToDevice));
    ns.upload(&n, 1);
    if (skipEmpty && T <= 0) return;
    X.reserve((size_t) T * bins);
    ok(run(n, T));
    op_expand_bins(X.p, T, bins, size_, d<double2>(), S0);
  }
};
}  // namespace

extern "C" {

namespace { struct AnalysisOp : BlockAnalysisOp {  // OverSampledDFTAnalysisBank: M/2+1 bins, nothing to run for an empty utterance
  dsr_fb* fb = nullptr;
  ~AnalysisOp() override { if (fb) dsr_fb_destroy(fb); }
  int frames(int n) override { return dsr_fb_analysis_frames(fb, n); }
  dsr_status run(int n, int T) override { return dsr_fb_analysis(fb, x.p, ns.p, 1, 1, n > 0 ? n : 1, T, (float*) X.p, S0); }
}; }
dsr_status dsr_analysis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, int dct, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "OverSampledDFTAnalysisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    const int D = M >> r;
    if (samp->size_ != D) throw Error(DSR_E_DIMENSION, "Input block length (%d) != _D (%d)", samp->size_, D);      // modulated.cc:373-374
    bank_create<AnalysisOp>(samp, name, "OverSampledDFTAnalysisBank", M, DSR_T_COMPLEX, M / 2 + 1, out,
                            [&](AnalysisOp& s) { s.skipEmpty = true; return dsr_fb_create(prototype, M, m, r, 0, dct, 1, &s.fb); });
  });
}
namespace { struct StftOp : BlockAnalysisOp {      // NormalFFTAnalysisBank (modulated.cc:121-257): all M bins
  dsr_stft* plan = nullptr;
  ~StftOp() override { if (plan) dsr_stft_destroy(plan); }
  int frames(int n) override { return dsr_stft_frames(plan, n); }
  dsr_status run(int n, int T) override { return dsr_stft_analysis(plan, x.p, ns.p, 1, 1, n > 0 ? n : 1, T, (float*) X.p, S0); }
}; }
dsr_status dsr_normal_fft_bank_create(dsr_stream* samp, int M, int r, int windowType, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "NormalFFTAnalysisBank"); if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    const int D = M >> r;
    if (samp->size_ != D) throw Error(DSR_E_DIMENSION, "Input block length (%d) != _D (%d)", samp->size_, D);      // modulated.cc:138-139
    bank_create<StftOp>(samp, name, "NormalFFTAnalysisBank", M, DSR_T_COMPLEX, M, out, [&](StftOp& s) { return dsr_stft_create(M, r, windowType, &s.plan); });
  });
}
namespace { struct PrAnalysisOp : BlockAnalysisOp {  // PerfectReconstructionFFTAnalysisBank (modulated.cc:686-818): all 2M bins
  dsr_prfb* fb = nullptr;
  ~PrAnalysisOp() override { if (fb) dsr_prfb_destroy(fb); }
  int frames(int n) override { return dsr_prfb_analysis_frames(fb, n); }
  dsr_status run(int n, int T) override { return dsr_prfb_analysis(fb, x.p, ns.p, 1, 1, n > 0 ? n : 1, T, (float*) X.p, S0); }
}; }
dsr_status dsr_pr_analysis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_FLOAT, "PerfectReconstructionFFTAnalysisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    const int D = M >> r;
    if (samp->size_ != D) throw Error(DSR_E_DIMENSION, "Input block length (%d) != _D (%d)", samp->size_, D);
    bank_create<PrAnalysisOp>(samp, name, "PerfectReconstructionFFTAnalysisBank", 2 * M, DSR_T_COMPLEX, 2 * M, out,
                              [&](PrAnalysisOp& s) { return dsr_prfb_create(prototype, M, m, r, &s.fb); });
  });
}
namespace {
// The synthesis banks: `bins` complex64 bins of every upstream frame in, blocks of size_ samples out.
struct BlockSynthesisOp : dsr_stream {
  int bins = 0; bool hermitian = false; DevBuf<float2> Y; DevBuf<int> nf;
  virtual int blocks(int Tin) = 0;
  virtual dsr_status run(int Tin, int nb) = 0;               // Y [Tin][bins] (nf = Tin) -> nb blocks
  void compute() override {
    dsr_stream* u = ups[0]; const int Tin = u->nFrames; const int nb = blocks(Tin); alloc(nb);
    if (nb <= 0) return;
    Y.reserve((size_t) Tin * bins);
    if (hermitian) op_pack_hermitian(u->d<double2>(), Tin, u->size_, Y.p, S0);      // frames need not be conjugate-symmetric (SubbandMMI + APAB)
    else op_pack_bins(u->d<double2>(), Tin, bins, u->size_, Y.p, S0);
    nf.upload(&Tin, 1);
    ok(run(Tin, nb));
  }
};
struct SynthesisOp : BlockSynthesisOp {  // OverSampledDFTSynthesisBank
  dsr_fb* fb = nullptr;
  ~SynthesisOp() override { if (fb) dsr_fb_destroy(fb); }
  int blocks(int Tin) override { return dsr_fb_synthesis_blocks(fb, Tin); }
  dsr_status run(int Tin, int nb) override { return dsr_fb_synthesis(fb, (const float*) Y.p, nf.p, 1, Tin, (int64_t) nb * size_, d<float>(), S0); }
};
}
dsr_status dsr_synthesis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, int dct, int gain, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_COMPLEX, "OverSampledDFTSynthesisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    if (samp->size_ != M) throw Error(DSR_E_DIMENSION, "Input size (%d) != M (%d)", samp->size_, M);
    bank_create<SynthesisOp>(samp, name, "OverSampledDFTSynthesisBank", M >> r, DSR_T_FLOAT, M / 2 + 1, out,
                             [&](SynthesisOp& s) { s.hermitian = true; return dsr_fb_create(prototype, M, m, r, 1, dct, gain, &s.fb); });
  });
}
namespace { struct PrSynthesisOp : BlockSynthesisOp {  // PerfectReconstructionFFTSynthesisBank (modulated.cc:820-970)
  dsr_prfb* fb = nullptr;
  ~PrSynthesisOp() override { if (fb) dsr_prfb_destroy(fb); }
  int blocks(int Tin) override { return dsr_prfb_synthesis_blocks(fb, Tin); }
  dsr_status run(int Tin, int nb) override { return dsr_prfb_synthesis(fb, (const float*) Y.p, nf.p, 1, Tin, (int64_t) nb * size_, d<float>(), S0); }
}; }
dsr_status dsr_pr_synthesis_bank_create(dsr_stream* samp, const double* prototype, int M, int m, int r, const char* name, dsr_stream** out)
{
  return guard([&] {
    need(samp, DSR_T_COMPLEX, "PerfectReconstructionFFTSynthesisBank"); if (!out || !prototype) throw Error(DSR_E_PARAMETER, "null argument");
    if (samp->size_ != 2 * M) throw Error(DSR_E_DIMENSION, "Input size (%d) != 2M (%d)", samp->size_, 2 * M);
    bank_create<PrSynthesisOp>(samp, name, "PerfectReconstructionFFTSynthesisBank", M >> r, DSR_T_FLOAT, 2 * M, out,
                               [&](PrSynthesisOp& s) { return dsr_prfb_create(prototype, M, m, r, &s.fb); });
  });
}

}  // extern "C"
