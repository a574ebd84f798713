// host/dsr_streams.hpp -- header-only C++ facade over the C-ABI (include/dsr.h) with the reference's class names, ctor
// argument order, pull protocol and exception types, so SWIG interface files written against btk/stream/stream.h,
// btk/feature/feature.h, btk/modulated/modulated.h and btk/beamformer/beamformer.h keep compiling.
#pragma once
#include <cmath>
#include <complex>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>
#include "../../include/dsr.h"

typedef std::string String;

// ---- exceptions (btk/common/jexception.h:41-70)
typedef enum { JERROR, JALLOCATION, JARITHMETIC, JCONSISTENCY, JDIMENSION, JINDEX, JINITIALIZATION, JIO, JITERATOR, JPYTHON,
               JKEY, JNUMERIC, JPARAMETER, JPARSE, JTYPE } error_type;
class j_error : public std::exception {
 public:
  j_error(error_type c, const std::string& w) : _what(w), code(c) {}
  const char* what() const throw() { return _what.c_str(); }
  error_type getCode() { return code; }
 protected:
  std::string _what; error_type code;
};
#define DSR_JERR(cls, val) class cls : public j_error { public: explicit cls(const std::string& w) : j_error(val, w) {} };
DSR_JERR(jallocation_error, JALLOCATION) DSR_JERR(jarithmetic_error, JARITHMETIC) DSR_JERR(jconsistency_error, JCONSISTENCY)
DSR_JERR(jdimension_error, JDIMENSION) DSR_JERR(jindex_error, JINDEX) DSR_JERR(jinitialization_error, JINITIALIZATION)
DSR_JERR(jio_error, JIO) DSR_JERR(jiterator_error, JITERATOR) DSR_JERR(jkey_error, JKEY) DSR_JERR(jnumeric_error, JNUMERIC)
DSR_JERR(jparameter_error, JPARAMETER) DSR_JERR(jparse_error, JPARSE) DSR_JERR(jtype_error, JTYPE)
#undef DSR_JERR

inline void dsr_throw(dsr_status s)
{
  if (s == DSR_OK) return;
  const std::string w = dsr_last_error();
  switch (s - 1) {
    case JALLOCATION: throw jallocation_error(w); case JARITHMETIC: throw jarithmetic_error(w); case JCONSISTENCY: throw jconsistency_error(w);
    case JDIMENSION: throw jdimension_error(w); case JINDEX: throw jindex_error(w); case JINITIALIZATION: throw jinitialization_error(w);
    case JIO: throw jio_error(w); case JITERATOR: throw jiterator_error(w); case JKEY: throw jkey_error(w); case JNUMERIC: throw jnumeric_error(w);
    case JPARAMETER: throw jparameter_error(w); case JPARSE: throw jparse_error(w); case JTYPE: throw jtype_error(w);
    default: throw j_error(JERROR, w);
  }
}

// ---- FeatureStream<item_type> (btk/stream/stream.h:36-75).  The reference's Type is a gsl_vector_X; here next() returns
// a pointer to size() items of item_type living in the operator's own buffer.
template <typename item_type>
class FeatureStream {
 public:
  virtual ~FeatureStream() { if (_h) dsr_stream_release(_h); }
  const String& name() const { return _name; }
  unsigned size() const { return (unsigned) dsr_stream_size(_h); }
  virtual const item_type* next(int frameX = -5) { const void* p = 0; size_t n = 0; dsr_throw(dsr_stream_next(_h, frameX, &p, &n)); return (const item_type*) p; }
  const item_type* current() { const void* p = 0; size_t n = 0; dsr_throw(dsr_stream_current(_h, &p, &n)); return (const item_type*) p; }
  bool isEnd() { return dsr_stream_is_end(_h) != 0; }
  virtual void reset() { dsr_throw(dsr_stream_reset(_h)); }
  virtual int frameX() const { return dsr_stream_frameX(_h); }
  dsr_stream* handle() const { return _h; }
 protected:
  FeatureStream() : _h(0) {}
  void adopt(dsr_stream* h) { _h = h; _name = dsr_stream_name(h); }
  dsr_stream* _h; String _name;
};
typedef FeatureStream<short> VectorShortFeatureStream;
typedef FeatureStream<float> VectorFloatFeatureStream;
typedef FeatureStream<double> VectorFeatureStream;
typedef FeatureStream<std::complex<double> > VectorComplexFeatureStream;
typedef std::shared_ptr<VectorShortFeatureStream> VectorShortFeatureStreamPtr;
typedef std::shared_ptr<VectorFloatFeatureStream> VectorFloatFeatureStreamPtr;
typedef std::shared_ptr<VectorFeatureStream> VectorFeatureStreamPtr;
typedef std::shared_ptr<VectorComplexFeatureStream> VectorComplexFeatureStreamPtr;

#define DSR_OP(cls, base, create_call) { dsr_stream* h = 0; dsr_throw(create_call); this->adopt(h); }

// ---- btk/feature/feature.h
class SampleFeature : public VectorFloatFeatureStream {
 public:
  SampleFeature(const String& fn = "", unsigned blockLen = 320, unsigned shiftLen = 160, bool padZeros = false, const String& nm = "Sample")
  { DSR_OP(SampleFeature, float, dsr_sample_feature_create((int) blockLen, (int) shiftLen, padZeros, nm.c_str(), &h)) if (fn != "") read(fn); }
  // feature.cc:243-393 (what btk/src/superdirectiveBeamformer.cc:150-247 calls): RIFF/WAVE PCM through the library's own reader
  unsigned read(const String& fn, int format = 0, int samplerate = 16000, int chX = 1, int chN = 1, int cfrom = 0, int to = -1, int outsamplerate = -1, float norm = 0.0) {
    int n = 0; dsr_throw(dsr_sample_feature_read(_h, fn.c_str(), format, samplerate, chX, chN, cfrom, to, outsamplerate, norm, &n)); return (unsigned) n;
  }
  int getSampleRate() const { return dsr_sample_feature_sample_rate(_h); }
  void setSamples(const float* samples, size_t n, unsigned sampleRate) { dsr_throw(dsr_sample_feature_set_samples(_h, samples, n, sampleRate)); }
};
class PreemphasisFeature : public VectorFloatFeatureStream {
 public: PreemphasisFeature(const VectorFloatFeatureStreamPtr& samp, double mu, const String& nm = "Preemphasis")
  : _s(samp) { DSR_OP(PreemphasisFeature, float, dsr_preemphasis_create(samp->handle(), mu, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class HammingFeature : public VectorFloatFeatureStream {
 public: HammingFeature(const VectorFloatFeatureStreamPtr& samp, const String& nm = "Hamming")
  : _s(samp) { DSR_OP(HammingFeature, float, dsr_hamming_create(samp->handle(), nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class FFTFeature : public VectorComplexFeatureStream {
 public: FFTFeature(const VectorFloatFeatureStreamPtr& samp, unsigned fftLen, const String& nm = "FFT")
  : _s(samp) { DSR_OP(FFTFeature, cplx, dsr_fft_create(samp->handle(), (int) fftLen, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class SpectralPowerFeature : public VectorFeatureStream {
 public: SpectralPowerFeature(const VectorComplexFeatureStreamPtr& fft, unsigned powN = 0, const String& nm = "Power")
  : _s(fft) { DSR_OP(SpectralPowerFeature, double, dsr_spectral_power_create(fft->handle(), (int) powN, nm.c_str(), &h)) }
 private: VectorComplexFeatureStreamPtr _s;
};
class VTLNFeature : public VectorFeatureStream {
 public: VTLNFeature(const VectorFeatureStreamPtr& pow, unsigned coeffN = 0, double ratio = 1.0, double edge = 1.0, int version = 1, const String& nm = "VTLN")
  : _s(pow) { DSR_OP(VTLNFeature, double, dsr_vtln_create(pow->handle(), (int) coeffN, ratio, edge, version, nm.c_str(), &h)) }
 private: VectorFeatureStreamPtr _s;
};
class MelFeature : public VectorFeatureStream {
 public: MelFeature(const VectorFeatureStreamPtr& mag, int powN = 0, float rate = 16000.0, float low = 0.0, float up = 0.0, unsigned filterN = 30, unsigned version = 1, const String& nm = "MelFFT")
  : _s(mag) { DSR_OP(MelFeature, double, dsr_mel_create(mag->handle(), powN, rate, low, up, (int) filterN, (int) version, nm.c_str(), &h)) }
 private: VectorFeatureStreamPtr _s;
};
class LogFeature : public VectorFloatFeatureStream {
 public: LogFeature(const VectorFeatureStreamPtr& mel, double m = 1.0, double a = 1.0, bool sphinxFlooring = false, const String& nm = "LogMel")
  : _s(mel) { DSR_OP(LogFeature, float, dsr_log_create(mel->handle(), m, a, sphinxFlooring, nm.c_str(), &h)) }
 private: VectorFeatureStreamPtr _s;
};
class CepstralFeature : public VectorFloatFeatureStream {
 public: CepstralFeature(const VectorFloatFeatureStreamPtr& mel, unsigned ncep = 13, int type = 1, const String& nm = "Cepstral")
  : _s(mel) { DSR_OP(CepstralFeature, float, dsr_cepstral_create(mel->handle(), (int) ncep, type, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class StorageFeature : public VectorFloatFeatureStream {
 public: StorageFeature(const VectorFloatFeatureStreamPtr& src, const String& nm = "Storage")
  : _s(src) { DSR_OP(StorageFeature, float, dsr_storage_create(src->handle(), nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class MeanSubtractionFeature : public VectorFloatFeatureStream {
 public: MeanSubtractionFeature(const VectorFloatFeatureStreamPtr& src, const VectorFloatFeatureStreamPtr& weight, double devNormFactor = 0.0, bool runon = false, const String& nm = "Mean Subtraction")
  : _s(src), _w(weight) {                                        // the reference's signature (feature.h): weight may be a null pointer
    DSR_OP(MeanSubtractionFeature, float, dsr_mean_subtraction_create(src->handle(), devNormFactor, runon, nm.c_str(), &h))
    if (_w.get()) dsr_throw(dsr_mean_subtraction_set_weight(_h, _w->handle()));
  }
  MeanSubtractionFeature(const VectorFloatFeatureStreamPtr& src, double devNormFactor = 0.0, bool runon = false, const String& nm = "Mean Subtraction")
  : _s(src) { DSR_OP(MeanSubtractionFeature, float, dsr_mean_subtraction_create(src->handle(), devNormFactor, runon, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s, _w;
};
class AdjacentFeature : public VectorFloatFeatureStream {
 public: AdjacentFeature(const VectorFloatFeatureStreamPtr& single, unsigned delta = 5, const String& nm = "Adjacent")
  : _s(single) { DSR_OP(AdjacentFeature, float, dsr_adjacent_create(single->handle(), (int) delta, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class LinearTransformFeature : public VectorFloatFeatureStream {
 public: LinearTransformFeature(const VectorFloatFeatureStreamPtr& src, unsigned sz = 0, const String& nm = "Transform")
  : _s(src) { DSR_OP(LinearTransformFeature, float, dsr_linear_transform_create(src->handle(), (int) sz, nm.c_str(), &h)) }
  void setMatrix(const float* m) { dsr_throw(dsr_linear_transform_set(_h, m)); }
 private: VectorFloatFeatureStreamPtr _s;
};

// ---- btk/feature/lpc.h: WarpMVDRFeature, BurgMVDRFeature, WarpLPCFeature, BurgLPCFeature (lpc.h:86-195,262-331)
#define DSR_LPC_OP(NAME, METHOD, KIND, DFLT) class NAME : public VectorFeatureStream { \
 public: NAME(const VectorFloatFeatureStreamPtr& src, unsigned order = 60, unsigned correlate = 0, float warp = 0.0, const String& nm = DFLT) \
  : _s(src) { DSR_OP(NAME, double, dsr_lpc_feature_create(src->handle(), (int) order, (int) correlate, warp, METHOD, KIND, nm.c_str(), &h)) } \
 private: VectorFloatFeatureStreamPtr _s; };
DSR_LPC_OP(WarpMVDRFeature, 0, 0, "MVDR")
DSR_LPC_OP(BurgMVDRFeature, 1, 0, "MVDR")
DSR_LPC_OP(WarpLPCFeature, 0, 1, "LPC")
DSR_LPC_OP(BurgLPCFeature, 1, 1, "LPC")
#undef DSR_LPC_OP
// WarpedTwiceMVDRFeature (lpc.h:205-246) and SpectralSmoothing (lpc.h:342-358)
class WarpedTwiceMVDRFeature : public VectorFeatureStream {
 public: WarpedTwiceMVDRFeature(const VectorFloatFeatureStreamPtr& src, unsigned order = 60, unsigned correlate = 0, float warp = 0.0, bool warpFactorFixed = false,
                                float sensibility = 0.1, const String& nm = "WTMVDR")
  : _s(src) { DSR_OP(WarpedTwiceMVDRFeature, double, dsr_wtmvdr_feature_create(src->handle(), (int) order, (int) correlate, warp, warpFactorFixed, sensibility, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class SpectralSmoothing : public VectorFeatureStream {
 public: SpectralSmoothing(const VectorFeatureStreamPtr& adjustTo, const VectorFeatureStreamPtr& adjustFrom, const String& nm = "Spectral Smoothing")
  : _to(adjustTo), _from(adjustFrom) { DSR_OP(SpectralSmoothing, double, dsr_spectral_smoothing_create(adjustTo->handle(), adjustFrom->handle(), nm.c_str(), &h)) }
 private: VectorFeatureStreamPtr _to, _from;
};
// FilterFeature (feature.h:1315-1410) and MergeFeature (feature.h:1423-1441): coeffA points to lenA (odd) taps
class FilterFeature : public VectorFloatFeatureStream {
 public: FilterFeature(const VectorFloatFeatureStreamPtr& src, const double* coeffA, unsigned lenA, const String& nm = "Filter")
  : _s(src) { DSR_OP(FilterFeature, float, dsr_filter_feature_create(src->handle(), coeffA, (int) lenA, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
// SamplerateConversionFeature (feature.h:794-816): include/dsr.h section 6d, the library's own converter under libsamplerate's method names
class SamplerateConversionFeature : public VectorFloatFeatureStream {
 public: SamplerateConversionFeature(const VectorFloatFeatureStreamPtr& src, unsigned sourcerate = 22050, unsigned destrate = 16000, unsigned len = 0,
                                     const String& method = "fastest", const String& nm = "SamplerateConversion")
  : _s(src) { DSR_OP(SamplerateConversionFeature, float, dsr_src_stream_create(src->handle(), sourcerate, destrate, len, method.c_str(), nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
typedef std::shared_ptr<SamplerateConversionFeature> SamplerateConversionFeaturePtr;
class MergeFeature : public VectorFloatFeatureStream {
 public: MergeFeature(const VectorFloatFeatureStreamPtr& stat, const VectorFloatFeatureStreamPtr& delta, const VectorFloatFeatureStreamPtr& deltaDelta, const String& nm = "Merge")
  : _a(stat), _b(delta), _c(deltaDelta) { DSR_OP(MergeFeature, float, dsr_merge_feature_create(stat->handle(), delta->handle(), deltaDelta->handle(), nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _a, _b, _c;
};
// ---- the scalar feature operators (feature.h:631-777, 933-970, 1594-1702, 1880-1893), include/dsr.h section 6c
class SignalPowerFeature : public VectorFloatFeatureStream {
 public: SignalPowerFeature(const VectorFloatFeatureStreamPtr& samp, const String& nm = "Signal Power")
  : _s(samp) { DSR_OP(SignalPowerFeature, float, dsr_signal_power_create(samp->handle(), nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class ALogFeature : public VectorFloatFeatureStream {
 public: ALogFeature(const VectorFloatFeatureStreamPtr& samp, double m = 1.0, double a = 4.0, bool runon = false, const String& nm = "ALog Power")
  : _s(samp) { DSR_OP(ALogFeature, float, dsr_alog_create(samp->handle(), m, a, runon, nm.c_str(), &h)) }
  void nextSpeaker() { dsr_throw(dsr_minmax_next_speaker(_h)); }
 private: VectorFloatFeatureStreamPtr _s;
};
class NormalizeFeature : public VectorFloatFeatureStream {
 public: NormalizeFeature(const VectorFloatFeatureStreamPtr& samp, double min = 0.0, double max = 1.0, bool runon = false, const String& nm = "Normalize")
  : _s(samp) { DSR_OP(NormalizeFeature, float, dsr_normalize_create(samp->handle(), min, max, runon, nm.c_str(), &h)) }
  void nextSpeaker() { dsr_throw(dsr_minmax_next_speaker(_h)); }
 private: VectorFloatFeatureStreamPtr _s;
};
class ThresholdFeature : public VectorFloatFeatureStream {
 public: ThresholdFeature(const VectorFloatFeatureStreamPtr& samp, double value = 0.0, double thresh = 1.0, const String& mode = "upper", const String& nm = "Threshold")
  : _s(samp) { DSR_OP(ThresholdFeature, float, dsr_threshold_create(samp->handle(), value, thresh, mode.c_str(), nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class SpectralResamplingFeature : public VectorFeatureStream {
 public: SpectralResamplingFeature(const VectorFeatureStreamPtr& src, double ratio = 16.0 / 22.05, unsigned len = 0, const String& nm = "Resampling")
  : _s(src) { DSR_OP(SpectralResamplingFeature, double, dsr_spectral_resampling_create(src->handle(), ratio, len, nm.c_str(), &h)) }
 private: VectorFeatureStreamPtr _s;
};
class SphinxMelFeature : public VectorFeatureStream {
 public: SphinxMelFeature(const VectorFeatureStreamPtr& mag, unsigned fftN = 512, unsigned powerN = 0, float sampleRate = 16000.0, float lowerF = 0.0, float upperF = 0.0,
                          unsigned filterN = 30, const String& nm = "Sphinx Mel Filter Bank")
  : _s(mag) { DSR_OP(SphinxMelFeature, double, dsr_sphinx_mel_feature_create(mag->handle(), fftN, powerN, sampleRate, lowerF, upperF, filterN, nm.c_str(), &h)) }
 private: VectorFeatureStreamPtr _s;
};
class ZeroCrossingRateHammingFeature : public VectorFloatFeatureStream {
 public: ZeroCrossingRateHammingFeature(const VectorFloatFeatureStreamPtr& samp, const String& nm = "Zero Crossing Rate Hamming")
  : _s(samp) { DSR_OP(ZeroCrossingRateHammingFeature, float, dsr_zcr_hamming_create(samp->handle(), nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class YINPitchFeature : public VectorFloatFeatureStream {
 public: YINPitchFeature(const VectorFloatFeatureStreamPtr& samp, unsigned samplerate = 16000, float threshold = 0.5, const String& nm = "YIN Pitch")
  : _s(samp) { DSR_OP(YINPitchFeature, float, dsr_yin_pitch_create(samp->handle(), samplerate, threshold, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class SpikeFilter : public VectorFloatFeatureStream {
 public: SpikeFilter(const VectorFloatFeatureStreamPtr& src, unsigned tapN = 3, const String& nm = "Spike Filter")
  : _s(src) { DSR_OP(SpikeFilter, float, dsr_spike_filter_create(src->handle(), tapN, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class SpikeFilter2 : public VectorFloatFeatureStream {
 public: SpikeFilter2(const VectorFloatFeatureStreamPtr& src, unsigned width = 3, float maxslope = 7000.0, float startslope = 100.0, float thresh = 15.0, float alpha = 0.2,
                      unsigned verbose = 1, const String& nm = "Spike Filter 2")
  : _s(src) { DSR_OP(SpikeFilter2, float, dsr_spike_filter2_create(src->handle(), width, maxslope, startslope, thresh, alpha, verbose, nm.c_str(), &h)) }
  unsigned spikesN() const { unsigned n = 0; dsr_throw(dsr_spike_filter2_spikes(_h, &n)); return n; }
 private: VectorFloatFeatureStreamPtr _s;
};
class AmplificationFeature : public VectorFloatFeatureStream {
 public: AmplificationFeature(const VectorFloatFeatureStreamPtr& src, double amplify = 1.0, const String& nm = "Amplification")
  : _s(src) { DSR_OP(AmplificationFeature, float, dsr_amplification_create(src->handle(), amplify, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
// ---- btk/convolution/convolution.h:40-104: impulseResponse points to P samples
class OverlapAdd : public VectorFloatFeatureStream {
 public: OverlapAdd(const VectorFloatFeatureStreamPtr& samp, const double* impulseResponse, unsigned P, unsigned fftLen = 0, const String& nm = "Overlap Add")
  : _s(samp) { DSR_OP(OverlapAdd, float, dsr_overlap_add_create(samp->handle(), impulseResponse, (int) P, (int) fftLen, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class OverlapSave : public VectorFloatFeatureStream {
 public: OverlapSave(const VectorFloatFeatureStreamPtr& samp, const double* impulseResponse, unsigned P, const String& nm = "Overlap Save")
  : _s(samp) { DSR_OP(OverlapSave, float, dsr_overlap_save_create(samp->handle(), impulseResponse, (int) P, nm.c_str(), &h)) }
  void update(const double* delta /* complex[n] */, unsigned n) { dsr_throw(dsr_overlap_save_update(_h, delta, (int) n)); }
 private: VectorFloatFeatureStreamPtr _s;
};
// ---- btk/sad/sadFeature.h: the spectral-shape operators
class EnergyDiffusionFeature : public VectorFloatFeatureStream {
 public: EnergyDiffusionFeature(const VectorFloatFeatureStreamPtr& src, const String& nm = "Energy Diffusion")
  : _s(src) { DSR_OP(EnergyDiffusionFeature, float, dsr_sad_shape_create(src->handle(), 0, 0.0f, 0.0f, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class BandEnergyRatioFeature : public VectorFloatFeatureStream {
 public: BandEnergyRatioFeature(const VectorFloatFeatureStreamPtr& src, float sampleRate, float threshF = 0.0, const String& nm = "Band Energy Ratio")
  : _s(src) { DSR_OP(BandEnergyRatioFeature, float, dsr_sad_shape_create(src->handle(), 1, sampleRate, threshF, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class NegativeEntropyFeature : public VectorFloatFeatureStream {
 public: NegativeEntropyFeature(const VectorFloatFeatureStreamPtr& src, const String& nm = "Negative Entropy")
  : _s(src) { DSR_OP(NegativeEntropyFeature, float, dsr_sad_shape_create(src->handle(), 2, 0.0f, 0.0f, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
class SignificantSubbandsFeature : public VectorFloatFeatureStream {
 public: SignificantSubbandsFeature(const VectorFloatFeatureStreamPtr& src, float thresh = 0.0, const String& nm = "Significant Subbands")
  : _s(src) { DSR_OP(SignificantSubbandsFeature, float, dsr_sad_shape_create(src->handle(), 3, 0.0f, thresh, nm.c_str(), &h)) }
 private: VectorFloatFeatureStreamPtr _s;
};
// ---- btk/sad/sad.h: the VAD metrics (:196-470), SimpleEnergyVAD (:109-133) and the hangover segmenters (:698-795) over include/dsr.h section 7b
class VADMetric {
 public:
  virtual ~VADMetric() { if (_m) dsr_sad_metric_release(_m); }
  virtual double next(int frameX = -5) { double v = 0.0; dsr_throw(dsr_sad_metric_next(_m, frameX, &v)); return v; }
  virtual void reset() { dsr_throw(dsr_sad_metric_reset(_m)); }
  virtual void nextSpeaker() { dsr_throw(dsr_sad_metric_next_speaker(_m)); }
  double score() { double v = 0.0; dsr_throw(dsr_sad_metric_score(_m, &v)); return v; }
  dsr_vad_metric* handle() const { return _m; }
 protected:
  VADMetric() : _m(0) {}
  dsr_vad_metric* _m;
 private:
  VADMetric(const VADMetric&); VADMetric& operator=(const VADMetric&);
};
typedef std::shared_ptr<VADMetric> VADMetricPtr;
class EnergyVADMetric : public VADMetric {
 public: EnergyVADMetric(const VectorFloatFeatureStreamPtr& source, double initialEnergy = 5.0e+07, double threshold = 0.5, unsigned headN = 4, unsigned tailN = 10,
                         unsigned energiesN = 200, const String& nm = "Energy VAD Metric")
  : _s(source) { dsr_throw(dsr_sad_energy_metric_create(source->handle(), initialEnergy, threshold, headN, tailN, energiesN, nm.c_str(), &_m)); }
  double energyPercentile(double percentile = 50.0) const { double v = 0.0; dsr_throw(dsr_sad_metric_energy_percentile(_m, percentile, &v)); return v; }
 private: VectorFloatFeatureStreamPtr _s;
};
typedef std::shared_ptr<EnergyVADMetric> EnergyVADMetricPtr;
template <typename ChannelType> class MultiChannelVADMetric : public VADMetric {
 public:
  void setChannel(ChannelType& chan) { dsr_throw(dsr_sad_metric_set_channel(_m, chan->handle())); _channelList.push_back(chan); }
  void clearChannel() { dsr_throw(dsr_sad_metric_clear_channel(_m)); _channelList.clear(); }
 protected: std::vector<ChannelType> _channelList;
};
typedef MultiChannelVADMetric<VectorFloatFeatureStreamPtr> FloatMultiChannelVADMetric;
typedef MultiChannelVADMetric<VectorComplexFeatureStreamPtr> ComplexMultiChannelVADMetric;
class PowerSpectrumVADMetric : public FloatMultiChannelVADMetric {
 public:
  PowerSpectrumVADMetric(unsigned fftLen, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0, const String& nm = "Power Spectrum VAD Metric")
  { dsr_throw(dsr_sad_power_metric_create(0, fftLen, sampleRate, lowCutoff, highCutoff, nm.c_str(), &_m)); }
  const std::vector<double>& getMetrics() { _p.assign(_channelList.size(), 0.0); dsr_throw(dsr_sad_metric_powers(_m, _p.data(), (int) _p.size())); return _p; }
  void setE0(double E0) { dsr_throw(dsr_sad_metric_set_e0(_m, E0)); }
 protected:
  PowerSpectrumVADMetric(int kind, unsigned fftLen, double sampleRate, double lowCutoff, double highCutoff, const String& nm)
  { dsr_throw(dsr_sad_power_metric_create(kind, fftLen, sampleRate, lowCutoff, highCutoff, nm.c_str(), &_m)); }
  std::vector<double> _p;
};
typedef std::shared_ptr<PowerSpectrumVADMetric> PowerSpectrumVADMetricPtr;
class NormalizedEnergyMetric : public PowerSpectrumVADMetric {
 public: NormalizedEnergyMetric(unsigned fftLen, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0, const String& nm = "NormalizedEnergyMetric")
  : PowerSpectrumVADMetric(1, fftLen, sampleRate, lowCutoff, highCutoff, nm) {}
};
typedef std::shared_ptr<NormalizedEnergyMetric> NormalizedEnergyMetricPtr;
class TSPSVADMetric : public PowerSpectrumVADMetric {
 public: TSPSVADMetric(unsigned fftLen, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0, const String& nm = "TSPS VAD Metric")
  : PowerSpectrumVADMetric(2, fftLen, sampleRate, lowCutoff, highCutoff, nm) {}
};
typedef std::shared_ptr<TSPSVADMetric> TSPSVADMetricPtr;
class CCCVADMetric : public ComplexMultiChannelVADMetric {
 public:
  CCCVADMetric(unsigned fftLen, unsigned nCand, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0, const String& nm = "CCC VAD Metric")
  { dsr_throw(dsr_sad_ccc_metric_create(fftLen, nCand, sampleRate, lowCutoff, highCutoff, nm.c_str(), &_m)); }
  void setNCand(unsigned nCand) { dsr_throw(dsr_sad_metric_set_ncand(_m, nCand)); }
  void setThreshold(double threshold) { dsr_throw(dsr_sad_metric_set_threshold(_m, threshold)); }
};
typedef std::shared_ptr<CCCVADMetric> CCCVADMetricPtr;
class NegentropyVADMetric : public VADMetric {
 public:
  NegentropyVADMetric(const VectorComplexFeatureStreamPtr& source, const VectorFloatFeatureStreamPtr& spectralEstimator, const String& shapeFactorFileName = "",
                      double threshold = 0.5, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0, const String& nm = "Negentropy VAD Metric")
  : _source(source), _spectralEstimator(spectralEstimator)
  { dsr_throw(dsr_sad_gg_metric_create(0, source->handle(), 0, spectralEstimator->handle(), 0, shapeFactorFileName.c_str(), -1.0, threshold, 0.95, sampleRate, lowCutoff, highCutoff, nm.c_str(), &_m)); }
 protected:
  NegentropyVADMetric(int kind, const VectorComplexFeatureStreamPtr& source1, const VectorComplexFeatureStreamPtr& source2, const VectorFloatFeatureStreamPtr& spectralEstimator1,
                      const VectorFloatFeatureStreamPtr& spectralEstimator2, const String& shapeFactorFileName, double twiddle, double threshold, double beta, double sampleRate,
                      double lowCutoff, double highCutoff, const String& nm)
  : _source(source1), _spectralEstimator(spectralEstimator1), _source2(source2), _spectralEstimator2(spectralEstimator2)
  { dsr_throw(dsr_sad_gg_metric_create(kind, source1->handle(), source2->handle(), spectralEstimator1->handle(), spectralEstimator2->handle(), shapeFactorFileName.c_str(), twiddle,
                                       threshold, beta, sampleRate, lowCutoff, highCutoff, nm.c_str(), &_m)); }
  VectorComplexFeatureStreamPtr _source; VectorFloatFeatureStreamPtr _spectralEstimator; VectorComplexFeatureStreamPtr _source2; VectorFloatFeatureStreamPtr _spectralEstimator2;
};
typedef std::shared_ptr<NegentropyVADMetric> NegentropyVADMetricPtr;
class MutualInformationVADMetric : public NegentropyVADMetric {
 public: MutualInformationVADMetric(const VectorComplexFeatureStreamPtr& source1, const VectorComplexFeatureStreamPtr& source2, const VectorFloatFeatureStreamPtr& spectralEstimator1,
                                    const VectorFloatFeatureStreamPtr& spectralEstimator2, const String& shapeFactorFileName = "", double twiddle = -1.0, double threshold = 1.3,
                                    double beta = 0.95, double sampleRate = 16000.0, double lowCutoff = -1.0, double highCutoff = -1.0,
                                    const String& nm = "Mutual Information VAD Metric")
  : NegentropyVADMetric(1, source1, source2, spectralEstimator1, spectralEstimator2, shapeFactorFileName, twiddle, threshold, beta, sampleRate, lowCutoff, highCutoff, nm) {}
};
typedef std::shared_ptr<MutualInformationVADMetric> MutualInformationVADMetricPtr;
class LikelihoodRatioVADMetric : public NegentropyVADMetric {
 public: LikelihoodRatioVADMetric(const VectorComplexFeatureStreamPtr& source1, const VectorComplexFeatureStreamPtr& source2, const VectorFloatFeatureStreamPtr& spectralEstimator1,
                                  const VectorFloatFeatureStreamPtr& spectralEstimator2, const String& shapeFactorFileName = "", double threshold = 0.0, double sampleRate = 16000.0,
                                  double lowCutoff = -1.0, double highCutoff = -1.0, const String& nm = "Mutual Information VAD Metric")
  : NegentropyVADMetric(2, source1, source2, spectralEstimator1, spectralEstimator2, shapeFactorFileName, -1.0, threshold, 0.95, sampleRate, lowCutoff, highCutoff, nm) {}
};
typedef std::shared_ptr<LikelihoodRatioVADMetric> LikelihoodRatioVADMetricPtr;
class SimpleEnergyVAD {
 public:
  SimpleEnergyVAD(VectorComplexFeatureStreamPtr& samp, double threshold, double gamma = 0.995) : _s(samp), _m(0) { dsr_throw(dsr_sad_simple_energy_create(samp->handle(), threshold, gamma, &_m)); }
  ~SimpleEnergyVAD() { if (_m) dsr_sad_metric_release(_m); }
  bool next(int frameX = -5) { double v = 0.0; dsr_throw(dsr_sad_metric_next(_m, frameX, &v)); return v > 0.5; }
  void reset() { dsr_throw(dsr_sad_metric_reset(_m)); }
  void nextSpeaker() { dsr_throw(dsr_sad_metric_next_speaker(_m)); }
 private:
  SimpleEnergyVAD(const SimpleEnergyVAD&); SimpleEnergyVAD& operator=(const SimpleEnergyVAD&);
  VectorComplexFeatureStreamPtr _s; dsr_vad_metric* _m;
};
typedef std::shared_ptr<SimpleEnergyVAD> SimpleEnergyVADPtr;
class HangoverVADFeature : public VectorFloatFeatureStream {
 public:
  HangoverVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& metric, double threshold = 0.5, unsigned headN = 4, unsigned tailN = 10,
                     const String& nm = "Hangover VAD Feature")
  : _s(source) { _create(source, metric, threshold, headN, tailN, 0, nm); }
  void nextSpeaker() { dsr_throw(dsr_sad_hangover_next_speaker(_h)); }
  int prefixN() const { int v = 0; dsr_throw(dsr_sad_hangover_prefix_n(_h, &v)); return v; }
 protected:
  HangoverVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& metric, double threshold, unsigned headN, unsigned tailN, int kind, const String& nm)
  : _s(source) { _create(source, metric, threshold, headN, tailN, kind, nm); }
  void _add(const VADMetricPtr& metric, double threshold) { dsr_throw(dsr_sad_hangover_add_metric(_h, metric->handle(), threshold)); _metrics.push_back(metric); }
  int _decisionMetric() const { int v = 0; dsr_throw(dsr_sad_hangover_decision_metric(_h, &v)); return v; }
 private:
  void _create(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& metric, double threshold, unsigned headN, unsigned tailN, int kind, const String& nm)
  { DSR_OP(HangoverVADFeature, float, dsr_sad_hangover_create(source->handle(), metric->handle(), threshold, headN, tailN, kind, nm.c_str(), &h)) _metrics.push_back(metric); }
  VectorFloatFeatureStreamPtr _s; std::vector<VADMetricPtr> _metrics;
};
typedef std::shared_ptr<HangoverVADFeature> HangoverVADFeaturePtr;
class HangoverMIVADFeature : public HangoverVADFeature {
 public:
  HangoverMIVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& energyMetric, const VADMetricPtr& mutualInformationMetric, const VADMetricPtr& powerMetric,
                       double energyThreshold = 0.5, double mutualInformationThreshold = 0.5, double powerThreshold = 0.5, unsigned headN = 4, unsigned tailN = 10,
                       const String& nm = "Hangover MIVAD Feature")
  : HangoverVADFeature(source, energyMetric, energyThreshold, headN, tailN, 1, nm) { _add(mutualInformationMetric, mutualInformationThreshold); _add(powerMetric, powerThreshold); }
  int decisionMetric() const { return _decisionMetric(); }
};
typedef std::shared_ptr<HangoverMIVADFeature> HangoverMIVADFeaturePtr;
class HangoverMultiStageVADFeature : public HangoverVADFeature {
 public:
  HangoverMultiStageVADFeature(const VectorFloatFeatureStreamPtr& source, const VADMetricPtr& energyMetric, double energyThreshold = 0.5, unsigned headN = 4, unsigned tailN = 10,
                               const String& nm = "HangoverMultiStageVADFeature")
  : HangoverVADFeature(source, energyMetric, energyThreshold, headN, tailN, 2, nm) {}
  int decisionMetric() const { return _decisionMetric(); }
  void setMetric(const VADMetricPtr& metricPtr, double threshold) { _add(metricPtr, threshold); }
};
typedef std::shared_ptr<HangoverMultiStageVADFeature> HangoverMultiStageVADFeaturePtr;

// ---- btk/localization/localization.h:118-218 and btk/TDEstimator/CCTDE.h:60-101.  The reference's gsl vectors are pointers to the items here:
// calculate() takes fftLen complex bins a spectrum, the getters return pointers into the object's own buffers (a null pointer where the
// reference has none: no noise frame yet), findMaximum() returns {delay, maxCorr, ratio}.
typedef std::shared_ptr<SampleFeature> SampleFeaturePtr;
class GCC {
 public:
  virtual ~GCC() { if (_g) dsr_gcc_destroy(_g); }
  void calculate(const std::complex<double>* spectralSample1, unsigned chan1, const std::complex<double>* spectralSample2, unsigned chan2, unsigned pair, double timestamp,
                 bool sad = false, bool smooth = true) {
    dsr_throw(dsr_gcc_calculate(_g, (const double*) spectralSample1, (int) _fftLen, (int) chan1, (const double*) spectralSample2, (int) _fftLen, (int) chan2, (int) pair,
                                timestamp, sad, smooth));
    _pair = pair;
  }
  const double* findMaximum(double minDelay = -3.4028234663852886e+38, double maxDelay = 3.4028234663852886e+38) {     // <math.h> HUGE
    int32_t valid = 0; dsr_throw(dsr_gcc_peak(_g, (int) _pair, minDelay, maxDelay, _ret, &valid)); return _ret;
  }
  double getPeakDelay() { return _ret[0]; }
  double getPeakCorr() { return _ret[1]; }
  double getRatio() { return _ret[2]; }
  const double* getNoisePowerSpectrum(unsigned chan) { return get(DSR_GCC_STATE_NOISE_POWER, chan, _fftLen / 2 + 1, false); }
  const std::complex<double>* getNoiseCrossSpectrum(unsigned pair) { return (const std::complex<double>*) get(DSR_GCC_STATE_NOISE_CROSS, pair, _fftLen + 2, false); }
  const std::complex<double>* getCrossSpectrum() { return (const std::complex<double>*) get(DSR_GCC_STATE_CROSS, _pair, _fftLen + 2, true); }
  const double* getCrossCorrelation() { return get(DSR_GCC_STATE_CORRELATION, _pair, _fftLen, true); }
  void setAlpha(double alpha) { dsr_throw(dsr_gcc_set_alpha(_g, alpha)); }
  double getAlpha() { return dsr_gcc_alpha(_g); }
 protected:
  GCC(int kind, double sampleRate, unsigned fftLen, unsigned nChan, unsigned pairs, double alpha, double beta, double q, bool interpolate, bool noisereduction)
  : _g(0), _fftLen(fftLen), _pair(0) {
    _ret[0] = _ret[1] = _ret[2] = 0.0;
    std::vector<int32_t> list(2 * (size_t) (pairs ? pairs : 1), 0);                      // calculate() names the channels of a pair
    dsr_throw(dsr_gcc_create(kind, sampleRate, (int) fftLen, (int) nChan, list.data(), (int) pairs, alpha, beta, q, interpolate, noisereduction, &_g));
  }
  const double* get(int what, unsigned index, size_t doubles, bool always) {
    _buf.assign(doubles, 0.0); int32_t exists = 0;
    dsr_throw(dsr_gcc_get(_g, what, (int) index, _buf.data(), doubles, &exists));
    return (exists || always) ? _buf.data() : 0;
  }
  dsr_gcc* _g; unsigned _fftLen, _pair; double _ret[3]; std::vector<double> _buf;
 private:
  GCC(const GCC&); GCC& operator=(const GCC&);
};
#define DSR_GCC(cls, kind) class cls : public GCC { public: \
  cls(double sampleRate = 44100.0, unsigned fftLen = 2048, unsigned nChan = 16, unsigned pairs = 6, double alpha = 0.95, double beta = 0.5, double q = 0.3, \
      bool interpolate = true, bool noisereduction = true) : GCC(kind, sampleRate, fftLen, nChan, pairs, alpha, beta, q, interpolate, noisereduction) {} }; \
  typedef std::shared_ptr<cls> cls##Ptr;
DSR_GCC(GCCRaw, DSR_GCC_RAW) DSR_GCC(GCCGnnSub, DSR_GCC_GNNSUB) DSR_GCC(GCCPhat, DSR_GCC_PHAT) DSR_GCC(GCCGnnSubPhat, DSR_GCC_GNNSUBPHAT)
DSR_GCC(GCCMLRRaw, DSR_GCC_MLRRAW) DSR_GCC(GCCMLRGnnSub, DSR_GCC_MLRGNNSUB)
#undef DSR_GCC
class CCTDE : public VectorFeatureStream {
 public:
  CCTDE(SampleFeaturePtr& samp1, SampleFeaturePtr& samp2, int fftLen = 512, unsigned nHeldMaxCC = 1, int freqLowerLimit = -1, int freqUpperLimit = -1, const String& nm = "CCTDE")
  : _s1(samp1), _s2(samp2) {
    DSR_OP(CCTDE, double, dsr_cctde_stream_create(samp1->handle(), samp2->handle(), fftLen, (int) nHeldMaxCC, freqLowerLimit, freqUpperLimit, nm.c_str(), &h))
  }
  void setTargetFrequencyRange(int freqLowerLimit, int freqUpperLimit) { dsr_throw(dsr_cctde_stream_set_target_frequency_range(_h, freqLowerLimit, freqUpperLimit)); }
  void allsamples(int fftLen = -1) { dsr_throw(dsr_cctde_stream_allsamples(_h, fftLen)); }
  virtual const double* nextX(unsigned chanX = 0, int frameX = -5) {
    const void* p = 0; size_t n = 0; dsr_throw(dsr_cctde_stream_next_x(_h, (int) chanX, frameX, &p, &n)); return (const double*) p;
  }
  const unsigned* getSampleDelays() { const int32_t* p = 0; size_t n = 0; dsr_throw(dsr_cctde_stream_get_sample_delays(_h, &p, &n)); return (const unsigned*) p; }
  const double* getCCValues() { const double* p = 0; size_t n = 0; dsr_throw(dsr_cctde_stream_get_cc_values(_h, &p, &n)); return p; }
 private: SampleFeaturePtr _s1, _s2;
};
typedef std::shared_ptr<CCTDE> CCTDEPtr;

// ---- btk/localization/MCCLocalizer.h:55-301.  Matrices are row-major double arrays here; getR() is nChan x nChan.
class SearchGridBuilder {
 public:
  SearchGridBuilder(int nChan, bool isFarField, unsigned samplingFreq = 16000) : _g(0) { make(DSR_SGB_LINEAR, nChan, isFarField, samplingFreq); }
  virtual ~SearchGridBuilder() { if (_g) dsr_sgb_destroy(_g); }
  const double* getSearchPosition() { dsr_throw(dsr_sgb_position(_g, _pos)); return _pos; }
  float maxTimeDelay() { return (float) dsr_sgb_max_time_delay(_g); }
  size_t chanN() { return (size_t) dsr_sgb_chan_n(_g); }
  unsigned samplingFrequency() { return (unsigned) dsr_sgb_sampling_frequency(_g); }
  void reset() { dsr_throw(dsr_sgb_reset(_g)); }
  virtual const double* getTimeDelays() { _delays.assign(chanN(), 0.0); dsr_throw(dsr_sgb_time_delays(_g, _delays.data())); return _delays.data(); }
  virtual bool nextSearchGrid() { int32_t more = 0; dsr_throw(dsr_sgb_next(_g, &more)); return more != 0; }
  dsr_sgb* handle() const { return _g; }
 protected:
  SearchGridBuilder(int kind, int nChan, bool isFarField, unsigned samplingFreq) : _g(0) { make(kind, nChan, isFarField, samplingFreq); }
  void make(int kind, int nChan, bool isFarField, unsigned samplingFreq) { _pos[0] = _pos[1] = _pos[2] = 0.0; dsr_throw(dsr_sgb_create(kind, nChan, isFarField, samplingFreq, &_g)); }
  dsr_sgb* _g; double _pos[3]; std::vector<double> _delays;
 private:
  SearchGridBuilder(const SearchGridBuilder&); SearchGridBuilder& operator=(const SearchGridBuilder&);
};
typedef std::shared_ptr<SearchGridBuilder> SearchGridBuilderPtr;
class SGB4LinearArray : public SearchGridBuilder {
 public:
  SGB4LinearArray(int nChan, bool isFarField, unsigned samplingFreq = 16000) : SearchGridBuilder(DSR_SGB_LINEAR, nChan, isFarField, samplingFreq) {}
  void setDistanceBtwMicrophones(float distance) { dsr_throw(dsr_sgb_set_distance(_g, distance)); }
  void setPositionsOfMicrophones(const double* mpos, int rows) { dsr_throw(dsr_sgb_set_positions(_g, mpos, rows)); }
};
typedef std::shared_ptr<SGB4LinearArray> SGB4LinearArrayPtr;
class SGB4CircularArray : public SearchGridBuilder {
 public:
  SGB4CircularArray(int nChan, bool isFarField, unsigned samplingFreq = 16000) : SearchGridBuilder(DSR_SGB_CIRCULAR, nChan, isFarField, samplingFreq) {}
  void setRadius(float radius, float height = 0.0) { dsr_throw(dsr_sgb_set_radius(_g, radius, height)); }
};
typedef std::shared_ptr<SGB4CircularArray> SGB4CircularArrayPtr;
class MCCLocalizer : public VectorFeatureStream {
 public:
  MCCLocalizer(const SearchGridBuilderPtr& sgbPtr, size_t maxSource = 1, const String& nm = "MCCSourceLocalizer") : _m(0), _sgb(sgbPtr) {
    dsr_throw(dsr_mcc_create(sgbPtr->handle(), (int) maxSource, &_m));
    open(dsr_mcc_stream_create(_m, nm.c_str(), &_h));
  }
  virtual ~MCCLocalizer() { if (_h) { dsr_stream_release(_h); _h = 0; } if (_m) dsr_mcc_destroy(_m); }
  void setChannel(const VectorFloatFeatureStreamPtr& chan) { dsr_throw(dsr_mcc_stream_set_channel(_h, chan->handle())); _chans.push_back(chan); }
  int getDelayedSample(int chanX) { return getNthBestDelayedSample(0, chanX); }
  double getMaxMCCC() { return getNthBestMCCC(0); }
  const double* getPosition() { return getNthBestPosition(0); }
  int getNthBestDelayedSample(int nth, int chanX) { return (int) get(DSR_MCC_GET_TAU, nth, (size_t) dsr_mcc_chan_n(_m))[chanX]; }
  double getNthBestMCCC(int nth) { return 1.0 - std::exp(get(DSR_MCC_GET_COST, nth, 1)[0]); }
  const double* getNthBestPosition(int nth) { return get(DSR_MCC_GET_POSITION, nth, 3); }
  const double* getEigenValues() { return get(DSR_MCC_GET_EIGEN, 0, (size_t) dsr_mcc_chan_n(_m)); }
  const double* getR() { const size_t c = (size_t) dsr_mcc_chan_n(_m); return get(DSR_MCC_GET_R, 0, c * c); }
 protected:
  MCCLocalizer(const SearchGridBuilderPtr& sgbPtr, bool normalizeVariance, const String& nm, int) : _m(0), _sgb(sgbPtr) {
    dsr_throw(dsr_mcc_create(sgbPtr->handle(), 1, &_m));
    open(dsr_mcccalc_stream_create(_m, normalizeVariance, nm.c_str(), &_h));
  }
  // a constructor that throws runs no destructor: the plan is freed here when the stream could not be made
  void open(dsr_status st) { if (st != DSR_OK) { dsr_mcc_destroy(_m); _m = 0; _h = 0; dsr_throw(st); } _name = dsr_stream_name(_h); }
  const double* get(int what, int nth, size_t doubles) { _buf.assign(doubles, 0.0); size_t n = 0; dsr_throw(dsr_mcc_stream_get(_h, what, nth, _buf.data(), doubles, &n)); return _buf.data(); }
  dsr_mcc* _m; SearchGridBuilderPtr _sgb; std::vector<VectorFloatFeatureStreamPtr> _chans; std::vector<double> _buf;
};
typedef std::shared_ptr<MCCLocalizer> MCCLocalizerPtr;
class MCCCalculator : public MCCLocalizer {
 public:
  MCCCalculator(const SearchGridBuilderPtr& sgbPtr, bool normalizeVariance = true, const String& nm = "MCCCalculator") : MCCLocalizer(sgbPtr, normalizeVariance, nm, 0) {}
  void setTimeDelays(const double* delays, int n) { dsr_throw(dsr_mcccalc_stream_set_time_delays(_h, delays, n)); }
  double getCostV() { return get(DSR_MCC_GET_COST, 0, 1)[0]; }
  double getMCCC() { return 1.0 - std::exp(getCostV()); }
};
typedef std::shared_ptr<MCCCalculator> MCCCalculatorPtr;

// ---- btk/dereverberation/dereverberation.h
class SingleChannelWPEDereverberationFeature : public VectorComplexFeatureStream {
 public:
  SingleChannelWPEDereverberationFeature(VectorComplexFeatureStreamPtr& samples, unsigned lowerN, unsigned upperN, unsigned iterationsN = 2, double loadDb = -20.0,
                                         double bandWidth = 0.0, double sampleRate = 16000.0, const String& nm = "SingleChannelWPEDereverberationFeature")
  : _s(samples) { DSR_OP(SingleChannelWPEDereverberationFeature, cplx, dsr_wpe_single_stream_create(samples->handle(), (int) lowerN, (int) upperN, (int) iterationsN, loadDb, bandWidth, sampleRate, nm.c_str(), &h)) }
  void nextSpeaker() { reset(); }
 private: VectorComplexFeatureStreamPtr _s;
};

// ---- btk/postfilter/postfilter.h:95-126
class ZelinskiPostFilter : public VectorComplexFeatureStream {
 public:
  ZelinskiPostFilter(VectorComplexFeatureStreamPtr& output, unsigned fftLen, double alpha = 0.6, int type = 2, int minFrames = 0, const String& nm = "ZelinskPostFilter")
  : _s(output) { DSR_OP(ZelinskiPostFilter, cplx, dsr_zelinski_stream_create(output->handle(), (int) fftLen, alpha, type, minFrames, nm.c_str(), &h)) }
  void setSnapShotChannel(VectorComplexFeatureStreamPtr& chan) { dsr_throw(dsr_zelinski_stream_set_channel(_h, chan->handle())); _chans.push_back(chan); }
  void setArrayManifoldVector(unsigned fbinX, const double* vec, unsigned chanN, bool halfBandShift = false, unsigned NC = 1)
  { (void) halfBandShift; (void) NC; dsr_throw(dsr_zelinski_stream_set_manifold(_h, (int) fbinX, vec, (int) chanN)); }
 private: VectorComplexFeatureStreamPtr _s; std::vector<VectorComplexFeatureStreamPtr> _chans;
};

// ---- btk/postfilter/postfilter.h:128-204.  The noise coherence setters fix the array size at their first call (chanN).
class McCowanPostFilter : public VectorComplexFeatureStream {
 public:
  McCowanPostFilter(VectorComplexFeatureStreamPtr& output, unsigned fftLen, double alpha = 0.6, int type = 2, int minFrames = 0, float threshold = 0.99f,
                    const String& nm = "McCowanPostFilterPtr")
  : _s(output) { DSR_OP(McCowanPostFilter, cplx, dsr_mccowan_stream_create(output->handle(), (int) fftLen, alpha, type, minFrames, threshold, nm.c_str(), &h)) }
  void setSnapShotChannel(VectorComplexFeatureStreamPtr& chan) { dsr_throw(dsr_zelinski_stream_set_channel(_h, chan->handle())); _chans.push_back(chan); }
  void setArrayManifoldVector(unsigned fbinX, const double* vec, unsigned chanN, bool halfBandShift = false, unsigned NC = 1)
  { (void) halfBandShift; (void) NC; dsr_throw(dsr_zelinski_stream_set_manifold(_h, (int) fbinX, vec, (int) chanN)); }
  void setDiffuseNoiseModel(const double* micPositions /* [chanN][3] */, unsigned chanN, double sampleRate, double sspeed = 343740.0)
  { _C = chanN; dsr_throw(dsr_mccowan_stream_set_noise(_h, 1, 0, micPositions, (int) chanN, sampleRate, sspeed)); }
  void setNoiseSpatialSpectralMatrix(unsigned fbinX, const double* Rnn /* [chanN][chanN] complex */, unsigned chanN)
  { _C = chanN; dsr_throw(dsr_mccowan_stream_set_noise(_h, 0, (int) fbinX, Rnn, (int) chanN, 0.0, 0.0)); }
  void setAllLevelsOfDiagonalLoading(float diagonalWeight) { dsr_throw(dsr_mccowan_stream_set_noise(_h, 2, -1, 0, (int) _C, diagonalWeight, 0.0)); }
  void setLevelOfDiagonalLoading(unsigned fbinX, float diagonalWeight) { dsr_throw(dsr_mccowan_stream_set_noise(_h, 2, (int) fbinX, 0, (int) _C, diagonalWeight, 0.0)); }
  void divideAllNonDiagonalElements(float myu) { dsr_throw(dsr_mccowan_stream_set_noise(_h, 3, 0, 0, (int) _C, myu, 0.0)); }
 protected:
  McCowanPostFilter(VectorComplexFeatureStreamPtr& output) : _s(output), _C(0) {}
  VectorComplexFeatureStreamPtr _s; std::vector<VectorComplexFeatureStreamPtr> _chans; unsigned _C = 0;
};
class LefkimmiatisPostFilter : public McCowanPostFilter {
 public:
  LefkimmiatisPostFilter(VectorComplexFeatureStreamPtr& output, unsigned fftLen, double minSV = 1.0E-8, unsigned fbinX1 = 0, double alpha = 0.6, int type = 2,
                         int minFrames = 0, float threshold = 0.99f, const String& nm = "LefkimmiatisPostFilte")
  : McCowanPostFilter(output) { DSR_OP(LefkimmiatisPostFilter, cplx, dsr_lefkimmiatis_stream_create(output->handle(), (int) fftLen, minSV, (int) fbinX1, alpha, type, minFrames, threshold, nm.c_str(), &h)) }
  void calcInverseNoiseSpatialSpectralMatrix() {}          // implied: refreshed whenever the coherence matrices or the manifold change
};

// ---- btk/postfilter/spectralsubtraction.h:70-166.  An utterance is computed at its first next(): control calls act from the next reset() on.
class SpectralSubtractor : public VectorComplexFeatureStream {
 public:
  SpectralSubtractor(unsigned fftLen, bool halfBandShift = false, float ft = 1.0f, float flooringV = 0.001f, const String& nm = "SpectralSubtractor")
  { DSR_OP(SpectralSubtractor, cplx, dsr_specsub_stream_create((int) fftLen, halfBandShift ? 1 : 0, ft, flooringV, nm.c_str(), &h)) }
  void setChannel(VectorComplexFeatureStreamPtr& chan, double alpha = -1) { dsr_throw(dsr_specsub_stream_set_channel(_h, chan ? chan->handle() : 0, alpha)); _chans.push_back(chan); }
  void setNoiseOverEstimationFactor(float ft) { ctl(0, ft); }
  void startTraining() { ctl(1); }
  void stopTraining() { ctl(2); }
  void startNoiseSubtraction() { ctl(3); }
  void stopNoiseSubtraction() { ctl(4); }
  void clear() { ctl(5); }
  void clearNoiseSamples() { ctl(6); }
  bool readNoiseFile(const String& fn, unsigned idx = 0) { ctl(7, 0.0, fn.c_str(), (int) idx); return true; }
  bool writeNoiseFile(const String& fn, unsigned idx = 0) { ctl(8, 0.0, fn.c_str(), (int) idx); return true; }
 private:
  void ctl(int what, double v = 0.0, const char* fn = 0, int idx = 0) { dsr_throw(dsr_specsub_stream_control(_h, what, v, fn, idx)); }
  std::vector<VectorComplexFeatureStreamPtr> _chans;
};
typedef std::shared_ptr<SpectralSubtractor> SpectralSubtractorPtr;
class WienerFilter : public VectorComplexFeatureStream {
 public:
  WienerFilter(VectorComplexFeatureStreamPtr& targetSignal, VectorComplexFeatureStreamPtr& noiseSignal, bool halfBandShift = false, float alpha = 0.0f,
               float flooringV = 0.001f, double beta = 1.0, const String& nm = "WienerFilter")
  : _t(targetSignal), _n(noiseSignal)
  { DSR_OP(WienerFilter, cplx, dsr_wiener_stream_create(_t ? _t->handle() : 0, _n ? _n->handle() : 0, halfBandShift ? 1 : 0, alpha, flooringV, beta, nm.c_str(), &h)) }
  void setNoiseAmplificationFactor(double beta) { dsr_throw(dsr_wiener_stream_control(_h, 0, beta)); }
  void startUpdatingNoisePSD() { dsr_throw(dsr_wiener_stream_control(_h, 1, 0.0)); }
  void stopUpdatingNoisePSD() { dsr_throw(dsr_wiener_stream_control(_h, 2, 0.0)); }
 private: VectorComplexFeatureStreamPtr _t, _n;
};
typedef std::shared_ptr<WienerFilter> WienerFilterPtr;

// ---- btk/postfilter/binauralprocessing.h.  dPowerCoeff: the reference's default `1/15` is integer division, 0.0 -- kept; every cost function is
// then degenerate, so callers pass a value.
class BinaryMaskFilter : public VectorComplexFeatureStream {
 public:
  BinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float threshold, float alpha,
                   float dEta = 0.01f, const String& nm = "BinaryMaskFilter")
  : _l(srcL), _r(srcR), _M(M) { create(0, chanX, threshold, alpha, dEta, 0.0f, nm); }
  void setThreshold(float threshold) { dsr_throw(dsr_binmask_stream_set_threshold(_h, threshold)); }
  void setThresholds(const double* thresholds, unsigned n) { dsr_throw(dsr_binmask_stream_set_thresholds(_h, thresholds, (int) n)); }
  double getThreshold() { double v = 0.0; dsr_throw(dsr_binmask_stream_threshold(_h, &v)); return v; }
  bool getThresholds(std::vector<double>& out) { int32_t ex = 0; out.assign(_M / 2 + 1, 0.0); dsr_throw(dsr_binmask_stream_thresholds(_h, out.data(), (int) out.size(), &ex)); return ex != 0; }
 protected:
  BinaryMaskFilter(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M) : _l(srcL), _r(srcR), _M(M) {}
  void create(int kind, unsigned chanX, float threshold, float alpha, float dEta, float dPowerCoeff, const String& nm)
  { DSR_OP(BinaryMaskFilter, cplx, dsr_binmask_stream_create(kind, chanX, _l ? _l->handle() : 0, _r ? _r->handle() : 0, _M, threshold, alpha, dEta, dPowerCoeff, nm.c_str(), &h)) }
  VectorComplexFeatureStreamPtr _l, _r; unsigned _M;
};
typedef std::shared_ptr<BinaryMaskFilter> BinaryMaskFilterPtr;
class KimBinaryMaskFilter : public BinaryMaskFilter {
 public:
  KimBinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float threshold, float alpha,
                      float dEta = 0.01f, float dPowerCoeff = 1 / 15, const String& nm = "KimBinaryMaskFilter")
  : BinaryMaskFilter(srcL, srcR, M) { create(1, chanX, threshold, alpha, dEta, dPowerCoeff, nm); }
};
typedef std::shared_ptr<KimBinaryMaskFilter> KimBinaryMaskFilterPtr;
class IIDBinaryMaskFilter : public BinaryMaskFilter {
 public:
  IIDBinaryMaskFilter(unsigned chanX, VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float threshold, float alpha,
                      float dEta = 0.01f, const String& nm = "IIDBinaryMaskFilter")
  : BinaryMaskFilter(srcL, srcR, M) { create(2, chanX, threshold, alpha, dEta, 0.0f, nm); }
};
typedef std::shared_ptr<IIDBinaryMaskFilter> IIDBinaryMaskFilterPtr;
class KimITDThresholdEstimator : public VectorComplexFeatureStream {
 public:
  KimITDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float minThreshold = 0, float maxThreshold = 0,
                           float width = 0.02f, float minFreq = -1, float maxFreq = -1, int sampleRate = -1, float dEta = 0.01f, float dPowerCoeff = 1 / 15,
                           const String& nm = "KimITDThresholdEstimator")
  : _l(srcL), _r(srcR), _M(M) { create(0, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, nm); }
  double calcThreshold() { double v = 0.0; dsr_throw(dsr_thest_stream_calc_threshold(_h, &v)); return v; }
  double getThreshold() { double v = 0.0; dsr_throw(dsr_thest_stream_threshold(_h, &v)); return v; }
  std::vector<double> getCostFunction(unsigned freqX = 0)
  { std::vector<double> c((size_t) dsr_thest_stream_n_cand(_h) + 1, 0.0); size_t n = 0; dsr_throw(dsr_thest_stream_get_cost_function(_h, freqX, c.data(), c.size(), &n)); c.resize(n); return c; }
 protected:
  KimITDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, int) : _l(srcL), _r(srcR), _M(M) {}
  void create(int kind, float minT, float maxT, float width, float minFreq, float maxFreq, int sampleRate, float dEta, float dPowerCoeff, const String& nm)
  { DSR_OP(KimITDThresholdEstimator, cplx, dsr_thest_stream_create(kind, _l ? _l->handle() : 0, _r ? _r->handle() : 0, _M, minT, maxT, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, nm.c_str(), &h)) }
  VectorComplexFeatureStreamPtr _l, _r; unsigned _M;
};
typedef std::shared_ptr<KimITDThresholdEstimator> KimITDThresholdEstimatorPtr;
class IIDThresholdEstimator : public KimITDThresholdEstimator {
 public:
  IIDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float minThreshold = 0, float maxThreshold = 0,
                        float width = 0.02f, float minFreq = -1, float maxFreq = -1, int sampleRate = -1, float dEta = 0.01f, float dPowerCoeff = 1 / 15,
                        const String& nm = "IIDThresholdEstimator")
  : KimITDThresholdEstimator(srcL, srcR, M, 0) { create(1, minThreshold, maxThreshold, width, minFreq, maxFreq, sampleRate, dEta, dPowerCoeff, nm); }
};
typedef std::shared_ptr<IIDThresholdEstimator> IIDThresholdEstimatorPtr;
class FDIIDThresholdEstimator : public KimITDThresholdEstimator {
 public:
  FDIIDThresholdEstimator(VectorComplexFeatureStreamPtr& srcL, VectorComplexFeatureStreamPtr& srcR, unsigned M, float minThreshold = 0, float maxThreshold = 0,
                          float width = 1000, float dEta = 0.01f, float dPowerCoeff = 1 / 15, const String& nm = "FDIIDThresholdEstimator")
  : KimITDThresholdEstimator(srcL, srcR, M, 0) { create(2, minThreshold, maxThreshold, width, -1, -1, -1, dEta, dPowerCoeff, nm); }
  std::vector<double> getThresholds() { std::vector<double> t(_M / 2 + 1, 0.0); dsr_throw(dsr_thest_stream_thresholds(_h, t.data(), (int) t.size())); return t; }
};
typedef std::shared_ptr<FDIIDThresholdEstimator> FDIIDThresholdEstimatorPtr;

// ---- btk/dereverberation/dereverberation.h:89-174
class MultiChannelWPEDereverberation {
 public:
  MultiChannelWPEDereverberation(unsigned subbandsN, unsigned channelsN, unsigned lowerN, unsigned upperN, unsigned iterationsN = 2, double loadDb = -20.0,
                                 double bandWidth = 0.0, double sampleRate = 16000.0)
  : _subbandsN(subbandsN), _channelsN(channelsN), _lowerN(lowerN), _upperN(upperN), _iterationsN(iterationsN), _loadDb(loadDb), _bandWidth(bandWidth),
    _sampleRate(sampleRate), _first(-1)
  { if (bandWidth > sampleRate / 2.0) throw jdimension_error("Bandwidth is greater than the Nyquist rate.\n"); }
  unsigned size() const { return _subbandsN; }
  void setInput(VectorComplexFeatureStreamPtr& samples) { if (_sources.size() == _channelsN) throw jallocation_error("Channel capacity exceeded."); _sources.push_back(samples); }
  void reset() { _first = -1; for (size_t i = 0; i < _features.size(); i++) dsr_throw(dsr_stream_reset(_features[i])); }
  void nextSpeaker() { reset(); }
 private:
  friend class MultiChannelWPEDereverberationFeature;
  // the channel whose feature asks for a frame first decides the filter all channels go through (dereverberation.cc:381)
  void asked(int channelX) { if (_first < 0) { _first = channelX; for (size_t i = 0; i < _features.size(); i++) dsr_throw(dsr_wpe_multi_feature_set_filter_channel(_features[i], channelX)); } }
  unsigned _subbandsN, _channelsN, _lowerN, _upperN, _iterationsN; double _loadDb, _bandWidth, _sampleRate; int _first;
  std::vector<VectorComplexFeatureStreamPtr> _sources; std::vector<dsr_stream*> _features;
};
typedef std::shared_ptr<MultiChannelWPEDereverberation> MultiChannelWPEDereverberationPtr;
class MultiChannelWPEDereverberationFeature : public VectorComplexFeatureStream {
 public:
  MultiChannelWPEDereverberationFeature(MultiChannelWPEDereverberationPtr& source, unsigned channelX, const String& nm = "MultiChannelWPEDereverberationFeature")
  : _source(source), _channelX((int) channelX) {
    std::vector<dsr_stream*> in; for (size_t i = 0; i < source->_sources.size(); i++) in.push_back(source->_sources[i]->handle());
    DSR_OP(MultiChannelWPEDereverberationFeature, cplx, dsr_wpe_multi_feature_create(in.data(), (int) in.size(), (int) channelX, (int) source->_lowerN, (int) source->_upperN,
           (int) source->_iterationsN, source->_loadDb, source->_bandWidth, source->_sampleRate, nm.c_str(), &h))
    source->_features.push_back(_h);
    if (source->_first >= 0) dsr_throw(dsr_wpe_multi_feature_set_filter_channel(_h, source->_first));
  }
  const std::complex<double>* next(int frameX = -5) { _source->asked(_channelX); return VectorComplexFeatureStream::next(frameX); }
  void reset() { _source->reset(); }
 private: MultiChannelWPEDereverberationPtr _source; int _channelX;
};

// ---- btk/cancelVP/cancelVP.h:264-339, defaults of cancelVP.i:161-165, :195-199.  The adaptive state outlives reset() (cancelVP.h:134-142).
// In the reference the base is BlockKalmanFilterEchoCancellationFeature, which this header does not carry.
class InformationFilterEchoCancellationFeature : public VectorComplexFeatureStream {
 public:
  InformationFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded, unsigned sampleN = 1,
                                           double beta = 0.95, double sigmau2 = 10e-4, double sigmak2 = 5.0, double snrTh = 2.0, double engTh = 100.0, double smooth = 0.9,
                                           double loading = 1.0e-02, double amp4play = 1.0, const String& nm = "DTDBlockKFEchoCanceller")
  : _aec(0), _played(played), _recorded(recorded) { create(0, sampleN, beta, sigmau2, sigmak2, snrTh, engTh, smooth, loading, amp4play, nm); }
  ~InformationFilterEchoCancellationFeature() { if (_h) { dsr_stream_release(_h); _h = 0; } if (_aec) dsr_aec_destroy(_aec); }
  // [fftLen/2+1][sampleN] complex
  std::vector<std::complex<double> > filterCoefficients() {
    std::vector<std::complex<double> > r((size_t) (size() / 2 + 1) * dsr_aec_sample_n(_aec)); size_t n = 0;
    dsr_throw(dsr_aec_stream_get(_h, DSR_AEC_STATE_FILTER, (double*) r.data(), r.size() * 2, &n)); return r;
  }
 protected:
  InformationFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded, int)
  : _aec(0), _played(played), _recorded(recorded) {}
  void create(int squareRoot, unsigned sampleN, double beta, double sigmau2, double sigmak2, double snrTh, double engTh, double smooth, double loading, double amp4play,
              const String& nm) {
    dsr_throw(dsr_aec_create_info(squareRoot, (int) _played->size(), (int) sampleN, &_aec));
    dsr_throw(dsr_aec_set_block(_aec, beta, sigmau2, sigmak2, snrTh, amp4play));
    dsr_throw(dsr_aec_set_info(_aec, snrTh, engTh, smooth, loading));
    DSR_OP(InformationFilterEchoCancellationFeature, cplx, dsr_aec_stream_create(_aec, _played->handle(), _recorded->handle(), nm.c_str(), &h))
  }
  dsr_aec* _aec; VectorComplexFeatureStreamPtr _played, _recorded;
};
typedef std::shared_ptr<InformationFilterEchoCancellationFeature> InformationFilterEchoCancellationFeaturePtr;
class SquareRootInformationFilterEchoCancellationFeature : public InformationFilterEchoCancellationFeature {
 public:
  SquareRootInformationFilterEchoCancellationFeature(const VectorComplexFeatureStreamPtr& played, const VectorComplexFeatureStreamPtr& recorded, unsigned sampleN = 1,
                                                     double beta = 0.95, double sigmau2 = 10e-4, double sigmak2 = 5.0, double snrTh = 2.0, double engTh = 100.0,
                                                     double smooth = 0.9, double loading = 1.0e-02, double amp4play = 1.0,
                                                     const String& nm = "Square Root Information Filter Echo Cancellation Feature")
  : InformationFilterEchoCancellationFeature(played, recorded, 0) { create(1, sampleN, beta, sigmau2, sigmak2, snrTh, engTh, smooth, loading, amp4play, nm); }
};
typedef std::shared_ptr<SquareRootInformationFilterEchoCancellationFeature> SquareRootInformationFilterEchoCancellationFeaturePtr;

// ---- btk/modulated/modulated.h
class NormalFFTAnalysisBank : public VectorComplexFeatureStream {
 public:
  NormalFFTAnalysisBank(VectorFloatFeatureStreamPtr& samp, unsigned M, unsigned r = 1, unsigned windowType = 1, const String& nm = "NormalFFTAnalysisBank")
  : _s(samp), _M(M) { DSR_OP(NormalFFTAnalysisBank, cplx, dsr_normal_fft_bank_create(samp->handle(), (int) M, (int) r, (int) windowType, nm.c_str(), &h)) }
  unsigned fftLen() const { return _M; }
 private: VectorFloatFeatureStreamPtr _s; unsigned _M;
};
class PerfectReconstructionFFTAnalysisBank : public VectorComplexFeatureStream {
 public:
  PerfectReconstructionFFTAnalysisBank(VectorFloatFeatureStreamPtr& samp, const double* prototype, unsigned M, unsigned m, unsigned r,
                                       const String& nm = "PerfectReconstructionFFTAnalysisBank")
  : _s(samp), _M(M) { DSR_OP(PerfectReconstructionFFTAnalysisBank, cplx, dsr_pr_analysis_bank_create(samp->handle(), prototype, (int) M, (int) m, (int) r, nm.c_str(), &h)) }
  unsigned fftLen() const { return 2 * _M; }
  unsigned nBlocks() const { return 4; }
  unsigned subSampRate() const { return 2; }
 private: VectorFloatFeatureStreamPtr _s; unsigned _M;
};
class PerfectReconstructionFFTSynthesisBank : public VectorFloatFeatureStream {
 public:
  PerfectReconstructionFFTSynthesisBank(VectorComplexFeatureStreamPtr& samp, const double* prototype, unsigned M, unsigned m, unsigned r = 0,
                                        const String& nm = "PerfectReconstructionFFTSynthesisBank")
  : _s(samp) { DSR_OP(PerfectReconstructionFFTSynthesisBank, float, dsr_pr_synthesis_bank_create(samp->handle(), prototype, (int) M, (int) m, (int) r, nm.c_str(), &h)) }
 private: VectorComplexFeatureStreamPtr _s;
};
class OverSampledDFTAnalysisBank : public VectorComplexFeatureStream {
 public:
  OverSampledDFTAnalysisBank(VectorFloatFeatureStreamPtr& samp, const double* prototype, unsigned M, unsigned m, unsigned r,
                             unsigned delayCompensationType = 0, const String& nm = "OverSampledDFTAnalysisBank")
  : _s(samp), _M(M) { DSR_OP(OverSampledDFTAnalysisBank, cplx, dsr_analysis_bank_create(samp->handle(), prototype, (int) M, (int) m, (int) r, (int) delayCompensationType, nm.c_str(), &h)) }
  unsigned fftLen() const { return _M; }
 private: VectorFloatFeatureStreamPtr _s; unsigned _M;
};
class OverSampledDFTSynthesisBank : public VectorFloatFeatureStream {
 public:
  OverSampledDFTSynthesisBank(VectorComplexFeatureStreamPtr& samp, const double* prototype, unsigned M, unsigned m, unsigned r = 0,
                              unsigned delayCompensationType = 0, int gainFactor = 1, const String& nm = "OverSampledDFTSynthesisBank")
  : _s(samp) { DSR_OP(OverSampledDFTSynthesisBank, float, dsr_synthesis_bank_create(samp->handle(), prototype, (int) M, (int) m, (int) r, (int) delayCompensationType, gainFactor, nm.c_str(), &h)) }
 private: VectorComplexFeatureStreamPtr _s;
};

// ---- btk/beamformer/beamformer.h: SubbandDS / SubbandGSC / SubbandMVDR
class SubbandDS : public VectorComplexFeatureStream {
 public:
  SubbandDS(unsigned fftLen = 512, bool halfBandShift = false, const String& nm = "SubbandDS") : _fftLen(fftLen), _hbs(halfBandShift), _nm(nm), _w(0), _mode(0) {}
  ~SubbandDS() { if (_w) dsr_bf_destroy(_w); }
  void setChannel(VectorComplexFeatureStreamPtr& chan) { _channelList.push_back(chan); }
  unsigned chanN() const { return (unsigned) _channelList.size(); }
  void calcArrayManifoldVectors(double sampleRate, const double* delays) { dsr_throw(dsr_bf_calc_array_manifold(weights(), sampleRate, delays)); }
  virtual const std::complex<double>* next(int frameX = -5) {
    if (!_h) throw j_error(JERROR, "call calcArrayManifoldVectorsX() once");
    return VectorComplexFeatureStream::next(frameX);
  }
 protected:
  dsr_bf* weights() {
    if (!_w) {
      dsr_throw(dsr_bf_create((int) _fftLen, (int) chanN(), _hbs, &_w)); dsr_throw(dsr_bf_select(_w, _mode));
      dsr_stream* h = 0; dsr_throw(dsr_subband_bf_create(_w, _nm.c_str(), &h)); adopt(h);
      for (size_t i = 0; i < _channelList.size(); i++) dsr_throw(dsr_subband_bf_set_channel(_h, _channelList[i]->handle()));
    }
    return _w;
  }
  unsigned _fftLen; bool _hbs; String _nm; dsr_bf* _w; int _mode; std::vector<VectorComplexFeatureStreamPtr> _channelList;
};
class SubbandGSC : public SubbandDS {
 public:
  SubbandGSC(unsigned fftLen = 512, bool halfBandShift = false, const String& nm = "SubbandGSC") : SubbandDS(fftLen, halfBandShift, nm) { _mode = 2; }
  void calcGSCWeights(double sampleRate, const double* delaysT) { dsr_throw(dsr_bf_calc_gsc_weights(weights(), sampleRate, delaysT)); }
  void setActiveWeights_f(unsigned fbinX, const double* packedWeight) { dsr_throw(dsr_bf_set_active_weights(weights(), (int) fbinX, packedWeight)); }
  void zeroActiveWeights() { dsr_throw(dsr_bf_zero_active_weights(weights())); }
};
class SubbandMVDR : public SubbandDS {
 public:
  SubbandMVDR(unsigned fftLen = 512, bool halfBandShift = false, const String& nm = "SubbandMVDR") : SubbandDS(fftLen, halfBandShift, nm) {
    if (halfBandShift) throw jallocation_error("halfBandShift==true is not yet supported");
    _mode = 1;
  }
  bool setDiffuseNoiseModel(const double* micPositions, double sampleRate, double sspeed = 343740.0) { dsr_throw(dsr_bf_set_diffuse_noise_model(weights(), micPositions, sampleRate, sspeed)); return true; }
  void divideAllNonDiagonalElements(float myu) { dsr_throw(dsr_bf_divide_nondiagonal(weights(), myu)); }
  void setAllLevelsOfDiagonalLoading(float w) { dsr_throw(dsr_bf_diagonal_loading(weights(), w)); }
  bool calcMVDRWeights(double sampleRate, double dThreshold = 1.0E-8, bool calcInverseMatrix = true) { (void) calcInverseMatrix; dsr_throw(dsr_bf_calc_mvdr_weights(weights(), sampleRate, dThreshold)); return true; }
};
// ---- beamformer.h:264-312 (SubbandMMI): one GSC per source, Zelinski post-filter, binary mask; matrices row-major as gsl_matrix
class SubbandMMI : public VectorComplexFeatureStream {
 public:
  SubbandMMI(unsigned fftLen = 512, bool halfBandShift = false, unsigned targetSourceX = 0, unsigned nSource = 2, int pfType = 0, double alpha = 0.9, const String& nm = "SubbandMMI")
    : _fftLen(fftLen), _hbs(halfBandShift), _target(targetSourceX), _nSource(nSource), _pfType(pfType), _alpha(alpha), _nm(nm), _w(0), _mask(false), _avg(-1.0), _fwidth(1), _mtype(0) {}
  ~SubbandMMI() { if (_w) dsr_mmi_destroy(_w); }
  void setChannel(VectorComplexFeatureStreamPtr& chan) { _channelList.push_back(chan); }
  unsigned chanN() const { return (unsigned) _channelList.size(); }
  void useBinaryMask(double avgFactor = -1.0, unsigned fwidth = 1, unsigned type = 0) { _mask = true; _avg = avgFactor; _fwidth = fwidth; _mtype = type; if (_w) dsr_throw(dsr_mmi_use_binary_mask(_w, avgFactor, fwidth, type)); }
  void calcWeights(double sampleRate, const double* delays /*[nSource][chanN]*/) { dsr_throw(dsr_mmi_calc_weights(weights(), sampleRate, delays)); }
  void calcWeightsN(double sampleRate, const double* delays, unsigned NC = 2) { dsr_throw(dsr_mmi_calc_weights_n(weights(), sampleRate, delays, NC)); }
  void setActiveWeights_f(unsigned fbinX, const double* packedWeights, size_t rows, size_t cols, int option = 0) {
    if (!_w) throw j_error(JERROR, "call calcWeightsX() once");
    dsr_throw(dsr_mmi_set_active_weights_f(_w, fbinX, packedWeights, rows, cols, option));
  }
  void setHiActiveWeights_f(unsigned fbinX, const double* pkdWa, size_t nWa, const double* pkdwb, size_t nWb, int option = 0) {
    if (!_w) throw j_error(JERROR, "call calcWeightsX() once");
    dsr_throw(dsr_mmi_set_hi_active_weights_f(_w, fbinX, pkdWa, nWa, pkdwb, nWb, option));
  }
  virtual const std::complex<double>* next(int frameX = -5) {
    if (!_h) throw j_error(JERROR, "call calcWeightsX() once");
    return VectorComplexFeatureStream::next(frameX);
  }
 private:
  dsr_mmi* weights() {
    if (!_w) {
      dsr_throw(dsr_mmi_create((int) _fftLen, (int) chanN(), _hbs, (int) _target, (int) _nSource, _pfType, _alpha, &_w));
      if (_mask) dsr_throw(dsr_mmi_use_binary_mask(_w, _avg, _fwidth, _mtype));
      dsr_stream* h = 0; dsr_throw(dsr_subband_mmi_stream_create(_w, (int) _fftLen, _nm.c_str(), &h)); adopt(h);
      for (size_t i = 0; i < _channelList.size(); i++) dsr_throw(dsr_subband_bf_set_channel(_h, _channelList[i]->handle()));
    }
    return _w;
  }
  unsigned _fftLen; bool _hbs; unsigned _target, _nSource; int _pfType; double _alpha; String _nm; dsr_mmi* _w;
  bool _mask; double _avg; unsigned _fwidth, _mtype; std::vector<VectorComplexFeatureStreamPtr> _channelList;
};
// ---- btk/beamformer/tracker.h: ModalDecomposition / SpatialDecomposition (:181-211), Modal / SpatialSphericalArrayTracker (:301-330),
// PlaneWaveSimulator (:335-359).  A decomposition keeps its arguments and a handle for its tables; the tracker built on it makes its own handle
// with the filter's parameters.  setV takes the L x L complex block row major (L = subbandLengthN()).
class BaseDecomposition {
 public:
  BaseDecomposition(unsigned orderN, unsigned subbandsN, double a, double sampleRate, unsigned useSubbandsN = 0, bool spatial = false)
    : _orderN(orderN), _subbandsN(subbandsN), _useSubbandsN(useSubbandsN), _a(a), _sampleRate(sampleRate), _spatial(spatial), _t(0) {
    dsr_throw(dsr_trk_create(spatial ? DSR_TRK_SPATIAL : DSR_TRK_MODAL, (int) orderN, (int) subbandsN, a, sampleRate, 1, 10.0, 10.0, 10.0, 1, 32, &_t));   // the tables only: the tracker's handle checks the observation's length
  }
  virtual ~BaseDecomposition() { if (_t) dsr_trk_destroy(_t); }
  unsigned orderN() const { return _orderN; }
  unsigned modesN() const { return (unsigned) dsr_trk_modes_n(_t); }
  unsigned subbandsN() const { return _subbandsN; }
  unsigned subbandsN2() const { return _subbandsN / 2; }
  unsigned useSubbandsN() const { return _useSubbandsN ? _useSubbandsN : _subbandsN / 2 + 1; }
  unsigned subbandLengthN() const { return (unsigned) dsr_trk_subband_length(_t); }
  virtual void reset() {}
  static std::complex<double> harmonic(int order, int degree, double theta, double phi) { double o[2]; dsr_throw(dsr_trk_harmonic(order, degree, theta, phi, o)); return std::complex<double>(o[0], o[1]); }
  static std::complex<double> harmonicDerivPolarAngle(int order, int degree, double theta, double phi) { double o[2]; dsr_throw(dsr_trk_harmonic_deriv_polar(order, degree, theta, phi, o)); return std::complex<double>(o[0], o[1]); }
  static std::complex<double> harmonicDerivAzimuth(int order, int degree, double theta, double phi) { double o[2]; dsr_throw(dsr_trk_harmonic_deriv_azimuth(order, degree, theta, phi, o)); return std::complex<double>(o[0], o[1]); }
  static std::complex<double> modalCoefficient(unsigned order, double ka) { double o[2]; dsr_throw(dsr_trk_modal_coefficient(order, ka, o)); return std::complex<double>(o[0], o[1]); }
  const dsr_trk* handle() const { return _t; }
  bool spatial() const { return _spatial; }
  double a() const { return _a; }
  double sampleRate() const { return _sampleRate; }
  unsigned useSubbandsArg() const { return _useSubbandsN; }
 private:
  BaseDecomposition(const BaseDecomposition&); BaseDecomposition& operator=(const BaseDecomposition&);
  unsigned _orderN, _subbandsN, _useSubbandsN; double _a, _sampleRate; bool _spatial; dsr_trk* _t;
};
class ModalDecomposition : public BaseDecomposition {
 public: ModalDecomposition(unsigned orderN, unsigned subbandsN, double a, double sampleRate, unsigned useSubbandsN = 0) : BaseDecomposition(orderN, subbandsN, a, sampleRate, useSubbandsN, false) {}
};
class SpatialDecomposition : public BaseDecomposition {
 public: SpatialDecomposition(unsigned orderN, unsigned subbandsN, double a, double sampleRate, unsigned useSubbandsN = 0) : BaseDecomposition(orderN, subbandsN, a, sampleRate, useSubbandsN, true) {}
};
typedef std::shared_ptr<BaseDecomposition> BaseDecompositionPtr;
typedef std::shared_ptr<ModalDecomposition> ModalDecompositionPtr;
typedef std::shared_ptr<SpatialDecomposition> SpatialDecompositionPtr;
class BaseSphericalArrayTracker : public VectorFloatFeatureStream {
 public:
  BaseSphericalArrayTracker(const BaseDecomposition& d, double sigma2_u, double sigma2_v, double sigma2_init, unsigned maxLocalN, const String& nm) : _t(0) {
    dsr_throw(dsr_trk_create(d.spatial() ? DSR_TRK_SPATIAL : DSR_TRK_MODAL, (int) d.orderN(), (int) d.subbandsN(), d.a(), d.sampleRate(), (int) d.useSubbandsArg(), sigma2_u, sigma2_v,
                             sigma2_init, (int) maxLocalN, 32, &_t));
    DSR_OP(BaseSphericalArrayTracker, float, dsr_trk_stream_create(_t, nm.c_str(), &h))
  }
  ~BaseSphericalArrayTracker() { if (_t) dsr_trk_destroy(_t); }
  void setChannel(VectorComplexFeatureStreamPtr& chan) { dsr_throw(dsr_trk_stream_set_channel(_h, chan->handle())); _channelList.push_back(chan); }
  void setV(const std::complex<double>* Vk, unsigned subbandX) { const size_t L = (size_t) dsr_trk_subband_length(_t); dsr_throw(dsr_trk_set_v(_t, reinterpret_cast<const double*>(Vk), 2 * L * L, subbandX)); }
  unsigned chanN() const { return (unsigned) _channelList.size(); }
  void nextSpeaker() { dsr_throw(dsr_trk_stream_next_speaker(_h)); }
  void setInitialPosition(double theta, double phi) { dsr_throw(dsr_trk_stream_set_initial_position(_h, theta, phi)); }
 private:
  dsr_trk* _t; std::vector<VectorComplexFeatureStreamPtr> _channelList;
};
class ModalSphericalArrayTracker : public BaseSphericalArrayTracker {
 public: ModalSphericalArrayTracker(ModalDecompositionPtr& modalDecomposition, double sigma2_u = 10.0, double sigma2_v = 10.0, double sigma2_init = 10.0, unsigned maxLocalN = 1,
                                    const String& nm = "ModalSphericalArrayTracker") : BaseSphericalArrayTracker(*modalDecomposition, sigma2_u, sigma2_v, sigma2_init, maxLocalN, nm) {}
};
class SpatialSphericalArrayTracker : public BaseSphericalArrayTracker {
 public: SpatialSphericalArrayTracker(SpatialDecompositionPtr& spatialDecomposition, double sigma2_u = 10.0, double sigma2_v = 10.0, double sigma2_init = 10.0, unsigned maxLocalN = 1,
                                      const String& nm = "SpatialSphericalArrayTracker") : BaseSphericalArrayTracker(*spatialDecomposition, sigma2_u, sigma2_v, sigma2_init, maxLocalN, nm) {}
};
typedef std::shared_ptr<ModalSphericalArrayTracker> ModalSphericalArrayTrackerPtr;
typedef std::shared_ptr<SpatialSphericalArrayTracker> SpatialSphericalArrayTrackerPtr;
class PlaneWaveSimulator : public VectorComplexFeatureStream {
 public:
  PlaneWaveSimulator(const VectorComplexFeatureStreamPtr& source, ModalDecompositionPtr& modalDecomposition, unsigned channelX, double theta, double phi, const String& nm = "Plane Wave Simulator")
    : _s(source), _d(modalDecomposition) { DSR_OP(PlaneWaveSimulator, cplx, dsr_pws_stream_create(source->handle(), modalDecomposition->handle(), channelX, theta, phi, nm.c_str(), &h)) }
 private: VectorComplexFeatureStreamPtr _s; ModalDecompositionPtr _d;
};
typedef std::shared_ptr<PlaneWaveSimulator> PlaneWaveSimulatorPtr;
#undef DSR_OP

// ======================================================================================================================
// ASR side (asr/dictionary, asr/gaussian, asr/decoder): the classes decoder.i:52-199 and gaussian.i:281-283,465-467 wrap, with
// their constructor argument order, over include/dsr.h sections 4, 5, 8 and 8b.
// ======================================================================================================================
#include <fstream>
#include <map>
#include <sstream>

// ---- btk/feature/feature.h:1486-1501
class FeatureSet {
 public:
  explicit FeatureSet(const String& nm = "FeatureSet") : _name(nm) {}
  const String& name() const { return _name; }
  void add(VectorFloatFeatureStreamPtr& feat) { _list[feat->name()] = feat; }
  VectorFloatFeatureStreamPtr& feature(const String& nm) {
    std::map<String, VectorFloatFeatureStreamPtr>::iterator it = _list.find(nm);
    if (it == _list.end()) throw jkey_error("Could not find key " + nm + " in list " + _name);          // List::operator[] (mlist.h:109-114)
    return it->second;
  }
 private:
  String _name; std::map<String, VectorFloatFeatureStreamPtr> _list;
};
typedef std::shared_ptr<FeatureSet> FeatureSetPtr;

// ---- asr/dictionary/distribTree.h:40-65
class Lexicon {
 public:
  explicit Lexicon(const String& nm, const String& fileName = "") : _h(0) { dsr_throw(dsr_lexicon_create(nm.c_str(), fileName.c_str(), &_h)); }
  ~Lexicon() { dsr_lexicon_destroy(_h); }
  void clear() { dsr_throw(dsr_lexicon_clear(_h)); }
  String name() const { return dsr_lexicon_name(_h); }
  unsigned size() const { return (unsigned) dsr_lexicon_size(_h); }
  void read(const String& fileName) { dsr_throw(dsr_lexicon_read(_h, fileName.c_str())); }
  void write(const String& fileName, bool writeHeader = false) const { dsr_throw(dsr_lexicon_write(_h, fileName.c_str(), writeHeader)); }
  unsigned index(const String& symbol, bool create = false) { unsigned i = 0; dsr_throw(dsr_lexicon_index(_h, symbol.c_str(), create, &i)); return i; }
  String symbol(unsigned idx) const { const char* p = 0; dsr_throw(dsr_lexicon_symbol(_h, idx, &p)); return p; }
  bool isPresent(const String& symbol) const { return dsr_lexicon_is_present(_h, symbol.c_str()) != 0; }
  dsr_lexicon* handle() const { return _h; }
 private:
  Lexicon(const Lexicon&); Lexicon& operator=(const Lexicon&);
  dsr_lexicon* _h;
};
typedef std::shared_ptr<Lexicon> LexiconPtr;

// ---- asr/gaussian: CodebookSetBasic(descFile, fs, cbkFile) (gaussian.i:281-283; description lines "name featureName refN dimN covType",
// ';' comments, codebookBasic.cc:804-828) and DistribSetBasic(cbs, descFile, distFile) (gaussian.i:465-467; lines "name codebookName",
// distribBasic.cc:218-232).  The big-endian set files are read by dsr_gmm_load.
inline std::vector<std::vector<String> > dsr_desc_rows(const String& path)
{
  std::vector<std::vector<String> > rows; if (path.empty()) return rows;
  std::ifstream f(path.c_str()); if (!f) throw jio_error("Could not open file " + path);
  String line;
  while (std::getline(f, line)) { if (!line.empty() && line[0] == ';') continue; std::istringstream is(line); std::vector<String> t; String w; while (is >> w) t.push_back(w); if (!t.empty()) rows.push_back(t); }
  return rows;
}
class CodebookSetBasic {
 public:
  CodebookSetBasic(const String& descFile = "", FeatureSetPtr fs = FeatureSetPtr(), const String& cbkFile = "") : _fs(fs), _cbkFile(cbkFile), _desc(dsr_desc_rows(descFile)) {}
  unsigned ncbks() const { return (unsigned) _desc.size(); }
  const String& cbkFile() const { return _cbkFile; }
  VectorFloatFeatureStreamPtr& feature() {
    if (_desc.empty() || _desc[0].size() < 2 || !_fs) throw jconsistency_error("the codebook description names no feature");
    return _fs->feature(_desc[0][1]);
  }
 private:
  FeatureSetPtr _fs; String _cbkFile; std::vector<std::vector<String> > _desc;
};
typedef std::shared_ptr<CodebookSetBasic> CodebookSetBasicPtr;

class DistribSetBasic;
class DistribBasic {                                          // Distrib::score(frameX), name() (distribBasic.h:40-60)
 public:
  DistribBasic(dsr_distribset* ds, int x) : _ds(ds), _x(x) {}
  float score(int frameX) { float s = 0.f; dsr_throw(dsr_distribset_score(_ds, _x, frameX, &s)); return s; }
  String name() const { return dsr_distribset_name(_ds, _x); }
 private:
  dsr_distribset* _ds; int _x;
};
class DistribSetBasic {
 public:
  DistribSetBasic(CodebookSetBasicPtr& cbs, const String& descFile = "", const String& distFile = "") : _cbs(cbs), _gmm(0), _ds(0) {
    const std::vector<std::vector<String> > d = dsr_desc_rows(descFile);
    dsr_throw(dsr_gmm_load(cbs->cbkFile().c_str(), distFile.c_str(), &_gmm));
    if (!d.empty() && (int) d.size() != dsr_gmm_num_dists(_gmm)) { dsr_gmm_destroy(_gmm); throw jconsistency_error("the description and the file hold different numbers of distributions"); }
    _feat = cbs->feature();
    const dsr_status s = dsr_distribset_create(_gmm, _feat->handle(), 0, &_ds);
    if (s != DSR_OK) { dsr_gmm_destroy(_gmm); dsr_throw(s); }
  }
  ~DistribSetBasic() { dsr_distribset_destroy(_ds); dsr_gmm_destroy(_gmm); }
  unsigned ndists() const { return (unsigned) dsr_distribset_ndists(_ds); }
  unsigned index(const String& key) const { int x = 0; dsr_throw(dsr_distribset_find(_ds, key.c_str(), &x)); return (unsigned) x; }
  DistribBasic find(const String& key) { return DistribBasic(_ds, (int) index(key)); }
  DistribBasic find(unsigned dsX) { if (dsX >= ndists()) throw jindex_error("distribution index out of range"); return DistribBasic(_ds, (int) dsX); }
  void resetCache() { dsr_throw(dsr_distribset_reset_cache(_ds)); }
  void resetFeature() { dsr_throw(dsr_distribset_reset_feature(_ds)); }
  dsr_distribset* handle() const { return _ds; }
  dsr_gmm* gmm() const { return _gmm; }
  VectorFloatFeatureStreamPtr& featureStream() { return _feat; }
 protected:
  explicit DistribSetBasic(dsr_distribset* ds) : _gmm(0), _ds(ds) {}                              // a set that is no model of its own (multi-stream)
 private:
  DistribSetBasic(const DistribSetBasic&); DistribSetBasic& operator=(const DistribSetBasic&);
  CodebookSetBasicPtr _cbs; VectorFloatFeatureStreamPtr _feat; dsr_gmm* _gmm; dsr_distribset* _ds;
};
typedef std::shared_ptr<DistribSetBasic> DistribSetBasicPtr;
typedef DistribSetBasicPtr DistribSetPtr;

// ---- multi-stream decoding (include/dsr.h section 8b): DistribMap (distribBasic.h:390-408), DistribMultiStream (:135-158) and
// DistribSetMultiStream(audioDistSet, videoDistSet[, distribMap], audioWeight, videoWeight) (distribBasic.cc:381-410).  A DistribSetMultiStreamPtr
// converts to DistribSetPtr, so it is what DecoderFlyWeight and Lattice::gammaProbsDist take.
class DistribMap {
 public:
  DistribMap() : _h(0) { dsr_throw(dsr_distribmap_create(&_h)); }
  ~DistribMap() { dsr_distribmap_destroy(_h); }
  void add(const String& fromName, const String& toName) { dsr_throw(dsr_distribmap_add(_h, fromName.c_str(), toName.c_str())); }
  String mapped(const String& name) const { const char* to = 0; dsr_throw(dsr_distribmap_mapped(_h, name.c_str(), &to)); return to; }
  unsigned size() const { return (unsigned) dsr_distribmap_size(_h); }
  void read(const String& fileName) { dsr_throw(dsr_distribmap_read(_h, fileName.c_str())); }
  void write(const String& fileName) const { dsr_throw(dsr_distribmap_write(_h, fileName.c_str())); }
  dsr_distribmap* handle() const { return _h; }
 private:
  DistribMap(const DistribMap&); DistribMap& operator=(const DistribMap&);
  dsr_distribmap* _h;
};
typedef std::shared_ptr<DistribMap> DistribMapPtr;

class DistribMultiStream : public DistribBasic {
 public:
  DistribMultiStream(dsr_distribset* ds, int x) : DistribBasic(ds, x), _set(ds) {}
  double audioWeight() const { double a = 0.0, v = 0.0; dsr_throw(dsr_distribset_get_weights(_set, &a, &v)); return a; }
  double videoWeight() const { double a = 0.0, v = 0.0; dsr_throw(dsr_distribset_get_weights(_set, &a, &v)); return v; }
 private:
  dsr_distribset* _set;
};
class DistribSetMultiStream : public DistribSetBasic {
 public:
  DistribSetMultiStream(DistribSetBasicPtr& audioDistSet, DistribSetBasicPtr& videoDistSet, double audioWeight = 0.95, double videoWeight = 0.05)
    : DistribSetBasic(make(audioDistSet, videoDistSet, 0, audioWeight, videoWeight)), _audio(audioDistSet), _video(videoDistSet) {}
  DistribSetMultiStream(DistribSetBasicPtr& audioDistSet, DistribSetBasicPtr& videoDistSet, DistribMapPtr& distribMap, double audioWeight = 0.95, double videoWeight = 0.05)
    : DistribSetBasic(make(audioDistSet, videoDistSet, distribMap ? distribMap->handle() : 0, audioWeight, videoWeight)), _audio(audioDistSet), _video(videoDistSet) {}
  DistribMultiStream find(const String& key) { return DistribMultiStream(handle(), (int) index(key)); }
  DistribMultiStream find(unsigned dsX) { if (dsX >= ndists()) throw jindex_error("distribution index out of range"); return DistribMultiStream(handle(), (int) dsX); }
  void setWeights(double audioWeight, double videoWeight) { dsr_throw(dsr_distribset_set_weights(handle(), audioWeight, videoWeight)); }
 private:
  static dsr_distribset* make(DistribSetBasicPtr& a, DistribSetBasicPtr& v, const dsr_distribmap* m, double wA, double wV) {
    if (!a || !v) throw jparameter_error("null argument");
    dsr_distribset* ds = 0; dsr_throw(dsr_distribset_create_multistream(a->handle(), v->handle(), m, wA, wV, &ds)); return ds;
  }
  DistribSetBasicPtr _audio, _video;
};
class DistribSetMultiStreamPtr : public std::shared_ptr<DistribSetMultiStream> {
 public:
  DistribSetMultiStreamPtr() {}
  explicit DistribSetMultiStreamPtr(DistribSetMultiStream* p) : std::shared_ptr<DistribSetMultiStream>(p), _base(*this) {}
  operator DistribSetPtr&() { return _base; }                                                     // the first argument of DecoderFlyWeight
 private:
  DistribSetPtr _base;
};

// ---- asr/decoder: WFSTFlyWeight(statelex, inlex, outlex, name) (decoder.i:52-70)
class WFSTFlyWeight {
 public:
  WFSTFlyWeight(LexiconPtr& statelex, LexiconPtr& inlex, LexiconPtr& outlex, const String& name = "WFSTFlyWeight")
    : _stateLexicon(statelex), _inputLexicon(inlex), _outputLexicon(outlex), _name(name), _h(0) {
    dsr_throw(dsr_wfst_create(&_h));
    dsr_throw(dsr_wfst_set_lexicons(_h, statelex ? statelex->handle() : 0, inlex ? inlex->handle() : 0, outlex ? outlex->handle() : 0));
  }
  ~WFSTFlyWeight() { dsr_wfst_destroy(_h); }
  void read(const String& fileName, bool binary = false) { dsr_throw(dsr_wfst_read(_h, fileName.c_str(), binary)); }
  void write(const String& fileName, bool binary = true, bool useSymbols = false) { dsr_throw(dsr_wfst_write_symbols(_h, fileName.c_str(), binary, useSymbols)); }
  void reverse(const std::shared_ptr<WFSTFlyWeight>& wfst) { dsr_throw(dsr_wfst_reverse(_h, wfst->handle())); }      // wfstFlyWeight.cc:141-213
  void reverseRead(const String& fileName) { dsr_throw(dsr_wfst_reverse_read(_h, fileName.c_str())); }                // :215-297
  bool hasFinalState() const { return dsr_wfst_has_final_state(_h) != 0; }
  LexiconPtr& stateLexicon() { return _stateLexicon; }
  LexiconPtr& inputLexicon() { return _inputLexicon; }
  LexiconPtr& outputLexicon() { return _outputLexicon; }
  dsr_wfst* handle() const { return _h; }
 private:
  WFSTFlyWeight(const WFSTFlyWeight&); WFSTFlyWeight& operator=(const WFSTFlyWeight&);
  LexiconPtr _stateLexicon, _inputLexicon, _outputLexicon; String _name; dsr_wfst* _h;
};
typedef std::shared_ptr<WFSTFlyWeight> WFSTFlyWeightPtr;
// asr/decoder/wfstFlyWeight.h:403-424: every node keeps its arcs ordered by (output, input); what DecoderWordTrace::set takes
class WFSTFlyWeightSortedOutput : public WFSTFlyWeight {
 public:
  WFSTFlyWeightSortedOutput(LexiconPtr& statelex, LexiconPtr& inlex, LexiconPtr& outlex, const String& name = "WFSTFlyWeight")
    : WFSTFlyWeight(statelex, inlex, outlex, name) { dsr_throw(dsr_wfst_set_sorted_output(handle(), 1)); }
};
typedef std::shared_ptr<WFSTFlyWeightSortedOutput> WFSTFlyWeightSortedOutputPtr;

typedef std::vector<String> DistribPath;                       // asr/path/distribPath.h:34-60: the distribution names along a path
// asr/lattice Lattice(statelex, inlex, outlex) (lattice.i:79-135, lattice.h:188-330): what _Decoder::lattice() returns, or an object to read() into
class Lattice {
 public:
  Lattice(LexiconPtr statelex, LexiconPtr inlex, LexiconPtr outlex) : _stateLexicon(statelex), _inputLexicon(inlex), _outputLexicon(outlex), _h(0) {}
  Lattice(dsr_lattice* h, LexiconPtr inlex, LexiconPtr outlex) : _inputLexicon(inlex), _outputLexicon(outlex), _h(h) {}
  explicit Lattice(dsr_lattice* h) : _h(h) {}
  ~Lattice() { if (_h) dsr_lattice_destroy(_h); }
  void read(const String& fileName, bool noSelfLoops = false, bool readData = false) {
    dsr_lattice* n = 0;
    dsr_throw(dsr_lattice_read(fileName.c_str(), noSelfLoops, readData, _inputLexicon ? _inputLexicon->handle() : 0, _outputLexicon ? _outputLexicon->handle() : 0, &n));
    if (_h) dsr_lattice_destroy(_h);
    _h = n;
  }
  void write(const String& fileName = "", bool useSymbols = false, bool writeData = false) {
    if (useSymbols) throw jparameter_error("useSymbols: write the numeric form and map the symbols with the lexica");
    dsr_throw(dsr_lattice_write(need(), fileName.c_str(), writeData));
  }
  float rescore(double lmScale = 30.0, double lmPenalty = 0.0, double silPenalty = 0.0, const String& silSymbol = "SIL-m") {
    float s = 0.0f; dsr_throw(dsr_lattice_rescore(need(), lmScale, lmPenalty, silPenalty, silX(silSymbol), &s)); return s;
  }
  String bestHypo(bool useInputSymbols = false) {
    int n = 0; dsr_throw(dsr_lattice_best_hypo(need(), useInputSymbols, 0, 0, &n));
    std::vector<uint32_t> ids((size_t) (n > 0 ? n : 1)); dsr_throw(dsr_lattice_best_hypo(_h, useInputSymbols, ids.data(), (int) ids.size(), &n));
    LexiconPtr& lex = useInputSymbols ? _inputLexicon : _outputLexicon;
    if (!lex) throw jkey_error("no lexicon to name the symbols with");
    String hypo; for (int i = 0; i < n; i++) hypo += lex->symbol(ids[(size_t) i]) + " ";           // "symbol " per link, as lattice.cc:292,298 build it
    return hypo;
  }
  double gammaProbs(double acScale = 1.0, double lmScale = 12.0, double lmPenalty = 0.0, double silPenalty = 0.0, const String& silSymbol = "SIL-m") {
    double p = 0.0; dsr_throw(dsr_lattice_gamma_probs(need(), acScale, lmScale, lmPenalty, silPenalty, silX(silSymbol), &p)); return p;
  }
  double gammaProbsDist(DistribSetBasicPtr& dss, double acScale = 1.0, double lmScale = 12.0, double lmPenalty = 0.0, double silPenalty = 0.0, const String& silSymbol = "SIL-m") {
    double p = 0.0; dsr_throw(dsr_lattice_gamma_probs_dist(need(), dss->handle(), acScale, lmScale, lmPenalty, silPenalty, silX(silSymbol), &p)); return p;
  }
  void prune(double threshold = 100.0) { dsr_throw(dsr_lattice_prune(need(), threshold)); }
  void pruneEdges(unsigned edgesN = 0) { dsr_throw(dsr_lattice_prune_edges(need(), edgesN)); }
  void purge() { dsr_throw(dsr_lattice_purge(need())); }
  void writeCTM(const String& conv, const String& channel, const String& spk, const String& utt, double cfrom, double score, const String& fileName = "",
                double frameInterval = 0.01, const String& endMarker = "</s>") {
    dsr_throw(dsr_lattice_write_ctm(need(), lexh(_outputLexicon), conv.c_str(), channel.c_str(), spk.c_str(), utt.c_str(), cfrom, score, fileName.c_str(), frameInterval, endMarker.c_str()));
  }
  void writePhoneCTM(const String& conv, const String& channel, const String& spk, const String& utt, double cfrom, double score, const String& fileName = "",
                     double frameInterval = 0.01, const String& endMarker = "</s>") {
    dsr_throw(dsr_lattice_write_phone_ctm(need(), lexh(_inputLexicon), conv.c_str(), channel.c_str(), spk.c_str(), utt.c_str(), cfrom, score, fileName.c_str(), frameInterval, endMarker.c_str()));
  }
  void writeHypoHTK(const String& conv, const String& channel, const String& spk, const String& utt, double cfrom, double score, const String& fileName = "",
                    int flag = 0, double frameInterval = 0.01, const String& endMarker = "</s>") {
    dsr_throw(dsr_lattice_write_hypo_htk(need(), lexh(_outputLexicon), conv.c_str(), channel.c_str(), spk.c_str(), utt.c_str(), cfrom, score, fileName.c_str(), flag, frameInterval, endMarker.c_str()));
  }
  void writeWordConfs(const String& fileName, const String& uttId, const String& endMarker = "</s>") {
    dsr_throw(dsr_lattice_write_word_confs(need(), lexh(_outputLexicon), fileName.c_str(), uttId.c_str(), endMarker.c_str()));
  }
  unsigned nodesN() const { return _h ? (unsigned) dsr_lattice_num_nodes(_h) : 0u; }
  unsigned edgesN() const { return _h ? (unsigned) dsr_lattice_num_edges(_h) : 0u; }
  LexiconPtr& stateLexicon() { return _stateLexicon; }
  LexiconPtr& inputLexicon() { return _inputLexicon; }
  LexiconPtr& outputLexicon() { return _outputLexicon; }
  dsr_lattice* handle() const { return _h; }
 private:
  Lattice(const Lattice&); Lattice& operator=(const Lattice&);
  dsr_lattice* need() const { if (!_h) throw jconsistency_error("empty lattice: decode or read one first"); return _h; }
  static dsr_lexicon* lexh(const LexiconPtr& l) { if (!l) throw jkey_error("no lexicon to name the symbols with"); return l->handle(); }
  unsigned silX(const String& silSymbol) { if (!_inputLexicon) throw jkey_error("no input lexicon to look " + silSymbol + " up in"); return _inputLexicon->index(silSymbol); }
  LexiconPtr _stateLexicon, _inputLexicon, _outputLexicon; dsr_lattice* _h;
};
typedef std::shared_ptr<Lattice> LatticePtr;

// DecoderFlyWeight(dist, beam, lmScale, lmPenalty, silPenalty, silSymbol, eosSymbol, heapSize, topN, generateLattice) (decoder.i:147-199).
// heapSize sizes the reference's token hash (decoder.h:48-76) and has no counterpart here.
class DecoderFlyWeight {
 public:
  DecoderFlyWeight(DistribSetPtr& dist, double beam = 100.0, double lmScale = 12.0, double lmPenalty = 0.0, double silPenalty = 0.0,
                   const String& silSymbol = "SIL-m", const String& eosSymbol = "</s>", unsigned heapSize = 5000, unsigned topN = 0, bool generateLattice = true)
    : _dist(dist), _sil(silSymbol), _eos(eosSymbol), _h(0), _score(0.0) {
    (void) heapSize;
    dsr_decoder_cfg c; dsr_decoder_default_cfg(&c);
    c.beam = beam; c.lmScale = lmScale; c.lmPenalty = lmPenalty; c.silPenalty = silPenalty; c.topN = (int) topN; c.streams = 1;
    c.latticeTokens = generateLattice ? ((int64_t) 1 << 22) : 0;
    dsr_throw(dsr_decoder_create(&c, &_h));
  }
  ~DecoderFlyWeight() { dsr_decoder_destroy(_h); }
  void set(WFSTFlyWeightPtr& wfst) { dsr_throw(dsr_decoder_set_symbols(_h, wfst->handle(), _sil.c_str(), _eos.c_str())); _wfst = wfst; }
  double decode(bool verbose = false) {
    (void) verbose;
    dsr_decode_result r; std::vector<int32_t> arcs((size_t) 1 << 16); std::vector<uint32_t> words((size_t) 1 << 16);
    dsr_throw(dsr_decoder_decode_stream(_h, _dist->handle(), &r, arcs.data(), words.data(), (int) arcs.size()));
    _score = r.score; return _score;
  }
  String bestHypo(bool useInputSymbols = false) {
    size_t need = 0; dsr_throw(dsr_decoder_best_hypo(_h, 0, useInputSymbols, 0, 0, &need));
    std::vector<char> b(need); dsr_throw(dsr_decoder_best_hypo(_h, 0, useInputSymbols, b.data(), b.size(), &need)); return String(b.data());
  }
  DistribPath bestPath() {
    size_t need = 0; int n = 0; dsr_throw(dsr_decoder_best_path(_h, 0, 0, 0, &need, &n));
    std::vector<char> b(need); dsr_throw(dsr_decoder_best_path(_h, 0, b.data(), b.size(), &need, &n));
    DistribPath p; std::istringstream is(String(b.data())); String w; while (std::getline(is, w)) p.push_back(w); return p;
  }
  unsigned finalStatesN() const { int n = 0; dsr_throw(dsr_decoder_final_states_n(_h, 0, &n)); return (unsigned) n; }
  bool traceBackSucceeded() const { int ok = 0; dsr_throw(dsr_decoder_trace_back_succeeded(_h, 0, &ok)); return ok != 0; }
  LatticePtr lattice() {
    dsr_lattice* l = 0; dsr_throw(dsr_decoder_lattice(_h, 0, dsr_decoder_eos_index(_h), &l));
    return LatticePtr(_wfst ? new Lattice(l, _wfst->inputLexicon(), _wfst->outputLexicon()) : new Lattice(l));
  }
  void writeGMM(const String& conv, const String& channel, const String& spk, const String& utt, double cfrom, double score, const String& fileName = "", double frameInterval = 0.01) {
    dsr_throw(dsr_decoder_write_gmm(_h, 0, conv.c_str(), channel.c_str(), spk.c_str(), utt.c_str(), cfrom, score, fileName.c_str(), frameInterval));
  }
  // decoder.h:398-401: the base template constructs a j_error and does not throw it -- a silent no-op in the shipped code, and here
  void writeCTM(const String&, const String&, const String&, const String&, double, double, const String& = "", double = 0.01) {}
  void setTokenMemoryLimit(unsigned limit) { dsr_throw(dsr_decoder_set_token_memory_limit(_h, limit)); }           // decoder.h:396
  void setBeam(double beam) { dsr_throw(dsr_decoder_set_beam(_h, beam)); }
  dsr_decoder* handle() const { return _h; }
 private:
  DecoderFlyWeight(const DecoderFlyWeight&); DecoderFlyWeight& operator=(const DecoderFlyWeight&);
  DistribSetPtr _dist; WFSTFlyWeightPtr _wfst; String _sil, _eos; dsr_decoder* _h; double _score;
};
typedef std::shared_ptr<DecoderFlyWeight> DecoderFlyWeightPtr;

// asr/decoder/decoder.h:1146-1304 (constructor :1227-1232).  generateLattice defaults to true as in the reference; that search reads the word trace of tokens
// that have none (decoder.cc:239) and is not built: decode() then throws jconsistency_error.  With generateLattice = false the 1-best search runs on the device.
class DecoderWordTrace {
 public:
  DecoderWordTrace(DistribSetPtr& dist, double beam = 100.0, double lmScale = 12.0, double lmPenalty = 0.0, double silPenalty = 0.0, const String& silSymbol = "SIL-m",
                   const String& eosSymbol = "</s>", unsigned heapSize = 5000, unsigned topN = 0, double epsilon = 0.0, unsigned validEndN = 30,
                   bool generateLattice = true, unsigned propagateN = 5, bool fastHash = false, bool insertSilence = false)
    : _dist(dist), _sil(silSymbol), _eos(eosSymbol), _h(0) {
    (void) heapSize; (void) topN; (void) validEndN;
    if (epsilon != 0.0) throw j_error(JPARAMETER, "DecoderWordTrace: epsilon > 0 (early stop, decoder.cc:172-182) is not built");
    dsr_decoder_cfg c; dsr_decoder_default_cfg(&c);
    c.beam = beam; c.lmScale = lmScale; c.lmPenalty = lmPenalty; c.silPenalty = silPenalty; c.streams = 1;
    c.wordTrace = 1; c.wordTraceLattice = generateLattice; c.propagateN = (int) propagateN; c.fastHash = fastHash; c.insertSilence = insertSilence;
    dsr_throw(dsr_decoder_create(&c, &_h));
  }
  ~DecoderWordTrace() { dsr_decoder_destroy(_h); }
  void set(WFSTFlyWeightSortedOutputPtr& wfst) { dsr_throw(dsr_decoder_set_symbols(_h, wfst->handle(), _sil.c_str(), _eos.c_str())); _wfst = wfst; }
  double decode(bool verbose = false) {
    (void) verbose;
    dsr_decode_result r; std::vector<int32_t> arcs(16); _words.assign((size_t) 1 << 16, 0u);
    dsr_throw(dsr_decoder_decode_stream(_h, _dist->handle(), &r, arcs.data(), _words.data(), (int) _words.size()));
    _words.resize((size_t) r.nWords); return r.score;
  }
  String bestHypo(bool useInputSymbols = false) {                       // (the shipped class's tokens have no prev(): one symbol)
    size_t need = 0; dsr_throw(dsr_decoder_best_hypo(_h, 0, useInputSymbols, 0, 0, &need));
    std::vector<char> b(need); dsr_throw(dsr_decoder_best_hypo(_h, 0, useInputSymbols, b.data(), b.size(), &need)); return String(b.data());
  }
  const std::vector<uint32_t>& wordTrace() const { return _words; }     // the words along the best token's word traces
  unsigned finalStatesN() const { int n = 0; dsr_throw(dsr_decoder_final_states_n(_h, 0, &n)); return (unsigned) n; }
  bool traceBackSucceeded() const { int ok = 0; dsr_throw(dsr_decoder_trace_back_succeeded(_h, 0, &ok)); return ok != 0; }
  void setBeam(double beam) { dsr_throw(dsr_decoder_set_beam(_h, beam)); }
 private:
  DecoderWordTrace(const DecoderWordTrace&); DecoderWordTrace& operator=(const DecoderWordTrace&);
  DistribSetPtr _dist; WFSTFlyWeightSortedOutputPtr _wfst; String _sil, _eos; dsr_decoder* _h; std::vector<uint32_t> _words;
};
typedef std::shared_ptr<DecoderWordTrace> DecoderWordTracePtr;

#include <cstdio>
// ---- asr/train: CodebookSetTrain(descFile, fs, cbkFile, massThreshold) (codebookTrain.cc:586-599), DistribSetTrain(cbs, descFile, distFile)
// (distribTrain.cc:424-437) over dsr_train_* (include/dsr.h section 9) for 1:1 diagonal models.  The two sets share one training handle, which
// the distribution set creates (it owns the model); the codebook set's methods need that to have happened.  Frames are pulled through the
// stream protocol (frames 0..T-1 of the feature the codebook set names) and run as one batch on the device.
// ---- asr/adapt: ParamTree (transform.h:520-552) and CodebookSetAdapt (codebookAdapt.h) over dsr_param_tree_* / dsr_mllr_* (include/dsr.h
// section 10).  MLLR parameters; the all-pass parameters have a tree of their own below.  A codebook set is bound to its model when its distribution set is built (the distribution set owns it).
class ParamTree {
 public:
  ParamTree(const String& fileName = "") : _h(0) { dsr_throw(dsr_param_tree_create(fileName.c_str(), &_h)); }
  ~ParamTree() { dsr_param_tree_destroy(_h); }
  void write(const String& fileName) const { dsr_throw(dsr_param_tree_write(_h, fileName.c_str())); }
  void read(const String& fileName) { dsr_throw(dsr_param_tree_read(_h, fileName.c_str())); }
  void clear() { dsr_throw(dsr_param_tree_clear(_h)); }
  int type() const { return dsr_param_tree_type(_h); }
  bool hasIndex(unsigned index) const { return dsr_param_tree_has_index(_h, index) != 0; }
  // find / findMLLR (transform.cc:835-860, 898-925): W [size][size + 1], the last column the bias
  std::vector<double> find(unsigned rc, bool useAncestor = true) { return get(rc, useAncestor, 0); }
  std::vector<double> findMLLR(unsigned rc, bool useAncestor = true) { return get(rc, useAncestor, 1); }
  dsr_param_tree* handle() const { return _h; }
 private:
  ParamTree(const ParamTree&); ParamTree& operator=(const ParamTree&);
  std::vector<double> get(unsigned rc, bool useAncestor, int mllr) {
    int n = 0; dsr_throw(dsr_param_tree_find(_h, rc, useAncestor, mllr, &n));
    std::vector<double> W((size_t) n * (n + 1) + 1); dsr_throw(dsr_param_tree_get(_h, rc, W.data())); W.resize((size_t) n * (n + 1)); return W;
  }
  dsr_param_tree* _h;
};
typedef std::shared_ptr<ParamTree> ParamTreePtr;

// ---- asr/adapt, the all-pass transforms over dsr_apt_* (include/dsr.h section 13): the ParamTree of RAPTParam or SLAPTParam blocks, the
// blocks themselves, and BLTTransformer / SLAPTTransformer (transform.h:350-404, transform.cc:1366-1430, 1636-1741).  RAPT with more than one
// parameter is refused by the library.  type: 1 RAPT, 2 SLAPT.
enum { APT_RAPT = 1, APT_SLAPT = 2 };
class APTParamTree {
 public:
  APTParamTree(const String& fileName = "") : _h(0) { dsr_throw(dsr_apt_params_create(fileName.c_str(), &_h)); }
  ~APTParamTree() { dsr_apt_params_destroy(_h); }
  void write(const String& fileName) const { dsr_throw(dsr_apt_params_write(_h, fileName.c_str())); }
  void read(const String& fileName) { dsr_throw(dsr_apt_params_read(_h, fileName.c_str())); }
  void clear() { dsr_throw(dsr_apt_params_clear(_h)); }
  int type() const { return dsr_apt_params_type(_h); }
  // findAPT (transform.cc:862-896): _conf and the bias of the class, a copy of its nearest ancestor when missing
  void findAPT(unsigned rc, int typ, std::vector<double>& conf, std::vector<float>& bias, bool useAncestor = true) {
    int nc = 0, nb = 0; dsr_throw(dsr_apt_params_find(_h, rc, typ, useAncestor, &nc, &nb));
    conf.assign((size_t) nc + 1, 0.0); bias.assign((size_t) nb + 1, 0.0f); dsr_throw(dsr_apt_params_get(_h, rc, conf.data(), bias.data()));
    conf.resize((size_t) nc); bias.resize((size_t) nb);
  }
  void set(unsigned rc, int typ, const std::vector<double>& conf, const std::vector<float>& bias = std::vector<float>()) {
    dsr_throw(dsr_apt_params_set(_h, rc, typ, (int) conf.size(), conf.data(), (int) bias.size(), bias.data()));
  }
  dsr_apt_params* handle() const { return _h; }
 private:
  APTParamTree(const APTParamTree&); APTParamTree& operator=(const APTParamTree&);
  dsr_apt_params* _h;
};
typedef std::shared_ptr<APTParamTree> APTParamTreePtr;

class APTParamBase {                                          // transform.h:307-346
 public:
  APTParamBase(int typ, const std::vector<double>& conf, const std::vector<float>& bias, unsigned rc) : _type(typ), _conf(conf), _bias(bias), _rc(rc) {}
  unsigned size() const { return (unsigned) _conf.size(); }
  double operator[](unsigned i) const { return _conf[i]; }
  unsigned regClass() const { return _rc; }
  const std::vector<double>& conf() const { return _conf; }
  const std::vector<float>& bias() const { return _bias; }
  int type() const { return _type; }
  void write(const String& fileName) const { APTParamTree t; t.set(_rc ? _rc : 1, _type, _conf, _bias); t.write(fileName); }
 private:
  int _type; std::vector<double> _conf; std::vector<float> _bias; unsigned _rc;
};
class RAPTParam : public APTParamBase {
 public:
  RAPTParam(double alpha, const std::vector<float>& bias = std::vector<float>(), unsigned rc = 0) : APTParamBase(APT_RAPT, std::vector<double>(1, alpha), bias, rc) {}
};
class SLAPTParam : public APTParamBase {
 public:
  SLAPTParam(const std::vector<double>& seq, const std::vector<float>& bias = std::vector<float>(), unsigned rc = 0) : APTParamBase(APT_SLAPT, seq, bias, rc) {}
};

class APTTransformerBase {                                    // the matrix and transform(from, to) of one block, both made on the device
 public:
  APTTransformerBase(const APTParamBase& par, unsigned sbFtSz, unsigned nSubFt) : _par(par), _L((int) sbFtSz), _nSub((int) nSubFt) { matrix(); }
  std::vector<double> matrix() const {                        // _calcTransMatrix (transform.cc:1212-1242): [sbFtSz][sbFtSz]
    std::vector<double> A((size_t) _L * _L + 1);
    dsr_throw(dsr_apt_transform_rows(_par.type(), _L, _nSub, (int) _par.size(), _par.conf().data(), 0, 0, 0, 0, A.data(), 0)); A.resize((size_t) _L * _L); return A;
  }
  std::vector<float> transform(const std::vector<float>& from, bool useBias = true) const {      // transform.cc:1295-1337, one mean
    std::vector<float> to(from.size());
    dsr_throw(dsr_apt_transform_rows(_par.type(), _L, _nSub, (int) _par.size(), _par.conf().data(), useBias ? (int) _par.bias().size() : 0,
                                     _par.bias().data(), from.data(), 1, 0, to.data()));
    return to;
  }
 private:
  APTParamBase _par; int _L, _nSub;
};
class BLTTransformer : public APTTransformerBase {
 public:
  BLTTransformer(const RAPTParam& par, unsigned sbFtSz, unsigned nSubFt = 1) : APTTransformerBase(par, sbFtSz, nSubFt) {}
};
class SLAPTTransformer : public APTTransformerBase {
 public:
  SLAPTTransformer(const SLAPTParam& par, unsigned sbFtSz, unsigned nSubFt = 1) : APTTransformerBase(par, sbFtSz, nSubFt) {}
};

class CodebookSetAdapt : public CodebookSetBasic {
 public:
  CodebookSetAdapt(const String& descFile = "", FeatureSetPtr fs = FeatureSetPtr(), const String& cbkFile = "")
    : CodebookSetBasic(descFile, fs, cbkFile), _g(0), _m(0), _subLen(0), _nSub(1) {}
  ~CodebookSetAdapt() { dsr_mllr_destroy(_m); for (std::map<int, dsr_apt*>::iterator it = _apt.begin(); it != _apt.end(); ++it) dsr_apt_destroy(it->second); }
  void setRegClasses(unsigned c = 1) {
    if (_m || !_apt.empty()) throw jconsistency_error("regression classes are set before the first estimation or transform");
    dsr_throw(dsr_gmm_set_reg_class_all(model(), c));
  }
  void resetMean() {
    if (_m) dsr_throw(dsr_mllr_reset_mean(_m, model()));
    else if (!_apt.empty()) dsr_throw(dsr_apt_reset_mean(_apt.begin()->second, model()));
  }
  // the sub-feature layout the all-pass transforms work on (CodebookSetBasic::subFeatLen / nSubFeat); one sub-feature of dimN until set
  void setSubFeatures(unsigned subFeatLen, unsigned nSubFeat = 1) { _subLen = (int) subFeatLen; _nSub = (int) nSubFeat; }
  int nSubFeat() const { return _nSub; }
  // the all-pass handle of this set for one kind and bias type, made on first use
  dsr_apt* aptAdapter(int kind, int biasType = 0) {
    dsr_apt*& h = _apt[kind * 4 + biasType];
    if (!h) { const int L = _subLen ? _subLen : dsr_gmm_dim(model()) / _nSub; dsr_throw(dsr_apt_create(model(), 1, kind, L, _nSub, biasType, &h)); }
    return h;
  }
  dsr_gmm* model() const { if (!_g) throw jconsistency_error("the codebook set has no model yet: build its DistribSet first"); return _g; }
  // the MLLR handle of this set, made on first use: its originals are the means the set was loaded with
  dsr_mllr* adapter() { if (!_m) dsr_throw(dsr_mllr_create(model(), 1, &_m)); return _m; }
  void bind(dsr_gmm* g) { _g = g; }
 private:
  dsr_gmm* _g; dsr_mllr* _m; std::map<int, dsr_apt*> _apt; int _subLen, _nSub;
};
typedef std::shared_ptr<CodebookSetAdapt> CodebookSetAdaptPtr;

class TransformerTree {                                       // TransformerTree(cbs, paramTree) (transform.cc:2122-2163)
 public:
  TransformerTree(CodebookSetAdaptPtr cbs, ParamTreePtr paramTree) : _cbs(cbs), _paramTree(paramTree) {}
  virtual ~TransformerTree() {}
  TransformerTree& transform() {
    printf("\nTransforming Means\n"); fflush(stdout);
    dsr_mllr* m = _cbs->adapter();
    dsr_throw(dsr_param_tree_copy(dsr_mllr_tree(m, 0), _paramTree->handle())); dsr_throw(dsr_mllr_adapt(m, 0, _cbs->model()));
    return *this;
  }
  ParamTreePtr& paramTree() { return _paramTree; }
 protected:
  CodebookSetAdaptPtr _cbs; ParamTreePtr _paramTree;
};
typedef std::shared_ptr<TransformerTree> TransformerTreePtr;
inline void adaptCbk(CodebookSetAdaptPtr cbs, ParamTreePtr paramTree) { TransformerTree(cbs, paramTree).transform(); }
inline void adaptCbk(CodebookSetAdaptPtr cbs, APTParamTreePtr paramTree) {      // BLTTransformer / SLAPTTransformer per class
  printf("\nTransforming Means\n"); fflush(stdout);
  dsr_apt* m = cbs->aptAdapter(paramTree->type() ? paramTree->type() : (int) APT_SLAPT);
  dsr_throw(dsr_apt_params_copy(dsr_apt_store(m, 0), paramTree->handle())); dsr_throw(dsr_apt_adapt(m, 0, cbs->model()));
}

class DistribSetTrain;
class CodebookSetTrain : public CodebookSetAdapt {            // a CodebookSetAdapt, as in the reference
 public:
  CodebookSetTrain(const String& descFile = "", FeatureSetPtr fs = FeatureSetPtr(), const String& cbkFile = "", double massThreshold = 5.0)
    : CodebookSetAdapt(descFile, fs, cbkFile), _massThreshold(massThreshold), _t(0), _totalPr(0.0f), _totalT(0) {}
  dsr_train* trainHandle() const { return need(); }
  void allocAccus() { if (_t) dsr_throw(dsr_train_zero(_t, 1, 1, 1)); }
  void zeroAccus(unsigned nParts = 1, unsigned part = 1) { dsr_throw(dsr_train_zero(need(), 1, (int) nParts, (int) part)); }
  void saveAccus(const String& fileName, float totalPr = 0.0f, unsigned totalT = 0, bool onlyCountsFlag = false) { dsr_throw(dsr_train_save_codebook_accus(need(), fileName.c_str(), totalPr, totalT, onlyCountsFlag)); }
  void loadAccus(const String& fileName, float& totalPr, unsigned& totalT, float factor = 1.0f, unsigned nParts = 1, unsigned part = 1) {
    dsr_throw(dsr_train_load_codebook_accus(need(), fileName.c_str(), &totalPr, &totalT, factor, (int) nParts, (int) part));
  }
  void loadAccus(const String& fileName) { loadAccus(fileName, _totalPr, _totalT); }
  void update(int nParts = 1, int part = 1, bool verbose = false) { (void) verbose; dsr_throw(dsr_train_update(need(), 1, nParts, part)); }
  void updateMMI(int nParts = 1, int part = 1, double E = 1.0) { dsr_throw(dsr_train_update_mmi(need(), 1, E, 0, nParts, part)); }
  void floorVariances(unsigned nParts = 1, unsigned part = 1) {
    unsigned total = 0, floored = 0; dsr_throw(dsr_train_floor_variances(need(), (int) nParts, (int) part, &total, &floored));
    printf("Floored %d of %d total variance components.\n", floored, total); fflush(stdout);
  }
  void fixGConsts(unsigned nParts = 1, unsigned part = 1) { dsr_throw(dsr_train_fix_gconsts(need(), (int) nParts, (int) part)); }
  void invertVariances(unsigned nParts = 1, unsigned part = 1) { dsr_throw(dsr_train_invert_variances(need(), (int) nParts, (int) part)); }
  double massThreshold() const { return _massThreshold; }
 private:
  friend class DistribSetTrain;
  dsr_train* need() const { if (!_t) throw jconsistency_error("Must allocate codebook accumulators before accumulating FB statistics: build the DistribSetTrain first"); return _t; }
  double _massThreshold; dsr_train* _t; float _totalPr; unsigned _totalT;
};
typedef std::shared_ptr<CodebookSetTrain> CodebookSetTrainPtr;

class DistribTrain {                                          // DistribTrain::split (distribTrain.cc:92-109)
 public:
  DistribTrain(dsr_train* t, dsr_gmm* g, int x) : _t(t), _g(g), _x(x) {}
  String name() const { return dsr_gmm_dist_name(_g, _x); }
  void split(float minCount = 0.0f, float splitFactor = 0.2f) { unsigned r = 0; dsr_throw(dsr_train_split(_t, _x, minCount, splitFactor, &r)); }
 private:
  dsr_train* _t; dsr_gmm* _g; int _x;
};

class DistribSetTrain : public DistribSetBasic {
 public:
  DistribSetTrain(CodebookSetTrainPtr& cbs, const String& descFile = "", const String& distFile = "")
    : DistribSetBasic(base(cbs), descFile, distFile), _cbsT(cbs), _t(0) {
    dsr_throw(dsr_train_create(gmm(), cbs->massThreshold(), &_t)); cbs->_t = _t; cbs->bind(gmm());
  }
  ~DistribSetTrain() { _cbsT->_t = 0; _cbsT->bind(0); dsr_train_destroy(_t); }
  DistribTrain find(const String& key) { return DistribTrain(_t, gmm(), (int) index(key)); }
  DistribTrain find(unsigned dsX) { if (dsX >= ndists()) throw jindex_error("distribution index out of range"); return DistribTrain(_t, gmm(), (int) dsX); }
  double accumulate(const DistribPath& path, float factor = 1.0f) {      // distribTrain.cc:515-526
    std::vector<int32_t> ids(path.size()); for (size_t i = 0; i < path.size(); i++) ids[i] = (int32_t) index(path[i]);
    double score = 0.0;
    dsr_throw(dsr_train_accumulate_path(_t, frames(path.size()), (int64_t) path.size(), ids.data(), factor, &score, 0));
    printf("Finished accumulation for %d frames.\n", (int) path.size()); fflush(stdout);
    return score;
  }
  void accumulateLattice(LatticePtr& lat, float factor = 1.0f) {        // distribTrain.cc:528-561
    const int E = dsr_lattice_num_edges(lat->handle()); std::vector<int32_t> end((size_t) (E > 0 ? E : 1)); std::vector<uint32_t> in(end.size());
    dsr_throw(dsr_lattice_get(lat->handle(), 0, 0, 0, in.data(), 0, 0, end.data(), 0, 0));
    int T = 0; for (int e = 0; e < E; e++) if (in[(size_t) e] != 0 && end[(size_t) e] + 1 > T) T = end[(size_t) e] + 1;
    unsigned n = 0; dsr_throw(dsr_train_accumulate_lattice(_t, lat->handle(), frames((size_t) T), T, factor, &n, 0));
    printf("Finished accumulation for %d links.\n", n); fflush(stdout);
  }
  void zeroAccus(int nParts = 1, int part = 1) { dsr_throw(dsr_train_zero(_t, 2, nParts, part)); }
  void saveAccus(const String& fileName) { dsr_throw(dsr_train_save_distrib_accus(_t, fileName.c_str())); }
  void loadAccus(const String& fileName, unsigned nParts = 1, unsigned part = 1) { dsr_throw(dsr_train_load_distrib_accus(_t, fileName.c_str(), 1.0f, (int) nParts, (int) part)); }
  void update(int nParts = 1, int part = 1) { dsr_throw(dsr_train_update(_t, 2, nParts, part)); }
  void updateMMI(int nParts = 1, int part = 1, bool merialdo = false) { dsr_throw(dsr_train_update_mmi(_t, 2, 1.0, merialdo, nParts, part)); }
  void save(const String& cbkFile, const String& distFile) { dsr_throw(dsr_gmm_save(gmm(), cbkFile.c_str(), distFile.c_str())); }
  dsr_train* trainHandle() const { return _t; }
 private:
  static CodebookSetBasicPtr& base(CodebookSetTrainPtr& cbs) { static thread_local CodebookSetBasicPtr b; b = cbs; return b; }
  const float* frames(size_t T) {                                        // frames 0..T-1 of the feature stream, on the device
    const int D = dsr_gmm_dim(gmm()); std::vector<float> x(T * (size_t) D);
    for (size_t t = 0; t < T; t++) { const float* p = featureStream()->next((int) t); for (int d = 0; d < D; d++) x[t * D + d] = p[d]; }
    const float* dev = 0; dsr_throw(dsr_train_upload_features(_t, x.data(), (int64_t) T, &dev)); return dev;
  }
  CodebookSetTrainPtr _cbsT; dsr_train* _t;
};
typedef std::shared_ptr<DistribSetTrain> DistribSetTrainPtr;

// ---- asr/train/estimateAdapt.h:913-921, estimateAdapt.cc:3064-3165: EstimatorTreeMLLR(cbs, paramTree, trace, threshold) and
// estimateAdaptationParameters(tree).  The statistics are the accumulators of the codebook set's training handle.
class EstimatorTreeMLLR : public TransformerTree {
 public:
  EstimatorTreeMLLR(CodebookSetTrainPtr& cb, ParamTreePtr& paramTree, int trace = 1, float threshold = 1500.0f)
    : TransformerTree(cb, paramTree), _cbsT(cb), _trace(trace), _threshold(threshold), _estimated(false) {
    const int G = dsr_gmm_num_gaussians(cb->model()); std::vector<uint16_t> cls((size_t) (G > 0 ? G : 1)); int present = 0;
    dsr_throw(dsr_gmm_get_reg_classes(cb->model(), cls.data(), &present));
    for (int g = 0; g < G; g++) if (!present || cls[(size_t) g] == 0) throw jindex_error("Regression class index must be >= 1");
  }
  void estimate() {
    dsr_mllr* m = _cbsT->adapter();
    dsr_throw(dsr_mllr_set_stats(m, 0, _cbsT->trainHandle())); dsr_throw(dsr_mllr_estimate(m, _threshold, 0));
    dsr_throw(dsr_param_tree_copy(_paramTree->handle(), dsr_mllr_tree(m, 0))); _estimated = true;
    if (!(_trace & 1)) return;
    int n = 0; dsr_throw(dsr_mllr_get_plan(m, &n, 0)); std::vector<int32_t> p((size_t) 4 * (n > 0 ? n : 1)); dsr_throw(dsr_mllr_get_plan(m, &n, p.data()));
    for (int i = 0; i < n; i++) {
      if (p[4 * i + 3]) printf("Copying parameters for node %d from node %d.\n", p[4 * i + 2], p[4 * i + 1]);
      else if (p[4 * i + 1] != p[4 * i + 2]) printf("Backing off from node %d to node %d.\n", p[4 * i + 2], p[4 * i + 1]);
    }
    fflush(stdout);
  }
  void writeParams(const String& fileName) { _paramTree->write(fileName); }
  double ttlFrames() {                                        // EstimatorTree::ttlFrames (estimateAdapt.cc:3052-3062): summed over ALL nodes
    if (!_estimated) throw jconsistency_error("ttlFrames is known after estimateAdaptationParameters");
    dsr_mllr* m = _cbsT->adapter(); int n = 0; dsr_throw(dsr_mllr_get_nodes(m, &n, 0, 0));
    std::vector<uint32_t> nodes((size_t) (n > 0 ? n : 1)); dsr_throw(dsr_mllr_get_nodes(m, &n, nodes.data(), 0));
    double ttl = 0.0; for (int k = 0; k < n; k++) { double t = 0.0; dsr_throw(dsr_mllr_ttl_frames(m, 0, nodes[(size_t) k], &t)); ttl += t; }
    return ttl;
  }
 private:
  CodebookSetTrainPtr _cbsT; int _trace; float _threshold; bool _estimated;
};
typedef std::shared_ptr<EstimatorTreeMLLR> EstimatorTreeMLLRPtr;
inline void estimateAdaptationParameters(EstimatorTreeMLLRPtr& tree) { tree->estimate(); }

// ---- train.i:366-386: EstimatorTreeSLAPT(cbs, paramTree, biasType, paramN, noItns, trace, threshold), and the same tree of BLTEstimatorAdapt
// nodes (estimateAdapt.cc:1623-1690).  Only paramN = 1, the line search of the reference's one-parameter branch, is implemented: the
// reference's default of 9 parameters is a jparameter_error here.  The tree is not cleared and nothing is copied (estimateAdapt.cc:3064-3133).
class EstimatorTreeSLAPT {
 public:
  EstimatorTreeSLAPT(CodebookSetTrainPtr& cb, APTParamTreePtr& paramTree, const String& biasType = "CepstraOnly", unsigned paramN = 1,
                     unsigned noItns = 10, int trace = 1, float threshold = 150.0f, int kind = APT_SLAPT)
    : _cbsT(cb), _paramTree(paramTree), _kind(kind), _trace(trace), _threshold(threshold) {
    (void) noItns;
    if (biasType == "NONE" || biasType == "None") _bias = 0;                    // getBiasType (estimateAdapt.cc:49-63)
    else if (biasType == "CEPSTRAONLY" || biasType == "CepstraOnly") _bias = 1;
    else if (biasType == "ALLCOMPONENTS" || biasType == "AllComponents") _bias = 2;
    else throw jtype_error("Unrecognized bias type " + biasType);
    dsr_throw(dsr_apt_set_param_n(cb->aptAdapter(_kind, _bias), (int) paramN));
  }
  virtual ~EstimatorTreeSLAPT() {}
  void estimate() {
    dsr_apt* m = _cbsT->aptAdapter(_kind, _bias);
    dsr_throw(dsr_apt_params_copy(dsr_apt_store(m, 0), _paramTree->handle()));
    dsr_throw(dsr_apt_set_stats(m, 0, _cbsT->trainHandle())); dsr_throw(dsr_apt_estimate(m, _threshold, 0));
    dsr_throw(dsr_apt_params_copy(_paramTree->handle(), dsr_apt_store(m, 0)));
    if (!(_trace & 1)) return;
    int n = 0; dsr_throw(dsr_apt_get_plan(m, &n, 0)); std::vector<int32_t> p((size_t) 3 * (n > 0 ? n : 1)); dsr_throw(dsr_apt_get_plan(m, &n, p.data()));
    for (int i = 0; i < n; i++) if (p[3 * i + 1] != p[3 * i + 2]) printf("Backing off from node %d to node %d.\n", p[3 * i + 2], p[3 * i + 1]);
    fflush(stdout);
  }
  void writeParams(const String& fileName) { _paramTree->write(fileName); }
  APTParamTreePtr& paramTree() { return _paramTree; }
  void transform() { adaptCbk(_cbsT, _paramTree); }
 private:
  CodebookSetTrainPtr _cbsT; APTParamTreePtr _paramTree; int _kind, _bias, _trace; float _threshold;
};
typedef std::shared_ptr<EstimatorTreeSLAPT> EstimatorTreeSLAPTPtr;
class EstimatorTreeBLT : public EstimatorTreeSLAPT {
 public:
  EstimatorTreeBLT(CodebookSetTrainPtr& cb, APTParamTreePtr& paramTree, const String& biasType = "CepstraOnly", int trace = 1, float threshold = 150.0f)
    : EstimatorTreeSLAPT(cb, paramTree, biasType, 1, 10, trace, threshold, APT_RAPT) {}
};
typedef std::shared_ptr<EstimatorTreeBLT> EstimatorTreeBLTPtr;
inline void estimateAdaptationParameters(EstimatorTreeSLAPTPtr& tree) { tree->estimate(); }
inline void estimateAdaptationParameters(EstimatorTreeBLTPtr& tree) { tree->estimate(); }

// ---- asr/train/fsa.h, train.i:531-590: FeatureSpaceAdaptationFeature(src, maxAccu, maxTran, nm), feature-space adaptation (constrained MLLR).
// A feature stream that delivers src under transformation 0, and the estimator of such transformations over dsr_fsa_* (include/dsr.h section 11).
// accumulate() pulls the scoring frames from the feature stream of the distribution set and the statistics' frames from src, both from frame 0
// after a reset().
class FeatureSpaceAdaptationFeature : public VectorFloatFeatureStream {
 public:
  FeatureSpaceAdaptationFeature(VectorFloatFeatureStreamPtr& src, unsigned maxAccu = 1, unsigned maxTran = 1, const String& nm = "FeatureSpaceAdaptationFeature")
    : _s(src) { dsr_stream* h = 0; dsr_throw(dsr_fsa_feature_create(src->handle(), (int) maxAccu, (int) maxTran, nm.c_str(), &h)); this->adopt(h); }
  void distribSet(DistribSetBasicPtr& dss) { dsr_throw(dsr_fsa_feature_distrib_set(_h, dss->gmm())); _dss = dss; }
  dsr_fsa* fsaHandle() const { dsr_fsa* f = dsr_fsa_feature_handle(_h); if (!f) throw jconsistency_error("Must initialize the distribution set before using."); return f; }
  unsigned topN() const { return dsr_fsa_top_n(fsaHandle()); }
  void setTopN(unsigned topN) { dsr_throw(dsr_fsa_set_top_n(fsaHandle(), topN)); }
  unsigned count(unsigned accuX = 0) const { double c = 0.0; dsr_throw(dsr_fsa_count(fsaHandle(), (int) accuX, &c)); return (unsigned) c; }
  float shift() const { return dsr_fsa_shift(fsaHandle()); }
  void setShift(float shift) { dsr_throw(dsr_fsa_set_shift(fsaHandle(), shift)); }
  void accumulate(const DistribPath& path, unsigned accuX = 0, float factor = 1.0f) {        // fsa.cc:282-297: an unknown name does not advance the frame
    dsr_fsa* f = fsaHandle(); std::vector<int32_t> ids(path.size()); size_t T = 0;
    for (size_t i = 0; i < path.size(); i++) { int x = -1; if (dsr_distribset_find(_dss->handle(), path[i].c_str(), &x) != DSR_OK) x = -1; ids[i] = x; if (x >= 0) T++; }
    const float *xs = 0, *xr = 0; frames(T, &xs, &xr);
    unsigned n = 0; dsr_throw(dsr_fsa_accumulate_path(f, xs, xr, (int64_t) T, ids.data(), (int64_t) ids.size(), (int) accuX, factor, &n, 0));
    printf("Accumulated %u frames.\n", n); fflush(stdout);
  }
  void accumulateLattice(LatticePtr& lat, unsigned accuX = 0, float factor = 1.0f) {         // fsa.cc:299-321: every second frame of a link
    (void) fsaHandle(); const int E = dsr_lattice_num_edges(lat->handle()); std::vector<int32_t> end((size_t) (E > 0 ? E : 1)); std::vector<uint32_t> in(end.size());
    dsr_throw(dsr_lattice_get(lat->handle(), 0, 0, 0, in.data(), 0, 0, end.data(), 0, 0));
    int T = 0; for (int e = 0; e < E; e++) if (in[(size_t) e] != 0 && end[(size_t) e] + 1 > T) T = end[(size_t) e] + 1;
    const float *xs = 0, *xr = 0; frames((size_t) T, &xs, &xr);
    unsigned n = 0; dsr_throw(dsr_fsa_accumulate_lattice(fsaHandle(), lat->handle(), xs, xr, T, (int) accuX, factor, &n, 0));
    printf("Finished accumulation for %d links.\n", n); fflush(stdout);
  }
  void zeroAccu(unsigned accuX = 0) { dsr_throw(dsr_fsa_zero(fsaHandle(), (int) accuX)); }
  void scaleAccu(float scale, unsigned accuX = 0) { dsr_throw(dsr_fsa_scale(fsaHandle(), scale, (int) accuX)); }
  void addAccu(unsigned accuX, unsigned accuY, float factor = 1.0f) { dsr_throw(dsr_fsa_add_accu(fsaHandle(), (int) accuX, (int) accuY, factor)); }
  void add(unsigned dsX) { dsr_throw(dsr_fsa_add(fsaHandle(), (int) dsX)); }
  void addAll() { dsr_throw(dsr_fsa_add_all(fsaHandle())); }
  void estimate(unsigned iterN = 1, unsigned accuX = 0, unsigned tranX = 0) {
    const int32_t a = (int32_t) accuX, t = (int32_t) tranX; dsr_throw(dsr_fsa_estimate(fsaHandle(), (int) iterN, &a, &t, 1, 0));
  }
  void clear(unsigned tranX = 0) { dsr_throw(dsr_fsa_clear(fsaHandle(), (int) tranX)); }
  float compareTransform(unsigned tranX, unsigned tranY) { float s = 0.0f; dsr_throw(dsr_fsa_compare(fsaHandle(), (int) tranX, (int) tranY, &s)); return s; }
  void saveAccu(const String& name, unsigned accuX = 0) { dsr_throw(dsr_fsa_save_accu(fsaHandle(), name.c_str(), (int) accuX)); }
  void loadAccu(const String& name, unsigned accuX = 0, float factor = 1.0f) { dsr_throw(dsr_fsa_load_accu(fsaHandle(), name.c_str(), (int) accuX, factor)); }
  void save(const String& name, unsigned tranX = 0) { dsr_throw(dsr_fsa_save(fsaHandle(), name.c_str(), (int) tranX)); }
  void load(const String& name, unsigned tranX = 0) { dsr_throw(dsr_fsa_load(fsaHandle(), name.c_str(), (int) tranX)); }
 private:
  void frames(size_t T, const float** xs, const float** xr) {             // frames 0..T-1 of both streams, on the device
    const size_t D = size(); std::vector<float> a(T * D + 1), b(T * D + 1);
    _s->reset();
    for (size_t t = 0; t < T; t++) { const float* p = _s->next((int) t); for (size_t d = 0; d < D; d++) b[t * D + d] = p[d]; }
    VectorFloatFeatureStreamPtr& f = _dss->featureStream();
    if (f.get() == _s.get()) a = b;
    else { f->reset(); for (size_t t = 0; t < T; t++) { const float* p = f->next((int) t); for (size_t d = 0; d < D; d++) a[t * D + d] = p[d]; } }
    dsr_throw(dsr_fsa_upload_features(fsaHandle(), a.data(), b.data(), (int64_t) T, xs, xr));
  }
  VectorFloatFeatureStreamPtr _s; DistribSetBasicPtr _dss;
};
typedef std::shared_ptr<FeatureSpaceAdaptationFeature> FeatureSpaceAdaptationFeaturePtr;

// ---- asr/adapt/transform.h, adapt.i:228-304: STCTransformer / LDATransformer(src, sbFtSz, nSubFt, nm) over dsr_stc_* / dsr_lda_* (include/dsr.h
// section 12), for one sub-feature: src under matrix 0 of the handle the stream owns -- the identity until load() or an estimate.
class STCTransformer : public VectorFloatFeatureStream {
 public:
  STCTransformer(VectorFloatFeatureStreamPtr& src, unsigned sbFtSz = 0, unsigned nSubFt = 0, const String& nm = "STC Transformer") : _s(src) { make(sbFtSz, nSubFt, nm, false, false); }
  dsr_stc* stcHandle() const { return dsr_stc_feature_handle(_h); }
  virtual void save(const String& fileName) { dsr_throw(dsr_stc_save(stcHandle(), fileName.c_str(), 0)); }         // raw doubles, transform.cc:1852-1857
  virtual void load(const String& fileName) { dsr_throw(dsr_stc_load(stcHandle(), fileName.c_str(), 0)); }
  std::vector<double> matrix() const { const size_t D = size(); std::vector<double> A(D * D); dsr_throw(dsr_stc_get_transform(stcHandle(), 0, A.data(), 0)); return A; }
 protected:
  STCTransformer(VectorFloatFeatureStreamPtr& src, const String& nm, bool cascade, bool mmi) : _s(src) { make(0, 0, nm, cascade, mmi); }
  VectorFloatFeatureStreamPtr _s;
 private:
  void make(unsigned sbFtSz, unsigned nSubFt, const String& nm, bool cascade, bool mmi) {
    if (nSubFt > 1 || (sbFtSz != 0 && sbFtSz != _s->size())) throw jdimension_error("STCTransformer is built for one sub-feature of the source's size");
    dsr_stream* h = 0; dsr_throw(dsr_stc_feature_create(_s->handle(), cascade, mmi, nm.c_str(), &h)); this->adopt(h);
  }
};
typedef std::shared_ptr<STCTransformer> STCTransformerPtr;

class LDATransformer : public VectorFloatFeatureStream {
 public:
  LDATransformer(VectorFloatFeatureStreamPtr& src, unsigned sbFtSz = 0, unsigned nSubFt = 0, const String& nm = "LDA Transformer") : _s(src) {
    if (nSubFt > 1) throw jdimension_error("LDATransformer is built for one sub-feature");
    dsr_stream* h = 0; dsr_throw(dsr_lda_feature_create(src->handle(), (int) (sbFtSz ? sbFtSz : src->size()), nm.c_str(), &h)); this->adopt(h);
  }
  dsr_lda* ldaHandle() const { return dsr_lda_feature_handle(_h); }
  void save(const String& fileName) const { dsr_throw(dsr_lda_save(ldaHandle(), fileName.c_str(), 0)); }            // float32, transform.cc:1961-1977
  void load(const String& fileName) { dsr_throw(dsr_lda_load(ldaHandle(), fileName.c_str(), 0)); }                  // float64, transform.cc:1979-1984
  std::vector<double> matrix() const { const size_t D = _s->size(); std::vector<double> L(D * D); dsr_throw(dsr_lda_get_transform(ldaHandle(), 0, L.data())); return L; }
 protected:
  VectorFloatFeatureStreamPtr _s;
};
typedef std::shared_ptr<LDATransformer> LDATransformerPtr;

// ---- asr/train/estimateAdapt.h, train.i:390-500: STCEstimator / LDAEstimator.  pt, idx, bt and trace are accepted and unused (the parameter-tree
// path ends in "Method not yet finished" in the reference).  accumulate() pulls the scoring frames from the feature stream of the distribution
// set and the statistics' frames from src, both from frame 0 after a reset().
enum BiasType { CepstralFeat = 0, AllFeat = 1 };
namespace dsr_detail {
template <class Upload> void path_frames(VectorFloatFeatureStreamPtr& src, DistribSetBasic& dss, size_t T, Upload upload) {
  const size_t D = src->size(); std::vector<float> a(T * D + 1), b(T * D + 1);
  src->reset();
  for (size_t t = 0; t < T; t++) { const float* p = src->next((int) t); for (size_t d = 0; d < D; d++) b[t * D + d] = p[d]; }
  VectorFloatFeatureStreamPtr& f = dss.featureStream();
  if (f.get() == src.get()) a = b;
  else { f->reset(); for (size_t t = 0; t < T; t++) { const float* p = f->next((int) t); for (size_t d = 0; d < D; d++) a[t * D + d] = p[d]; } }
  upload(a.data(), b.data());
}
}
class STCEstimator : public STCTransformer {
 public:
  STCEstimator(VectorFloatFeatureStreamPtr& src, ParamTreePtr& pt, DistribSetTrainPtr& dss, unsigned idx = 0, BiasType bt = CepstralFeat, bool cascade = false,
               bool mmiEstimation = false, int trace = 1, const String& nm = "STC Estimator")
    : STCTransformer(src, nm, cascade, mmiEstimation), _dss(dss) { (void) pt; (void) idx; (void) bt; (void) trace; dsr_throw(dsr_stc_feature_distrib_set(_h, dss->gmm())); }
  void accumulate(const DistribPath& path, float factor = 1.0f) {           // estimateAdapt.cc:2265-2294
    std::vector<int32_t> ids(path.size()); for (size_t i = 0; i < path.size(); i++) ids[i] = (int32_t) _dss->index(path[i]);
    const float *xs = 0, *xr = 0; dsr_stc* h = stcHandle(); const int64_t T = (int64_t) path.size();
    dsr_detail::path_frames(_s, *_dss, path.size(), [&](const float* a, const float* b) { dsr_throw(dsr_stc_upload_features(h, a, b, T, &xs, &xr)); });
    unsigned n = 0; dsr_throw(dsr_stc_accumulate_path(h, xs, xr, T, ids.data(), T, 0, factor, &n, 0));
    printf("STCEstimator: accumulated %u %s frames.\n", n, factor > 0.0f ? "numerator" : "denominator"); fflush(stdout);
  }
  STCEstimator& estimate(unsigned rc = 1, double minE = 1.0, double multE = 1.0) {
    (void) rc; const int32_t e = 0; dsr_throw(dsr_stc_estimate(stcHandle(), &e, 1, minE, multE, 0));
    double E = 0.0; dsr_throw(dsr_stc_E(stcHandle(), 0, &E)); printf("Using E = %g\n", E); fflush(stdout); return *this;
  }
  std::vector<float> transMatrix() const { const size_t D = size(); std::vector<float> T(D * D); dsr_throw(dsr_stc_trans_matrix(stcHandle(), 0, T.data())); return T; }
  // STCEstimator::save(fileName, trans) (estimateAdapt.cc:2327-2346): the float matrix, times trans [dimN][dimN] when given
  void save(const String& fileName, const float* trans) { dsr_throw(dsr_stc_save_float(stcHandle(), fileName.c_str(), 0, trans)); }
  virtual void save(const String& fileName) { save(fileName, 0); }
  void zeroAccu() { dsr_throw(dsr_stc_zero(stcHandle(), 0)); }
  void saveAccu(const String& fileName) const { dsr_throw(dsr_stc_save_accu(stcHandle(), fileName.c_str(), 0)); }
  void loadAccu(const String& fileName) { dsr_throw(dsr_stc_load_accu(stcHandle(), fileName.c_str(), 0)); }
  double totalPr() const { double p = 0.0; dsr_throw(dsr_stc_get_accu(stcHandle(), 0, 0, 0, 0, &p, 0, 0, 0)); return p; }
  unsigned totalT() const { unsigned t = 0; dsr_throw(dsr_stc_get_accu(stcHandle(), 0, 0, 0, 0, 0, &t, 0, 0)); return t; }
 private:
  DistribSetTrainPtr _dss;
};
typedef std::shared_ptr<STCEstimator> STCEstimatorPtr;

class LDAEstimator : public LDATransformer {
 public:
  // globalCodebook: a distribution set whose codebook 0 is the global codebook
  LDAEstimator(VectorFloatFeatureStreamPtr& src, ParamTreePtr& pt, DistribSetTrainPtr& dss, const DistribSetBasicPtr& globalCodebook, unsigned idx = 0,
               BiasType bt = CepstralFeat, int trace = 1)
    : LDATransformer(src, 0, 0), _dss(dss), _global(globalCodebook) {
    (void) pt; (void) idx; (void) bt; (void) trace; dsr_throw(dsr_lda_feature_codebooks(_h, dss->gmm(), globalCodebook->gmm()));
  }
  double accumulate(const DistribPath& path, float factor = 1.0f) {         // estimateAdapt.cc:2761-2790
    std::vector<int32_t> ids(path.size()); for (size_t i = 0; i < path.size(); i++) ids[i] = (int32_t) _dss->index(path[i]);
    const float *xs = 0, *xr = 0; dsr_lda* h = ldaHandle(); const int64_t T = (int64_t) path.size();
    dsr_detail::path_frames(_s, *_dss, path.size(), [&](const float* a, const float* b) { dsr_throw(dsr_lda_upload_features(h, a, b, T, &xs, &xr)); });
    double score = 0.0; dsr_throw(dsr_lda_accumulate_path(h, xs, xr, T, ids.data(), T, 0, factor, &score, 0)); return score;
  }
  LDAEstimator& estimate(unsigned rc = 1) { (void) rc; const int32_t e = 0; dsr_throw(dsr_lda_estimate(ldaHandle(), &e, 1, 0)); return *this; }
  void zeroAccu() { dsr_throw(dsr_lda_zero(ldaHandle(), 0)); }
  void saveAccu(const String& fileName) const { dsr_throw(dsr_lda_save_accu(ldaHandle(), fileName.c_str(), 0)); }
  void loadAccu(const String& fileName) { dsr_throw(dsr_lda_load_accu(ldaHandle(), fileName.c_str(), 0)); }
 private:
  DistribSetTrainPtr _dss; DistribSetBasicPtr _global;
};
typedef std::shared_ptr<LDAEstimator> LDAEstimatorPtr;

// ---- asr/sat over dsr_sat_* (include/dsr.h section 14): SpeakerList (transform.cc:1989-1998), MeanSAT and VarianceSAT = SAT<SATBase::MeanAcc>,
// SAT<SATBase::VarianceAcc> (sat.h:736-800, sat.cc:1763-1855).  The ML slice: a likelihood threshold, extended means and the fast,
// regression-class and MMI accumulators are refused by the library.
class SpeakerList {
 public:
  SpeakerList(const String& spkrList) : _fileName(spkrList) {
    int n = 0, bytes = 0; dsr_throw(dsr_speaker_list_read(spkrList.c_str(), 0, 0, &n, &bytes));
    std::vector<char> buf((size_t) bytes + 1, '\0'); dsr_throw(dsr_speaker_list_read(spkrList.c_str(), buf.data(), bytes, &n, &bytes));
    const String all(buf.data(), (size_t) bytes);
    for (size_t p = 0; (int) _slist.size() < n; p = all.find('\n', p) + 1) _slist.push_back(all.substr(p, all.find('\n', p) - p));
  }
  const std::vector<String>& speakers() const { return _slist; }
  const String& fileName() const { return _fileName; }
 private:
  String _fileName; std::vector<String> _slist;
};
typedef std::shared_ptr<SpeakerList> SpeakerListPtr;

class SATBase {
 public:
  virtual ~SATBase() { dsr_sat_destroy(_h); }
  void zero() { dsr_throw(dsr_sat_zero(_h)); }
  // SATBase::estimate (sat.cc:1802-1839): <meanVarsStats><spkr>.cbs.accu and <spkrAdaptParms><spkr> of every speaker, then the update
  double estimate(const SpeakerListPtr& sList, const String& spkrAdaptParms, const String& meanVarsStats) {
    double r = 0.0; dsr_throw(dsr_sat_estimate_files(_h, _what, sList->fileName().c_str(), spkrAdaptParms.c_str(), meanVarsStats.c_str(), &r)); return r;
  }
  dsr_sat* satHandle() const { return _h; }
 protected:
  SATBase(CodebookSetTrainPtr& cbs, int what, int kind, unsigned meanLen, double lhoodThreshhold, double massThreshhold, unsigned nParts, unsigned part, double mmiMultiplier, bool meanOnly, int slots)
    : _cbs(cbs), _h(0), _what(what) {
    if (mmiMultiplier != 1.0 || meanOnly) throw jparameter_error("mmiMultiplier and meanOnly act in the MMI-SAT accumulators only, which are not implemented");
    dsr_throw(dsr_sat_check((int) meanLen, dsr_gmm_dim(cbs->model()), lhoodThreshhold, kind));
    dsr_throw(dsr_sat_create(cbs->trainHandle(), slots, massThreshhold, (int) nParts, (int) part, &_h));
    const dsr_status st = dsr_sat_set_apt_sub_features(_h, cbs->nSubFeat()); if (st) { dsr_sat_destroy(_h); _h = 0; dsr_throw(st); }
  }
 private:
  SATBase(const SATBase&); SATBase& operator=(const SATBase&);
  CodebookSetTrainPtr _cbs; dsr_sat* _h; int _what;
};
class MeanSAT : public SATBase {
 public:
  MeanSAT(CodebookSetTrainPtr& cbs, unsigned meanLen = 0, double lhoodThreshhold = 0.0, double massThreshhold = 0.0, unsigned nParts = 1, unsigned part = 1,
          double mmiMultiplier = 1.0, bool meanOnly = false, int slots = 16)
    : SATBase(cbs, 1, 0, meanLen, lhoodThreshhold, massThreshhold, nParts, part, mmiMultiplier, meanOnly, slots) {}
};
class VarianceSAT : public SATBase {
 public:
  VarianceSAT(CodebookSetTrainPtr& cbs, unsigned meanLen = 0, double lhoodThreshhold = 0.0, double massThreshhold = 0.0, unsigned nParts = 1, unsigned part = 1,
              double mmiMultiplier = 1.0, bool meanOnly = false, int slots = 16)
    : SATBase(cbs, 2, 1, meanLen, lhoodThreshhold, massThreshhold, nParts, part, mmiMultiplier, meanOnly, slots) {}
};
typedef std::shared_ptr<MeanSAT> MeanSATPtr;
typedef std::shared_ptr<VarianceSAT> VarianceSATPtr;

// ---- the fast form over dsr_fsat_* (include/dsr.h section 14b): CodebookSetFastSAT (codebookFastSAT.cc:571-717) and FastMeanVarianceSAT =
// SATFast<SATBase::FastAcc> (sat.h:803-844, sat.i:164-190).  The regression-class and MMI variants are not built: their constructors throw.
class CodebookSetFastSAT : public CodebookSetTrain {          // a CodebookSetTrain that keeps one fast accumulator per Gaussian
 public:
  CodebookSetFastSAT(const String& descFile = "", FeatureSetPtr fs = FeatureSetPtr(), const String& cbkFile = "", double massThreshold = 5.0)
    : CodebookSetTrain(descFile, fs, cbkFile, massThreshold), _f(0) {}
  ~CodebookSetFastSAT() { dsr_fsat_destroy(_f); }
  // normFastAccus(transTree, olen): the accumulators of the current speaker, adapted by the MLLR parameters pt, folded into the fast accumulators
  void normFastAccus(const ParamTreePtr& pt, unsigned olen = 0) {
    if (olen != 0 && (int) olen != dsr_gmm_dim(model())) throw jdimension_error("olen for extended means is not implemented");
    dsr_fsat* f = fastHandle();
    dsr_throw(dsr_fsat_set_tree(f, 0, pt->handle())); dsr_throw(dsr_fsat_set_stats(f, 0, trainHandle())); dsr_throw(dsr_fsat_norm(f, 1, 0));
  }
  void saveFastAccus(const String& fileName) { dsr_throw(dsr_fsat_save_fast(fastHandle(), fileName.c_str())); }
  void loadFastAccus(const String& fileName, unsigned nParts = 1, unsigned part = 1) { dsr_throw(dsr_fsat_load_fast(fastHandle(), fileName.c_str(), (int) nParts, (int) part)); }
  void zeroFastAccus(unsigned nParts = 1, unsigned part = 1) { (void) nParts; (void) part; dsr_throw(dsr_fsat_zero_fast(fastHandle())); }
  unsigned descLength() { unsigned dl = 0; dsr_throw(dsr_fsat_desc_length(fastHandle(), &dl)); return dl; }
  void setRegClassesToOne() { dsr_throw(dsr_fsat_set_reg_classes_to_one(fastHandle())); }
  dsr_fsat* fastHandle() {                                    // made on first use, one slot
    if (!_f) {
      dsr_throw(dsr_fsat_create(trainHandle(), 1, 0.0, 0.0, 1, 1, 0, &_f));
      const dsr_status st = dsr_sat_set_apt_sub_features(dsr_fsat_sat(_f), nSubFeat()); if (st) { dsr_fsat_destroy(_f); _f = 0; dsr_throw(st); }
    }
    return _f;
  }
 private:
  CodebookSetFastSAT(const CodebookSetFastSAT&); CodebookSetFastSAT& operator=(const CodebookSetFastSAT&);
  dsr_fsat* _f;
};
typedef std::shared_ptr<CodebookSetFastSAT> CodebookSetFastSATPtr;

class FastMeanVarianceSAT {
 public:
  FastMeanVarianceSAT(CodebookSetFastSATPtr& cbs, unsigned meanLen = 0, double lhoodThreshhold = 0.1, double massThreshhold = 10.0, unsigned nParts = 1,
                      unsigned part = 1, double mmiMultiplier = 1.0, bool meanOnly = false, unsigned maxNoRegClass = 1, int slots = 16)
    : _cbs(cbs), _h(0) {
    dsr_throw(dsr_fsat_check((int) meanLen, dsr_gmm_dim(cbs->model()), massThreshhold, mmiMultiplier, meanOnly, (int) maxNoRegClass));
    dsr_throw(dsr_fsat_create(cbs->trainHandle(), slots, lhoodThreshhold, massThreshhold, (int) nParts, (int) part, meanOnly, &_h));
    const dsr_status st = dsr_sat_set_apt_sub_features(dsr_fsat_sat(_h), cbs->nSubFeat()); if (st) { dsr_fsat_destroy(_h); _h = 0; dsr_throw(st); }
  }
  ~FastMeanVarianceSAT() { dsr_fsat_destroy(_h); }
  void zero() { dsr_throw(dsr_fsat_zero(_h)); }
  // SATFast::estimate (sat.h:825-831): the fast accumulators and description lengths are the codebook set's; the lengths the update leaves go back
  double estimate(const SpeakerListPtr& sList, const String& spkrAdaptParms, const String& meanVarsStats) {
    dsr_fsat* src = _cbs->fastHandle(); const int nB = dsr_fsat_fast_blocks(src);
    if (!nB) throw jconsistency_error("no fast accumulators: normFastAccus or loadFastAccus first");
    const size_t G = (size_t) dsr_gmm_num_gaussians(_cbs->model()), D = (size_t) dsr_gmm_dim(_cbs->model());
    std::vector<double> c(G), d(G), m(G * D), v(G * D), sc(G * nB); std::vector<uint16_t> dl(G * nB);
    dsr_throw(dsr_fsat_get_fast(src, c.data(), d.data(), m.data(), v.data(), sc.data()));
    dsr_throw(dsr_fsat_set_fast(_h, nB, c.data(), d.data(), m.data(), v.data(), sc.data()));
    dsr_throw(dsr_fsat_get_desc_len(src, dl.data())); dsr_throw(dsr_fsat_set_desc_len(_h, nB, dl.data()));
    double r = 0.0; dsr_throw(dsr_fsat_estimate_files(_h, sList->fileName().c_str(), spkrAdaptParms.c_str(), meanVarsStats.c_str(), &r));
    dsr_throw(dsr_fsat_get_desc_len(_h, dl.data())); dsr_throw(dsr_fsat_set_desc_len(src, nB, dl.data()));
    return r;
  }
  dsr_fsat* fsatHandle() const { return _h; }
 private:
  FastMeanVarianceSAT(const FastMeanVarianceSAT&); FastMeanVarianceSAT& operator=(const FastMeanVarianceSAT&);
  CodebookSetFastSATPtr _cbs; dsr_fsat* _h;
};
typedef std::shared_ptr<FastMeanVarianceSAT> FastMeanVarianceSATPtr;

#define DSR_SAT_NOT_BUILT(Name) \
  class Name { public: template <class... A> explicit Name(A&&...) { throw jparameter_error(#Name " is not built"); } }; \
  typedef std::shared_ptr<Name> Name##Ptr;
DSR_SAT_NOT_BUILT(FastRegClassSAT)                            // SATFast<RegClassAcc>: fast accumulators of several classes per Gaussian
DSR_SAT_NOT_BUILT(FastMaxMutualInfoSAT)                       // SATFast<MMIAcc>
DSR_SAT_NOT_BUILT(FastMMIRegClassSAT)                         // SATFast<MMIRegClassAcc>
#undef DSR_SAT_NOT_BUILT
