"""btk.feature: the MFCC operator chain with the SWIG constructor signatures of btk/feature/feature.i."""
import ctypes as C

import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, lib, _new


def _b(s):
    return s.encode() if isinstance(s, str) else s


class SampleFeaturePtr(FeatureStreamPtr):
    """feature.i:526-528; read(): see there."""

    def __init__(self, fn="", blockLen=320, shiftLen=160, padZeros=False, nm="Sample"):
        h, _ = _new(lib().dsr_sample_feature_create, blockLen, shiftLen, int(padZeros), _b(nm)); FeatureStreamPtr.__init__(self, h)
        self._rate = 16000
        if fn != "":
            self.read(fn)

    def read(self, fn, format=0, samplerate=16000, chX=1, chN=1, cfrom=0, to=-1, outsamplerate=-1, norm=0.0):
        """SampleFeature::read (feature.cc:243-393, feature.i:487-489).  The reference reads through libsndfile's sf_readf_float; here RIFF/WAV
        PCM of 8, 16, 24 or 32 bits (the library's own reader, dsr_sample_feature_read: the C++ face reads the same way).  norm == 0 keeps the file's integer scale (SFC_SET_NORM_FLOAT off), otherwise samples
        are normalised to [-1, 1) and, for norm != 1, multiplied by norm.  The error branches are the reference's: chX == 0 and chX out of range
        are jconsistency errors, an empty range a jio error.  Sample-rate conversion (outsamplerate != the file's rate; SRCONV builds only) is
        refused.  Returns the number of frames read."""
        n = C.c_int(0)
        st = lib().dsr_sample_feature_read(self._h, _b(fn), int(format), int(samplerate), int(chX), int(chN), int(cfrom), int(to), int(outsamplerate),
                                           C.c_float(norm), C.byref(n))
        if st == K.E_IO:
            raise IOError((lib().dsr_last_error() or b"").decode(errors="replace"))
        K.check(st)
        self._rate = lib().dsr_sample_feature_sample_rate(self._h)
        return n.value

    def setSamples(self, samples, sampleRate=16000):
        a = np.ascontiguousarray(samples, dtype=np.float32)
        K.check(lib().dsr_sample_feature_set_samples(self._h, a.ctypes.data_as(C.c_void_p), a.size, int(sampleRate)))

    def getSampleRate(self):
        return self._rate


def _unary(create, dflt):
    class Op(FeatureStreamPtr):
        def __init__(self, src, *a, **kw):
            nm = kw.pop("nm", dflt)
            h, _ = _new(create, src._h, *self._args(src, *a, **kw), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(src,))
            if hasattr(self, "_post"):
                self._post()
    return Op


class PreemphasisFeaturePtr(_unary(lambda *a: lib().dsr_preemphasis_create(*a), "Preemphasis")):
    def _args(self, src, mu=0.95):
        return (float(mu),)


class HammingFeaturePtr(_unary(lambda *a: lib().dsr_hamming_create(*a), "Hamming")):
    def _args(self, src):
        return ()


HammingFeatureShortPtr = HammingFeaturePtr


class FFTFeaturePtr(_unary(lambda *a: lib().dsr_fft_create(*a), "FFT")):
    def _args(self, src, fftLen=512):
        return (int(fftLen),)


class SpectralPowerFeaturePtr(_unary(lambda *a: lib().dsr_spectral_power_create(*a), "Power")):
    def _args(self, src, powN=0):
        return (int(powN),)


PowerFeaturePtr = SpectralPowerFeaturePtr


class VTLNFeaturePtr(_unary(lambda *a: lib().dsr_vtln_create(*a), "VTLN")):
    def _args(self, src, coeffN=0, ratio=1.0, edge=1.0, version=1):
        return (int(coeffN), float(ratio), float(edge), int(version))


class MelFeaturePtr(_unary(lambda *a: lib().dsr_mel_create(*a), "MelFFT")):
    def _args(self, src, powN=0, rate=16000.0, low=0.0, up=0.0, filterN=30, version=1):
        return (int(powN), float(rate), float(low), float(up), int(filterN), int(version))


class LogFeaturePtr(_unary(lambda *a: lib().dsr_log_create(*a), "LogMel")):
    def _args(self, src, m=1.0, a=1.0, sphinxFlooring=False):
        return (float(m), float(a), int(sphinxFlooring))


class CepstralFeaturePtr(_unary(lambda *a: lib().dsr_cepstral_create(*a), "Cepstral")):
    def _args(self, src, ncep=13, type=1):
        return (int(ncep), int(type))


class _LpcBase(FeatureStreamPtr):
    """lpc.h:86-195,262-331 (feature.i: WarpMVDRFeaturePtr(src, order=60, correlate=0, warp=0.0, nm=...))."""
    _method = 0; _kind = 0; _dflt = "MVDR"

    def __init__(self, src, order=60, correlate=0, warp=0.0, nm=None):
        h, _ = _new(lib().dsr_lpc_feature_create, src._h, int(order), int(correlate), float(warp), self._method, self._kind, _b(nm or self._dflt))
        FeatureStreamPtr.__init__(self, h, keep=(src,))


class WarpMVDRFeaturePtr(_LpcBase):
    _method = 0; _kind = 0; _dflt = "MVDR"


class BurgMVDRFeaturePtr(_LpcBase):
    _method = 1; _kind = 0; _dflt = "MVDR"


class WarpLPCFeaturePtr(_LpcBase):
    _method = 0; _kind = 1; _dflt = "LPC"


class BurgLPCFeaturePtr(_LpcBase):
    _method = 1; _kind = 1; _dflt = "LPC"


class WarpedTwiceMVDRFeaturePtr(FeatureStreamPtr):
    """lpc.h:205-246, feature.i:1326: the warped MVDR envelope re-warped by a fixed or per-frame amount."""

    def __init__(self, src, order=60, correlate=0, warp=0.0, warpFactorFixed=False, sensibility=0.1, nm="WTMVDR"):
        h, _ = _new(lib().dsr_wtmvdr_feature_create, src._h, int(order), int(correlate), float(warp), int(bool(warpFactorFixed)), float(sensibility), _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(src,))


class SpectralSmoothingPtr(FeatureStreamPtr):
    """lpc.h:342-358, feature.i:1409: adjustTo scaled to the smoothed peak of adjustFrom."""

    def __init__(self, adjustTo, adjustFrom, nm="Spectral Smoothing"):
        h, _ = _new(lib().dsr_spectral_smoothing_create, adjustTo._h, adjustFrom._h, _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(adjustTo, adjustFrom))


class FilterFeaturePtr(FeatureStreamPtr):
    """feature.h:1315-1410, feature.i: an odd-length FIR across frames (the delta and delta-delta filter)."""

    def __init__(self, src, coeffA, nm="Filter"):
        a = np.ascontiguousarray(np.asarray(coeffA, dtype=np.float64).reshape(-1))
        h, _ = _new(lib().dsr_filter_feature_create, src._h, K._ptr(a), int(a.size), _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(src,))


class SamplerateConversionFeaturePtr(FeatureStreamPtr):
    """feature.h:794-816, feature.i: the source's blocks resampled from sourcerate to destrate and served in blocks of len samples (0: the source's
    size times the ratio, in float arithmetic).  method: "best", "medium", "fastest", "zoh" or "linear".  The converter is the library's own
    (include/dsr.h section 6d), not libsamplerate."""

    def __init__(self, src, sourcerate=22050, destrate=16000, len=0, method="fastest", nm="SamplerateConversion"):
        h, _ = _new(lib().dsr_src_stream_create, src._h, int(sourcerate), int(destrate), int(len), _b(method), _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(src,))


class MergeFeaturePtr(FeatureStreamPtr):
    """feature.h:1423-1441: static, delta and delta-delta features side by side."""

    def __init__(self, stat, delta, deltaDelta, nm="Merge"):
        h, _ = _new(lib().dsr_merge_feature_create, stat._h, delta._h, deltaDelta._h, _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(stat, delta, deltaDelta))


class SignalPowerFeaturePtr(FeatureStreamPtr):
    """feature.i:899: the mean square of a block over (65536^2 / 4), one value a frame."""

    def __init__(self, samp, nm="Signal Power"):
        h, _ = _new(lib().dsr_signal_power_create, samp._h, _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(samp,))


class ALogFeaturePtr(FeatureStreamPtr):
    """feature.i:928: m log10(max / 10^a + x), max over the utterance or, with runon, over everything seen since nextSpeaker()."""

    def __init__(self, samp, m=1.0, a=4.0, runon=False, nm="ALog Power"):
        h, _ = _new(lib().dsr_alog_create, samp._h, float(m), float(a), int(bool(runon)), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(samp,))

    def nextSpeaker(self):
        K.check(lib().dsr_minmax_next_speaker(self._h))


class NormalizeFeaturePtr(FeatureStreamPtr):
    """feature.i:958: the source's [min, max] mapped onto [min, max] of the arguments."""

    def __init__(self, samp, min=0.0, max=1.0, runon=False, nm="Normalize"):
        h, _ = _new(lib().dsr_normalize_create, samp._h, float(min), float(max), int(bool(runon)), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(samp,))

    def nextSpeaker(self):
        K.check(lib().dsr_minmax_next_speaker(self._h))


class ThresholdFeaturePtr(FeatureStreamPtr):
    """feature.i:986: mode "upper", "lower" or "both"; any other is a key error."""

    def __init__(self, samp, value=0.0, thresh=1.0, mode="upper", nm="Threshold"):
        h, _ = _new(lib().dsr_threshold_create, samp._h, float(value), float(thresh), _b(mode), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(samp,))


class SpectralResamplingFeaturePtr(FeatureStreamPtr):
    """feature.i:1016: linear interpolation of a spectrum onto len (0: as many) points at ratio times the source's spacing."""

    def __init__(self, src, ratio=K.SPECTRAL_SAMPLE_RATIO, len=0, nm="Resampling"):
        h, _ = _new(lib().dsr_spectral_resampling_create, src._h, float(ratio), int(len), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(src,))


class SphinxMelFeaturePtr(FeatureStreamPtr):
    """feature.i:1148: Sphinx's unnormalised triangular mel filters; the defaults lowerF = upperF = 0 give an all-zero bank, as there."""

    def __init__(self, mag, fftN=512, powerN=0, sampleRate=16000.0, lowerF=0.0, upperF=0.0, filterN=30, nm="Sphinx Mel Filter Bank"):
        h, _ = _new(lib().dsr_sphinx_mel_feature_create, mag._h, int(fftN), int(powerN), float(sampleRate), float(lowerF), float(upperF), int(filterN), _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(mag,))


class ZeroCrossingRateHammingFeaturePtr(FeatureStreamPtr):
    """feature.i:1883: the Hamming-weighted zero-crossing rate of a block."""

    def __init__(self, samp, nm="Zero Crossing Rate Hamming"):
        h, _ = _new(lib().dsr_zcr_hamming_create, samp._h, _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(samp,))


class YINPitchFeaturePtr(FeatureStreamPtr):
    """feature.i:1908: the YIN fundamental-frequency estimate of a block in Hz, 0 where none is found."""

    def __init__(self, samp, samplerate=16000, threshold=0.5, nm="YIN Pitch"):
        h, _ = _new(lib().dsr_yin_pitch_create, samp._h, int(samplerate), float(threshold), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(samp,))


class SpikeFilterPtr(FeatureStreamPtr):
    """feature.i:1936: a running median of tapN (odd, at least 3) samples within each block."""

    def __init__(self, src, tapN=3, nm="Spike Filter"):
        h, _ = _new(lib().dsr_spike_filter_create, src._h, int(tapN), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(src,))


class SpikeFilter2Ptr(FeatureStreamPtr):
    """feature.i:1968: steep slopes against a running mean slope mark a spike, which is replaced by a straight line."""

    def __init__(self, src, width=3, maxslope=7000.0, startslope=100.0, thresh=15.0, alpha=0.2, verbose=1, nm="Spike Filter 2"):
        h, _ = _new(lib().dsr_spike_filter2_create, src._h, int(width), float(maxslope), float(startslope), float(thresh), float(alpha), int(verbose), _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(src,))

    def spikesN(self):
        n = C.c_uint(0); K.check(lib().dsr_spike_filter2_spikes(self._h, C.byref(n)))
        return n.value


class AmplificationFeaturePtr(FeatureStreamPtr):
    """feature.i:2169: every sample times amplify."""

    def __init__(self, src, amplify=1.0, nm="Amplification"):
        h, _ = _new(lib().dsr_amplification_create, src._h, float(amplify), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(src,))


class StorageFeaturePtr(_unary(lambda *a: lib().dsr_storage_create(*a), "Storage")):
    def _args(self, src):
        return ()

    def evaluate(self):
        self.reset(); n = 0
        try:
            while True:
                self.next(n); n += 1
        except StopIteration:
            pass
        return n - 1

    def write(self, fileName, plainText=False):
        """StorageFeature::write (feature.cc:3025-3050)"""
        K.check(lib().dsr_storage_write(self._h, fileName.encode(), int(bool(plainText))))

    def read(self, fileName):
        """StorageFeature::read (feature.cc:3052-3066)"""
        K.check(lib().dsr_storage_read(self._h, fileName.encode()))


class MeanSubtractionFeaturePtr(_unary(lambda *a: lib().dsr_mean_subtraction_create(*a), "Mean Subtraction")):
    def _args(self, src, weight=None, devNormFactor=0.0, runon=False):
        self._weight = weight
        return (float(devNormFactor), int(runon))

    def _post(self):
        if getattr(self, "_weight", None) is not None:                    # (the operator keeps a reference of its own; self._weight keeps the Python face alive)
            K.check(lib().dsr_mean_subtraction_set_weight(self._h, self._weight._h))


class AdjacentFeaturePtr(_unary(lambda *a: lib().dsr_adjacent_create(*a), "Adjacent")):
    def _args(self, src, delta=5):
        return (int(delta),)


class LinearTransformFeaturePtr(_unary(lambda *a: lib().dsr_linear_transform_create(*a), "Transform")):
    def _args(self, src, sz=0):
        self._shape = (int(sz), src.size()); return (int(sz),)

    def setMatrix(self, m):
        a = np.ascontiguousarray(m, dtype=np.float32)
        if a.shape != self._shape:
            raise K.DsrError(5, "Matrix (%d x %d) does not match (%d x %d)" % (a.shape + self._shape))
        K.check(lib().dsr_linear_transform_set(self._h, a.ctypes.data_as(C.c_void_p)))

    def identity(self):
        if self._shape[0] != self._shape[1]:
            raise K.DsrError(5, "Cannot set an (%d x %d) matrix to identity." % self._shape)
        self.setMatrix(np.eye(self._shape[0], dtype=np.float32))

    def load(self, fileName, old=False):
        """LinearTransformFeature::load(fileName, old) (feature.cc:2972-2976): GSL raw float block or Janus 'FMAT' file (gslmatrix.cc:27-96),
        with the reference's error branches (dsr_linear_transform_load)"""
        K.check(lib().dsr_linear_transform_load(self._h, fileName.encode(), int(bool(old))))


class FeatureSetPtr(object):
    """feature.h:1486-1501: name -> stream registry the codebooks look their feature up in."""

    def __init__(self, nm="FeatureSet"):
        self._d = {}

    def add(self, feat):
        self._d[feat.name()] = feat

    def feature(self, nm):
        return self._d[nm]
