"""btk.sad: the speech activity detectors of btk/sad/sad.i over dsr_sad_* handles (include/dsr.h section 7b): the VAD metrics
(EnergyVADMetric, PowerSpectrumVADMetric, NormalizedEnergyMetric, TSPSVADMetric, CCCVADMetric, NegentropyVADMetric, MutualInformationVADMetric,
LikelihoodRatioVADMetric), SimpleEnergyVAD and the hangover segmenters
(HangoverVADFeature, HangoverMIVADFeature, HangoverMultiStageVADFeature), and the spectral-shape operators of sadFeature.h (EnergyDiffusionFeature,
BandEnergyRatioFeature, NegativeEntropyFeature, SignificantSubbandsFeature).  Constructor signatures and defaults are sad.i's."""
import ctypes as C

import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, _new, lib


def _b(s):
    return s.encode() if isinstance(s, str) else s


class VADMetricPtr(object):
    """sad.i:227-262: next(frameX) returns the frame's decision, score() the value behind it; iterating resets first."""

    def __init__(self, handle, keep=()):
        self._h = handle; self._keep = list(keep)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                lib().dsr_sad_metric_release(self._h)
        except Exception:
            pass

    def next(self, frameX=-5):
        v = C.c_double(0.0)
        st = lib().dsr_sad_metric_next(self._h, int(frameX), C.byref(v))
        if st == K.E_ITERATOR:
            raise StopIteration
        K.check(st)
        return v.value

    __next__ = next

    def __iter__(self):
        self.reset(); return self

    def reset(self):
        K.check(lib().dsr_sad_metric_reset(self._h))

    def nextSpeaker(self):
        K.check(lib().dsr_sad_metric_next_speaker(self._h))

    def score(self):
        v = C.c_double(0.0); K.check(lib().dsr_sad_metric_score(self._h, C.byref(v))); return v.value


class EnergyVADMetricPtr(VADMetricPtr):
    """sad.i:265-300: 1.0 where a block's energy exceeds the `threshold` quantile of the last energiesN blocks taken outside speech."""

    def __init__(self, source, initialEnergy=5.0e+07, threshold=0.5, headN=4, tailN=10, energiesN=200, nm="Energy VAD Metric"):
        h, _ = _new(lib().dsr_sad_energy_metric_create, source._h, float(initialEnergy), float(threshold), int(headN), int(tailN), int(energiesN), _b(nm))
        VADMetricPtr.__init__(self, h, keep=(source,))

    def energyPercentile(self, percentile=50.0):
        v = C.c_double(0.0); K.check(lib().dsr_sad_metric_energy_percentile(self._h, float(percentile), C.byref(v))); return v.value


class _MultiChannelVADMetricPtr(VADMetricPtr):
    def setChannel(self, chan):
        K.check(lib().dsr_sad_metric_set_channel(self._h, chan._h)); self._keep.append(chan)

    def clearChannel(self):
        K.check(lib().dsr_sad_metric_clear_channel(self._h)); self._keep = []


FloatMultiChannelVADMetricPtr = ComplexMultiChannelVADMetricPtr = _MultiChannelVADMetricPtr


class PowerSpectrumVADMetricPtr(_MultiChannelVADMetricPtr):
    """sad.i:344-380: +1.0 where channel 0 holds more than E0 / C of the band power of all channels, else -1.0."""
    _KIND = K.SAD_POWER_RATIO

    def __init__(self, fftLen, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, nm="Power Spectrum VAD Metric"):
        h, _ = _new(lib().dsr_sad_power_metric_create, self._KIND, int(fftLen), float(sampleRate), float(lowCutoff), float(highCutoff), _b(nm))
        VADMetricPtr.__init__(self, h)

    def getMetrics(self):
        n = len(self._keep); p = np.zeros(n, np.float64)
        K.check(lib().dsr_sad_metric_powers(self._h, p.ctypes.data_as(C.c_void_p), n)); return p

    def setE0(self, E0):
        K.check(lib().dsr_sad_metric_set_e0(self._h, float(E0)))


class NormalizedEnergyMetricPtr(PowerSpectrumVADMetricPtr):
    """sad.i:382-412: the same over the square roots of the band powers."""
    _KIND = K.SAD_ENERGY_RATIO

    def __init__(self, fftLen, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, nm="NormalizedEnergyMetric"):
        PowerSpectrumVADMetricPtr.__init__(self, fftLen, sampleRate, lowCutoff, highCutoff, nm)


class TSPSVADMetricPtr(PowerSpectrumVADMetricPtr):
    """sad.i:450-481: log(p0 / (sum p - p0)) - log(E0 / sum p) > 0, E0 = 5000."""
    _KIND = K.SAD_TSPS

    def __init__(self, fftLen, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, nm="TSPS VAD Metric"):
        PowerSpectrumVADMetricPtr.__init__(self, fftLen, sampleRate, lowCutoff, highCutoff, nm)


class CCCVADMetricPtr(_MultiChannelVADMetricPtr):
    """sad.i:414-448: the mean of the nCand best PHAT cross-correlation values with channel 0; +1.0 where it stays below the threshold (0.1)."""

    def __init__(self, fftLen, nCand, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, nm="CCC VAD Metric"):
        h, _ = _new(lib().dsr_sad_ccc_metric_create, int(fftLen), int(nCand), float(sampleRate), float(lowCutoff), float(highCutoff), _b(nm))
        VADMetricPtr.__init__(self, h)

    def setNCand(self, nCand):
        K.check(lib().dsr_sad_metric_set_ncand(self._h, int(nCand)))

    def setThreshold(self, threshold):
        K.check(lib().dsr_sad_metric_set_threshold(self._h, float(threshold)))


class NegentropyVADMetricPtr(VADMetricPtr):
    """sad.i:483-523: the mean log-likelihood ratio of the per-bin generalised Gaussian against the Gaussian; shapeFactorFileName names the directory of
    _M-%04d files ("": all 2.0)."""
    _KIND = K.SAD_NEGENTROPY

    def __init__(self, source, spectralEstimator, shapeFactorFileName="", threshold=0.5, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0,
                 nm="Negentropy VAD Metric"):
        self._gg(source, None, spectralEstimator, None, shapeFactorFileName, -1.0, threshold, 0.95, sampleRate, lowCutoff, highCutoff, nm)

    def _gg(self, s1, s2, e1, e2, sf, twiddle, threshold, beta, sampleRate, lowCutoff, highCutoff, nm):
        h, _ = _new(lib().dsr_sad_gg_metric_create, self._KIND, s1._h, s2._h if s2 is not None else None, e1._h, e2._h if e2 is not None else None, _b(sf), float(twiddle),
                    float(threshold), float(beta), float(sampleRate), float(lowCutoff), float(highCutoff), _b(nm))
        VADMetricPtr.__init__(self, h, keep=(s1, s2, e1, e2))


class MutualInformationVADMetricPtr(NegentropyVADMetricPtr):
    """sad.i:525-568: the empirical mutual information of two channels under matched joint and marginal generalised Gaussians; the cross-correlation
    coefficients are smoothed with beta and carried from frame to frame until nextSpeaker().  twiddle < 0: the fixed threshold."""
    _KIND = K.SAD_MUTUAL_INFORMATION

    def __init__(self, source1, source2, spectralEstimator1, spectralEstimator2, shapeFactorFileName="", twiddle=-1.0, threshold=1.3, beta=0.95,
                 sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, nm="Mutual Information VAD Metric"):
        self._gg(source1, source2, spectralEstimator1, spectralEstimator2, shapeFactorFileName, twiddle, threshold, beta, sampleRate, lowCutoff, highCutoff, nm)


class LikelihoodRatioVADMetricPtr(NegentropyVADMetricPtr):
    """sad.i:570-612: the mean log-likelihood ratio of the two channels under a common scale."""
    _KIND = K.SAD_LIKELIHOOD_RATIO

    def __init__(self, source1, source2, spectralEstimator1, spectralEstimator2, shapeFactorFileName="", threshold=0.0, sampleRate=16000.0, lowCutoff=-1.0,
                 highCutoff=-1.0, nm="Mutual Information VAD Metric"):
        self._gg(source1, source2, spectralEstimator1, spectralEstimator2, shapeFactorFileName, -1.0, threshold, 0.95, sampleRate, lowCutoff, highCutoff, nm)


class VADPtr(VADMetricPtr):
    """sad.i:100-127: next() returns a bool."""

    def next(self, frameX=-5):
        return VADMetricPtr.next(self, frameX) > 0.5

    __next__ = next


class SimpleEnergyVADPtr(VADPtr):
    """sad.i:129-160: a frame is speech where its energy exceeds `threshold` times the recursively smoothed energy."""

    def __init__(self, samp, threshold, gamma=0.98):
        h, _ = _new(lib().dsr_sad_simple_energy_create, samp._h, float(threshold), float(gamma))
        VADMetricPtr.__init__(self, h, keep=(samp,))


class HangoverVADFeaturePtr(FeatureStreamPtr):
    """sad.i:646-680: the source's frames from headN frames above threshold to tailN frames below."""
    _KIND = K.SAD_HANGOVER

    def __init__(self, source, metric, threshold=0.5, headN=4, tailN=10, nm="Hangover VAD Feature"):
        h, _ = _new(lib().dsr_sad_hangover_create, source._h, metric._h, float(threshold), int(headN), int(tailN), self._KIND, _b(nm))
        FeatureStreamPtr.__init__(self, h, keep=(source, metric))

    def _add(self, metric, threshold):
        K.check(lib().dsr_sad_hangover_add_metric(self._h, metric._h, float(threshold))); self._keep = self._keep + (metric,)

    def nextSpeaker(self):
        K.check(lib().dsr_sad_hangover_next_speaker(self._h))

    def prefixN(self):
        v = C.c_int(0); K.check(lib().dsr_sad_hangover_prefix_n(self._h, C.byref(v))); return v.value


class HangoverMIVADFeaturePtr(HangoverVADFeaturePtr):
    """sad.i:682-716: the energy metric gates, then the second metric (< 0.5 is speech), then the third (> 0.5 is speech)."""
    _KIND = K.SAD_HANGOVER_MI

    def __init__(self, source, energyMetric, mutualInformationMetric, powerMetric, energyThreshold=0.5, mutualInformationThreshold=0.5, powerThreshold=0.5,
                 headN=4, tailN=10, nm="Hangover MIVAD Feature"):
        HangoverVADFeaturePtr.__init__(self, source, energyMetric, energyThreshold, headN, tailN, nm)
        self._add(mutualInformationMetric, mutualInformationThreshold); self._add(powerMetric, powerThreshold)

    def decisionMetric(self):
        v = C.c_int(0); K.check(lib().dsr_sad_hangover_decision_metric(self._h, C.byref(v))); return v.value


class HangoverMultiStageVADFeaturePtr(HangoverVADFeaturePtr):
    """sad.i:718-754: the energy metric gates, then the first later stage above 0.5 decides; fewer than three metrics never detect speech."""
    _KIND = K.SAD_HANGOVER_MULTISTAGE

    def __init__(self, source, energyMetric, energyThreshold=0.5, headN=4, tailN=10, nm="HangoverMultiStageVADFeature"):
        HangoverVADFeaturePtr.__init__(self, source, energyMetric, energyThreshold, headN, tailN, nm)

    def setMetric(self, metricPtr, threshold):
        self._add(metricPtr, threshold)

    decisionMetric = HangoverMIVADFeaturePtr.decisionMetric


class _ShapeFeaturePtr(FeatureStreamPtr):
    def _make(self, src, op, sampleRate, thresh, nm):
        h, _ = _new(lib().dsr_sad_shape_create, src._h, op, float(sampleRate), float(thresh), _b(nm)); FeatureStreamPtr.__init__(self, h, keep=(src,))


class EnergyDiffusionFeaturePtr(_ShapeFeaturePtr):
    """sad.i:782-806: the entropy (base 10) of the frame normalised to unit length."""

    def __init__(self, src, nm="Energy Diffusion"):
        self._make(src, K.SAD_ENERGY_DIFFUSION, 0.0, 0.0, nm)


class BandEnergyRatioFeaturePtr(_ShapeFeaturePtr):
    """sad.i:808-832: the root of the energy below threshF (default a quarter of the sample rate) over the energy above."""

    def __init__(self, src, sampleRate, threshF=0.0, nm="Band Energy Ratio"):
        self._make(src, K.SAD_BAND_ENERGY_RATIO, sampleRate, threshF, nm)


class NegativeEntropyFeaturePtr(_ShapeFeaturePtr):
    """sad.i:860-884: 100 (E ln cosh z - 0.374576)^2 of the rectified, normalised frame."""

    def __init__(self, src, nm="Negative Entropy"):
        self._make(src, K.SAD_NEGATIVE_ENTROPY, 0.0, 0.0, nm)


class SignificantSubbandsFeaturePtr(_ShapeFeaturePtr):
    """sad.i:886-910: how many elements of the frame normalised to unit length exceed thresh."""

    def __init__(self, src, thresh=0.0, nm="Significant Subbands"):
        self._make(src, K.SAD_SIGNIFICANT_SUBBANDS, 0.0, thresh, nm)
