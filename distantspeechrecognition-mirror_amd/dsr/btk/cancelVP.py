"""btk.cancelVP: NLMSAcousticEchoCancellationFeaturePtr, KalmanFilterEchoCancellationFeaturePtr, BlockKalmanFilterEchoCancellationFeaturePtr,
InformationFilterEchoCancellationFeaturePtr, SquareRootInformationFilterEchoCancellationFeaturePtr, DTDBlockKalmanFilterEchoCancellationFeaturePtr
(cancelVP.i:62-254) -- constructor signatures, defaults and inheritance of the SWIG interface.

As in the reference the adaptive state outlives reset(): NLMS and Kalman zero their filter coefficients (cancelVP.h:60, :98), the block variants
keep filter, covariance and played history (:134-142), DTD also its three smoothed scalars, the information filters their per-bin scalars, the
plain one its count of skipped (frame, bin) pairs, the square-root one its information state.  The reference fixes the information filter's
diagonal load at the first call in the process (a function-static, cancelVP.cc:610); here every object uses its own `loading`."""
import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, lib, _new


class _EchoCanceller(FeatureStreamPtr):
    def _make(self, aec, played, recorded, nm):
        self._aec = aec
        h, _ = _new(lib().dsr_aec_stream_create, aec.h, played._h, recorded._h, nm.encode())
        FeatureStreamPtr.__init__(self, h, keep=(played, recorded, aec))

    def _get(self, what, shape, dt):
        import ctypes as C
        out = np.zeros(shape, dt); n = C.c_size_t()
        K.check(lib().dsr_aec_stream_get(self._h, int(what), out.ctypes.data_as(C.c_void_p), out.size * (2 if dt is np.complex128 else 1), C.byref(n)))
        return out

    def filterCoefficients(self):
        """[fftLen/2+1][sampleN] complex128"""
        return self._get(K.Aec.FILTER, (self._aec.F, self._aec.L), np.complex128)


class NLMSAcousticEchoCancellationFeaturePtr(_EchoCanceller):
    def __init__(self, original, distorted, delta=100.0, epsilon=1.0E-04, threshold=100.0, nm="AEC"):
        self._make(K.Aec("nlms", original.size(), delta=delta, epsilon=epsilon, threshold=threshold), original, distorted, nm)


class KalmanFilterEchoCancellationFeaturePtr(_EchoCanceller):
    """sigmau2 and crossCorrTh are taken and ignored, as the SWIG constructor ignores them (cancelVP.i:108-113)."""

    def __init__(self, played, recorded, beta=0.95, sigmau2=10e-4, sigma2=5.0, threshold=100.0, crossCorrTh=0.5, nm="KFEchoCanceller"):
        self._make(K.Aec("kalman", played.size(), beta=beta, sigma2=sigma2, threshold=threshold), played, recorded, nm)

    def covariance(self):
        return self._get(K.Aec.K, (self._aec.F, 1, 1), np.complex128)

    def sigma2v(self):
        return self._get(K.Aec.SIGMA2V, (self._aec.F,), np.float64)


class BlockKalmanFilterEchoCancellationFeaturePtr(KalmanFilterEchoCancellationFeaturePtr):
    def __init__(self, played, recorded, sampleN=1, beta=0.95, sigmau2=10e-4, sigmak2=5.0, threshold=100.0, amp4play=1.0, nm="BlockKFEchoCanceller"):
        self._make(K.Aec("block", played.size(), sampleN, beta=beta, sigmau2=sigmau2, sigmak2=sigmak2, threshold=threshold, amp4play=amp4play),
                   played, recorded, nm)

    def covariance(self):
        return self._get(K.Aec.K, (self._aec.F, self._aec.L, self._aec.L), np.complex128)


class InformationFilterEchoCancellationFeaturePtr(BlockKalmanFilterEchoCancellationFeaturePtr):
    _KIND = "info"

    def __init__(self, played, recorded, sampleN=1, beta=0.95, sigmau2=10e-4, sigmak2=5.0, snrTh=2.0, engTh=100.0, smooth=0.9, loading=1.0e-02, amp4play=1.0,
                 nm="DTDBlockKFEchoCanceller"):
        self._make(K.Aec(self._KIND, played.size(), sampleN, beta=beta, sigmau2=sigmau2, sigmak2=sigmak2, amp4play=amp4play, snrTh=snrTh, engTh=engTh,
                         smooth=smooth, loading=loading), played, recorded, nm)

    def bandScalars(self):
        """[fftLen/2+1][3]: _EkEnergy, _SkEnergy, _snr of every bin"""
        return self._get(K.Aec.BAND, (self._aec.F, 3), np.float64)

    def skippedN(self):
        """_skippedN, and how often the reset rule fired (cancelVP.cc:550-560)"""
        return int(self._get(K.Aec.SKIPPED, (1,), np.float64)[0]), int(self._get(K.Aec.RESETS, (1,), np.float64)[0])


class SquareRootInformationFilterEchoCancellationFeaturePtr(InformationFilterEchoCancellationFeaturePtr):
    """covariance() is the inverse Cholesky factor the reference keeps in _K_k (lower triangular)."""
    _KIND = "sqrtinfo"

    def __init__(self, played, recorded, sampleN=1, beta=0.95, sigmau2=10e-4, sigmak2=5.0, snrTh=2.0, engTh=100.0, smooth=0.9, loading=1.0e-02, amp4play=1.0,
                 nm="Square Root Information Filter Echo Cancellation Feature"):
        InformationFilterEchoCancellationFeaturePtr.__init__(self, played, recorded, sampleN, beta, sigmau2, sigmak2, snrTh, engTh, smooth, loading, amp4play, nm)

    def informationState(self):
        return self._get(K.Aec.INFO, (self._aec.F, self._aec.L), np.complex128)

    def skippedN(self):
        raise AttributeError("the square-root information filter does not count skipped frames (cancelVP.cc:781)")


class DTDBlockKalmanFilterEchoCancellationFeaturePtr(BlockKalmanFilterEchoCancellationFeaturePtr):
    def __init__(self, played, recorded, sampleN=1, beta=0.95, sigmau2=10e-4, sigmak2=5.0, snrTh=2.0, engTh=100.0, smooth=0.9, amp4play=1.0,
                 nm="DTDBlockKFEchoCanceller"):
        self._make(K.Aec("dtd", played.size(), sampleN, beta=beta, sigmau2=sigmau2, sigmak2=sigmak2, amp4play=amp4play, snrTh=snrTh, engTh=engTh,
                         smooth=smooth), played, recorded, nm)

    def dtdScalars(self):
        """_EkEnergy, _SkEnergy, _snr"""
        return self._get(K.Aec.DTD, (3,), np.float64)
