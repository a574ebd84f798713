"""btk.convolution: block convolution of a sample stream with an impulse response, the constructor signatures of btk/convolution/convolution.i."""
import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, lib, _new


def _b(s):
    return s.encode() if isinstance(s, str) else s


def _response(impulseResponse):
    if impulseResponse is None:
        raise K.DsrError(K.E_PARAMETER, "null impulse response")
    return np.ascontiguousarray(np.asarray(impulseResponse, dtype=np.float64).reshape(-1))


class OverlapAddPtr(FeatureStreamPtr):
    """convolution.h:40-72, convolution.i:52-59: blocks of samp->size() samples, the tail of a block added into the following ones."""

    def __init__(self, samp, impulseResponse, fftLen=0, nm="Overlap Add"):
        h = _response(impulseResponse)
        s, _ = _new(lib().dsr_overlap_add_create, samp._h, K._ptr(h), int(h.size), int(fftLen), _b(nm))
        FeatureStreamPtr.__init__(self, s, keep=(samp,))


class OverlapSavePtr(FeatureStreamPtr):
    """convolution.h:76-104, convolution.i:82-91: overlapping blocks of a power-of-two size above the response's length come in, the
    size - P samples of each that the circular convolution leaves intact go out."""

    def __init__(self, samp, impulseResponse, nm="Overlap Save"):
        h = _response(impulseResponse)
        s, _ = _new(lib().dsr_overlap_save_create, samp._h, K._ptr(h), int(h.size), _b(nm))
        FeatureStreamPtr.__init__(self, s, keep=(samp,))

    def update(self, delta):
        """add delta (complex, one value per sample of a block) to the frequency response; holds from the next reset() on"""
        d = np.ascontiguousarray(np.asarray(delta, dtype=np.complex128).reshape(-1))
        K.check(lib().dsr_overlap_save_update(self._h, K._ptr(d), int(d.size)))
