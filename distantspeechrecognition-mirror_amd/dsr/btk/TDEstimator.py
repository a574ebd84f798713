"""btk.TDEstimator: CCTDEPtr (TDEstimator.i, CCTDE.h:60-101) over two SampleFeaturePtr, a face of dsr_cctde_stream_create: next() / nextX() /
allsamples() return the nHeldMaxCC delays in seconds.  While the two sources move together, one device call serves every block pair of the
utterance.  The band limits are kept and, as in the reference, never used (CCTDE.cc:186-205 cannot be reached)."""
import ctypes as C

import numpy as np

from .. import _capi as K
from .stream import FeatureStreamPtr, lib


class CCTDEPtr(FeatureStreamPtr):
    def __init__(self, samp1, samp2, fftLen=512, nHeldMaxCC=1, freqLowerLimit=-1, freqUpperLimit=-1, nm="CCTDE"):
        h = C.c_void_p()
        K.check(lib().dsr_cctde_stream_create(samp1._h, samp2._h, int(fftLen), int(nHeldMaxCC), int(freqLowerLimit), int(freqUpperLimit), nm.encode(),
                                              C.byref(h)))
        FeatureStreamPtr.__init__(self, h, keep=(samp1, samp2))

    def setTargetFrequencyRange(self, freqLowerLimit, freqUpperLimit):
        K.check(lib().dsr_cctde_stream_set_target_frequency_range(self._h, int(freqLowerLimit), int(freqUpperLimit)))

    def _row(self, p, n, ctype, dtype):
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), (n,)).astype(dtype) if n else np.zeros(0, dtype)

    def nextX(self, chanX=0, frameX=-5):
        p = C.c_void_p(); n = C.c_size_t()
        st = lib().dsr_cctde_stream_next_x(self._h, int(chanX), int(frameX), C.byref(p), C.byref(n))
        if st == K.E_ITERATOR:
            raise StopIteration
        K.check(st)
        return self._row(p, n.value, C.c_double, np.float64)

    def allsamples(self, fftLen=-1):
        K.check(lib().dsr_cctde_stream_allsamples(self._h, int(fftLen)))

    def getSampleDelays(self):
        p = C.c_void_p(); n = C.c_size_t()
        K.check(lib().dsr_cctde_stream_get_sample_delays(self._h, C.byref(p), C.byref(n)))
        return self._row(p, n.value, C.c_int32, np.uint32)

    def getCCValues(self):
        p = C.c_void_p(); n = C.c_size_t()
        K.check(lib().dsr_cctde_stream_get_cc_values(self._h, C.byref(p), C.byref(n)))
        return self._row(p, n.value, C.c_double, np.float64)
