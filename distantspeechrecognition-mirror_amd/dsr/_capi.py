"""ctypes binding of libdsr_hip.so (include/dsr.h).

This is plumbing: device memory and streams come from torch (ROCm), every compute call goes
through the C-ABI with raw device pointers.  There is no CPU path here; if the shared library or
a HIP device is missing the call raises.
"""
import ctypes as C
import os
import re

C_ = C

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIBPATH = os.path.join(os.path.dirname(_HERE), "lib", "libdsr_hip.so")
_lib = None

vp, i32, i64, f32, f64, u32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_uint32

ERROR_NAMES = ["OK", "JERROR", "JALLOCATION", "JARITHMETIC", "JCONSISTENCY", "JDIMENSION", "JINDEX", "JINITIALIZATION",
               "JIO", "JITERATOR", "JPYTHON", "JKEY", "JNUMERIC", "JPARAMETER", "JPARSE", "JTYPE"]
E_ITERATOR, E_IO, E_INDEX, E_DIMENSION = 9, 8, 6, 5
E_CONSISTENCY, E_KEY, E_PARAMETER, E_PARSE = 4, 11, 13, 14


class DsrError(Exception):
    """j_error (btk/common/jexception.h:57-70): carries the reference's error_type as .code."""

    def __init__(self, status, msg):
        super().__init__("%s: %s" % (ERROR_NAMES[status] if 0 <= status < len(ERROR_NAMES) else status, msg))
        self.status = status
        self.code = status - 1


class MfccCfg(C.Structure):
    _fields_ = [("blockLen", C.c_int), ("shiftLen", C.c_int), ("padZeros", C.c_int), ("mu", f64), ("fftLen", C.c_int),
                ("powN", C.c_int), ("vtlnRatio", f64), ("vtlnEdge", f64), ("vtlnVersion", C.c_int), ("rate", f32), ("low", f32),
                ("up", f32), ("filterN", C.c_int), ("melVersion", C.c_int), ("logM", f64), ("logA", f64), ("sphinxFlooring", C.c_int),
                ("ncep", C.c_int), ("dctType", C.c_int), ("cmnMode", C.c_int), ("devNormFactor", f64), ("delta", C.c_int),
                ("outDim", C.c_int)]


class DecoderCfg(C.Structure):
    _fields_ = [("beam", f64), ("lmScale", f64), ("lmPenalty", f64), ("silPenalty", f64), ("silenceX", u32),
                ("maxActive", C.c_int), ("maxCandidates", C.c_int), ("arenaTokens", i64), ("streams", C.c_int), ("topN", C.c_int), ("latticeTokens", i64),
                ("wordTrace", C.c_int), ("propagateN", C.c_int), ("fastHash", C.c_int), ("insertSilence", C.c_int), ("wordTraceLattice", C.c_int), ("wordTraces", i64)]


class DecodeResult(C.Structure):
    _fields_ = [("score", f64), ("ac", f32), ("lm", f32), ("frames", i32), ("reachedFinal", i32), ("nArcs", i32),
                ("nWords", i32), ("status", i32), ("maxActiveSeen", i32), ("activeHypos", i64), ("placements", i64), ("registerFrames", i64), ("finalStatesN", i32), ("laidOutFrames_", i32)]


_HEADER = os.path.join(os.path.dirname(os.path.dirname(_HERE)), "include", "dsr.h")
_SCALARS = {"int": C.c_int, "dsr_status": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "uint32_t": C.c_uint32, "int32_t": C.c_int32,
            "int64_t": C.c_int64, "size_t": C.c_size_t, "float": C.c_float, "double": C.c_double, "uint8_t": C.c_uint8}


def _ctype_of(decl):
    """ctypes type of one C parameter / return declaration of include/dsr.h (pointers are opaque: c_void_p; const char* is c_char_p)."""
    d = re.sub(r"/\*.*?\*/", " ", decl).strip()
    if "*" in d or "[" in d:
        return C.c_char_p if re.match(r"^const\s+char\s*\*\s*\w*$", d) else C.c_void_p
    d = re.sub(r"\bconst\b", " ", d).strip()
    toks = d.split()
    for k in (2, 1):                                   # "unsigned int x", "int x", or a bare type
        for cand in (" ".join(toks[:k]),):
            if cand in _SCALARS and len(toks) <= k + 1:
                return _SCALARS[cand]
    raise ValueError("include/dsr.h: cannot map parameter %r" % decl)


def header_prototypes(path=None):
    """{name: (restype, [argtypes])} for every function include/dsr.h declares -- the single source of the ctypes signatures, so that no
    entry point is ever called with libffi's default int promotion (a 64-bit stride passed as a 32-bit int reads stack garbage)."""
    text = open(path or _HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"\benum\s*\{.*?\}\s*;", " ", text, flags=re.S)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(dsr_\w+)\s*\(([^;{}]*?)\)\s*;", text):
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        if ret.startswith("typedef") or not ret:
            continue
        restype = None if ret == "void" else _ctype_of(ret)
        argtypes = [] if args in ("", "void") else [_ctype_of(a) for a in args.split(",")]
        out[name] = (restype, argtypes)
    return out


def declare_from_header(L):
    for name, (restype, argtypes) in header_prototypes().items():
        fn = getattr(L, name)                          # AttributeError here = a declared symbol the library does not export
        fn.restype = restype; fn.argtypes = argtypes


def load():
    """Load the library.  torch is imported first so that its HIP runtime (same SONAME) is the one bound."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (binds libamdhip64.so.7 before our library asks for it)
    path = _LIBPATH
    if os.environ.get("DSR_LIB_VARIANT"):      # A/B tooling (tools/ab_*.sh): a variant build under lib/var/<name>/, never copied over the shipped library
        path = os.path.join(os.path.dirname(_LIBPATH), "var", os.environ["DSR_LIB_VARIANT"], "libdsr_hip.so")
    if not os.path.exists(path):
        raise ImportError("libdsr_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'` (%s)" % path)
    L = C.CDLL(path)
    declare_from_header(L)
    _lib = L
    return L


def check(status):
    if status != 0:
        raise DsrError(status, (_lib.dsr_last_error() or b"").decode(errors="replace"))


def cur_stream():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a):
    return a.ctypes.data_as(vp)


def _dev(t):
    return C.c_void_p(t.data_ptr())


# ----------------------------------------------------------------------------------------------
class FilterBank:
    """OverSampledDFTAnalysisBank / OverSampledDFTSynthesisBank plan (btk/modulated/modulated.h:291-360)."""

    def __init__(self, prototype, M, m, r, synthesis=False, delayCompensationType=0, gainFactor=1):
        L = load()
        p = _np(prototype, np.float64)
        if p.size != M * m:
            raise DsrError(4, "Prototype sizes do not match (%d vs. %d)." % (p.size, M * m))   # modulated.cc:268-270
        self.h = vp()
        check(L.dsr_fb_create(_ptr(p), M, m, r, int(synthesis), delayCompensationType, gainFactor, C.byref(self.h)))
        self.M, self.m, self.r, self.D, self.synthesis = M, m, r, M >> r, synthesis
        self.pd = L.dsr_fb_processing_delay(self.h)
        self.laN = (m << r) // 2 - 1 if (delayCompensationType == 2 and not synthesis) else 0      # look-ahead in blocks of D (modulated.cc:289)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_fb_destroy(self.h)

    def frames(self, nsamp):
        return _lib.dsr_fb_analysis_frames(self.h, int(nsamp))

    def blocks(self, nframes):
        return _lib.dsr_fb_synthesis_blocks(self.h, int(nframes))

    def analysis(self, x, nsamp=None):
        """x: cuda float32 [U][C][N] -> complex64 [U][C][Tmax][M/2+1]"""
        import torch
        U, Cn, N = x.shape
        if nsamp is None:
            nsamp = torch.full((U,), N, dtype=torch.int32, device=x.device)
        Tmax = max(1, max(self.frames(int(n)) for n in nsamp.tolist()))
        X = torch.empty((U, Cn, Tmax, self.M // 2 + 1, 2), dtype=torch.float32, device=x.device)
        check(_lib.dsr_fb_analysis(self.h, _dev(x), _dev(nsamp), U, Cn, N, Tmax, _dev(X), cur_stream()))
        return torch.view_as_complex(X)

    def analysis_beamform(self, bf, x, nsamp=None):
        """analysis bank + fixed-weight beamformer in one pass (dsr_fb_analysis_beamform): x cuda float32 [U][C][N] -> complex64 [U][Tmax][M/2+1]"""
        import torch
        U, Cn, N = x.shape
        if nsamp is None:
            nsamp = torch.full((U,), N, dtype=torch.int32, device=x.device)
        Tmax = max(1, max(self.frames(int(n)) for n in nsamp.tolist()))
        Y = torch.empty((U, Tmax, self.M // 2 + 1, 2), dtype=torch.float32, device=x.device)
        check(_lib.dsr_fb_analysis_beamform(self.h, bf.h, _dev(x), _dev(nsamp), U, Cn, N, Tmax, _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)

    def analysis_beamform_supported(self, bf):
        return bool(_lib.dsr_fb_analysis_beamform_supported(self.h, bf.h))

    def synthesis_run(self, Y, nframes=None):
        """Y: cuda complex64 [U][Tmax][M/2+1] -> float32 [U][nblocks*D]"""
        import torch
        U, Tmax, F = Y.shape
        if nframes is None:
            nframes = torch.full((U,), Tmax, dtype=torch.int32, device=Y.device)
        nb = max(1, max(self.blocks(int(n)) for n in nframes.tolist()))
        y = torch.zeros((U, nb * self.D), dtype=torch.float32, device=Y.device)
        Yr = torch.view_as_real(Y.contiguous())
        check(_lib.dsr_fb_synthesis(self.h, _dev(Yr), _dev(nframes), U, Tmax, nb * self.D, _dev(y), cur_stream()))
        return y


class FilterBankState:
    """what a filter bank carries from one block of a long stream to the next (dsr_fb_state): m*M - D samples per (stream, channel) for an
    analysis plan, R*m - 1 subband frames per stream for a synthesis plan."""

    def __init__(self, fb, U, C=1):
        L = load(); self.h = vp(); self.fb, self.U, self.C = fb, U, C
        self._started = False
        check(L.dsr_fb_state_create(fb.h, U, C, C_.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_fb_state_destroy(self.h)

    def reset(self):
        check(_lib.dsr_fb_state_reset(self.h))
        self._started = False

    def analysis_block(self, x, nsamp=None, last=False):
        """x: cuda float32 [U][C][N] = the block's new samples -> complex64 [U][C][T][M/2+1], T = the frames this block yields"""
        import torch
        U, Cn, N = x.shape
        ns = [N] * U if nsamp is None else [int(v) for v in nsamp]
        # include/dsr.h: the look-ahead of delayCompensationType 2 is spent inside a stream's first block, which must hold it
        if not self._started and not last and min(ns) < self.fb.laN * self.fb.D:
            raise DsrError(E_DIMENSION, "the first block of a stream must hold at least %d samples (the look-ahead)" % (self.fb.laN * self.fb.D))
        self._started = True
        nd = torch.tensor(ns, dtype=torch.int32, device=x.device)
        T = max(1, max(_lib.dsr_fb_analysis_block_frames(self.fb.h, self.h, n, int(last)) for n in ns))
        X = torch.empty((U, Cn, T, self.fb.M // 2 + 1, 2), dtype=torch.float32, device=x.device)
        check(_lib.dsr_fb_analysis_block(self.fb.h, self.h, _dev(x), _dev(nd), U, Cn, N, int(last), T, _dev(X), cur_stream()))
        return torch.view_as_complex(X)

    def synthesis_block(self, Y, nframes=None):
        """Y: cuda complex64 [U][T][M/2+1] = the block's new subband frames -> float32 [U][nblocks * D]"""
        import torch
        U, T, F = Y.shape
        nf = [T] * U if nframes is None else [int(v) for v in nframes]
        nd = torch.tensor(nf, dtype=torch.int32, device=Y.device)
        nb = max(1, max(_lib.dsr_fb_synthesis_block_blocks(self.fb.h, self.h, n) for n in nf))
        y = torch.zeros((U, nb * self.fb.D), dtype=torch.float32, device=Y.device)
        Yr = torch.view_as_real(Y.contiguous())
        check(_lib.dsr_fb_synthesis_block(self.fb.h, self.h, _dev(Yr), _dev(nd), max(nf), U, T, nb * self.fb.D, _dev(y), cur_stream()))
        return y


class Beamformer:
    """beamformerWeights + SubbandDS/GSC/MVDR weight design and apply (btk/beamformer/beamformer.h)."""

    def __init__(self, fftLen, chanN, halfBandShift=False):
        L = load()
        self.h = vp(); self.M, self.C = fftLen, chanN
        check(L.dsr_bf_create(fftLen, chanN, int(halfBandShift), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_bf_destroy(self.h)

    def calcArrayManifoldVectors(self, sampleRate, delays):
        d = _np(delays, np.float64)
        if d.size != self.C:
            raise DsrError(5, "Number of delays does not match number of channels (%d vs. %d)." % (d.size, self.C))
        check(_lib.dsr_bf_calc_array_manifold(self.h, sampleRate, _ptr(d)))

    def setDiffuseNoiseModel(self, micPositions, sampleRate, sspeed=343740.0):
        mp = _np(micPositions, np.float64)
        check(_lib.dsr_bf_set_diffuse_noise_model(self.h, _ptr(mp), sampleRate, sspeed))

    def divideAllNonDiagonalElements(self, myu):
        check(_lib.dsr_bf_divide_nondiagonal(self.h, myu))

    def setAllLevelsOfDiagonalLoading(self, w):
        check(_lib.dsr_bf_diagonal_loading(self.h, w))

    def setNoiseSpatialSpectralMatrix(self, fbinX, Rnn):
        R = _np(Rnn, np.complex128)
        check(_lib.dsr_bf_set_noise_matrix(self.h, fbinX, _ptr(R)))

    def calcMVDRWeights(self, sampleRate, dThreshold=1.0e-8):
        check(_lib.dsr_bf_calc_mvdr_weights(self.h, sampleRate, dThreshold))

    def calcGSCWeights(self, sampleRate, delays):
        d = _np(delays, np.float64)
        check(_lib.dsr_bf_calc_gsc_weights(self.h, sampleRate, _ptr(d)))

    def setActiveWeights_f(self, fbinX, packedWeight):
        w = _np(packedWeight, np.float64)
        if w.size != 2 * (self.C - 1):
            raise DsrError(5, "the size of an active weight vector must be %d but it is %d" % (2 * (self.C - 1), w.size))
        check(_lib.dsr_bf_set_active_weights(self.h, fbinX, _ptr(w)))

    def zeroActiveWeights(self):
        check(_lib.dsr_bf_zero_active_weights(self.h))

    def select(self, mode):
        check(_lib.dsr_bf_select(self.h, {"ds": 0, "mvdr": 1, "gsc": 2, "gsc_norm": 3, "mvdr_gsc": 4}.get(mode, mode)))

    def get(self, kind):
        F = self.M // 2 + 1
        shape = {0: (self.M, self.C), 1: (F, self.C), 2: (F, self.C, self.C), 3: (self.M, self.C, self.C - 1), 4: (_lib.dsr_bf_bins(self.h), self.C)}[kind]
        out = np.zeros(shape, np.complex128)
        check(_lib.dsr_bf_get(self.h, kind, _ptr(out), out.size * 2))
        return out

    # SubbandMVDRGSC (beamformer.h:394-425): the MVDR vector as quiescent weight, active weights from outside (select("mvdr_gsc"))
    def calcBlockingMatrix1(self, sampleRate, delaysT):
        self.calcGSCWeights(sampleRate, delaysT); return True

    def calcBlockingMatrix2(self):
        try:
            check(_lib.dsr_bf_calc_blocking_matrix2(self.h)); return True
        except DsrError:
            return False                                       # "You have to call calcMVDRWeights() first": the reference returns false

    def upgradeBlockingMatrix(self):
        check(_lib.dsr_bf_upgrade_blocking_matrix(self.h))

    def blockingMatrixOutput(self, X, outChanX=0):
        """X: cuda complex64 [U][C][T][F] -> B[:, outChanX]^H X, [U][T][F]"""
        import torch
        U, Cn, T, F = X.shape
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        check(_lib.dsr_bf_blocking_matrix_output(self.h, _dev(torch.view_as_real(X.contiguous())), U, T, int(outChanX), _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)

    # SubbandGSCRLS (beamformer.h:213-262): recursive-least-squares adaptation of the active weights
    def rlsConfig(self, myu=0.9, sigma2=0.0):
        check(_lib.dsr_bf_rls_config(self.h, myu, sigma2))

    def initPrecisionMatrix(self, sigma2=0.01):
        check(_lib.dsr_bf_rls_init_precision(self.h, sigma2))

    def setPrecisionMatrix(self, fbinX, Pz):
        p = np.ascontiguousarray(Pz, np.complex128)
        if p.shape != (self.C - 1, self.C - 1):
            raise DsrError(5, "the precision matrix must be %d x %d" % (self.C - 1, self.C - 1))
        check(_lib.dsr_bf_rls_set_precision(self.h, fbinX, _ptr(p)))

    def setQuadraticConstraint(self, alpha, qctype=1):
        check(_lib.dsr_bf_rls_quadratic_constraint(self.h, alpha, qctype))

    def updateActiveWeightVecotrs(self, flag):
        check(_lib.dsr_bf_rls_adapt(self.h, int(bool(flag))))

    def gsc_rls(self, X, nframes=None):
        """X: cuda complex64 [U][C][T][F] -> (Y [U][T][F], final active weights [U][F][C-1] complex128); nframes: cuda int32 [U] valid frames"""
        import torch
        U, Cn, T, F = X.shape
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        wa = torch.zeros((U, F, Cn - 1), dtype=torch.complex128, device=X.device)
        check(_lib.dsr_bf_gsc_rls(self.h, _dev(torch.view_as_real(X.contiguous())), _dev(nframes) if nframes is not None else None, U, T, _dev(Y), _dev(wa), cur_stream()))
        return torch.view_as_complex(Y), wa

    def rlsCarry(self, on=True):
        """keep adapting from call to call (block streaming; the reference's behaviour across reset())"""
        check(_lib.dsr_bf_rls_carry(self.h, int(bool(on))))

    def rlsResetState(self):
        check(_lib.dsr_bf_rls_reset_state(self.h))

    def rls_path(self):
        """bf_rls_path(chanN) of this object: the kernel gsc_rls launches and where its adaptation state lives"""
        return bf_rls_path(self.C)

    def bins(self):
        """bins per frame of apply(): fftLen/2+1, or fftLen with halfBandShift"""
        return _lib.dsr_bf_bins(self.h)

    def apply(self, X):
        """X: cuda complex64 [U][C][T][F] -> [U][T][F]"""
        import torch
        U, Cn, T, F = X.shape
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        check(_lib.dsr_bf_apply(self.h, _dev(torch.view_as_real(X.contiguous())), U, T, _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)


def calcDelaysPolar2(azimuth, elevation, micPositions):
    load()
    mp = _np(micPositions, np.float64); d = np.zeros(mp.shape[0], np.float64)
    check(_lib.dsr_calc_delays_polar2(azimuth, elevation, _ptr(mp), mp.shape[0], _ptr(d)))
    return d


class PrFilterBank:
    """PerfectReconstructionFFTAnalysisBank / SynthesisBank (modulated.cc:686-970), prototype of length 2M*m."""

    def __init__(self, prototype, M, m, r=0):
        L = load(); self.h = vp(); self.M, self.m, self.r = M, m, r
        p = _np(prototype, np.float64)
        if p.size != 2 * M * m:
            raise DsrError(4, "Prototype sizes do not match (%d vs. %d)." % (p.size, 2 * M * m))
        check(L.dsr_prfb_create(_ptr(p), M, m, r, C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_prfb_destroy(self.h)

    def analysis(self, x, nsamp=None):
        """x: cuda float32 [U][C][N] -> complex64 [U][C][T][2M]"""
        import torch
        U, Cn, N = x.shape
        if nsamp is None:
            nsamp = torch.full((U,), N, dtype=torch.int32, device=x.device)
        T = max(1, max(_lib.dsr_prfb_analysis_frames(self.h, int(n)) for n in nsamp.tolist()))
        X = torch.zeros((U, Cn, T, 2 * self.M), dtype=torch.complex64, device=x.device)
        check(_lib.dsr_prfb_analysis(self.h, _dev(x), _dev(nsamp), U, Cn, N, T, _dev(X), cur_stream()))
        return X

    def synthesis(self, Y, nframes=None):
        """Y: cuda complex64 [U][T][2M] -> float32 [U][(T-(2m-1))*D]"""
        import torch
        U, T, M2 = Y.shape
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=Y.device)
        nb = max(1, max(_lib.dsr_prfb_synthesis_blocks(self.h, int(n)) for n in nframes.tolist()))
        D = self.M >> self.r
        y = torch.zeros((U, nb * D), dtype=torch.float32, device=Y.device)
        check(_lib.dsr_prfb_synthesis(self.h, _dev(Y.contiguous()), _dev(nframes), U, T, nb * D, _dev(y), cur_stream()))
        return y


class NormalFFTBank:
    """NormalFFTAnalysisBank (modulated.cc:121-257): windowed STFT, windowType 0 rectangle / 1 Hamming / 2 Hanning."""

    def __init__(self, M, r, windowType=1):
        L = load(); self.h = vp(); self.M = M
        check(L.dsr_stft_create(M, r, windowType, C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_stft_destroy(self.h)

    def frames(self, nsamp):
        return _lib.dsr_stft_frames(self.h, int(nsamp))

    def analysis(self, x, nsamp=None):
        """x: cuda float32 [U][C][N] -> complex64 [U][C][T][M]"""
        import torch
        U, Cn, N = x.shape
        if nsamp is None:
            nsamp = torch.full((U,), N, dtype=torch.int32, device=x.device)
        T = max(1, max(self.frames(int(n)) for n in nsamp.tolist()))
        X = torch.zeros((U, Cn, T, self.M), dtype=torch.complex64, device=x.device)
        check(_lib.dsr_stft_analysis(self.h, _dev(x), _dev(nsamp), U, Cn, N, T, _dev(X), cur_stream()))
        return X


def wpe_single(Y, fftLen, lowerN, upperN, iterationsN=2, loadDb=-20.0, bandWidth=0.0, sampleRate=16000.0, nframes=None, want_filters=False, gn=None):
    """Single-channel WPE (dereverberation.cc:28-300): Y cuda complex64 [U][N][M/2+1] -> out (and the filters [U][M/2+1][P] complex128).
    gn: the filters of the utterance / block before (reset() keeps them in the reference): used as the start and overwritten."""
    import torch
    load()
    U, N, F = Y.shape
    if nframes is None:
        nframes = torch.full((U,), N, dtype=torch.int32, device=Y.device)
    out = torch.zeros((U, N, F), dtype=torch.complex64, device=Y.device)
    if gn is not None:
        check(_lib.dsr_wpe_single_continue(_dev(Y.contiguous()), _dev(nframes), U, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, _dev(out),
                                           _dev(gn), cur_stream()))
        return out, gn
    gn = torch.zeros((U, F, upperN - lowerN + 1), dtype=torch.complex128, device=Y.device) if want_filters else None
    check(_lib.dsr_wpe_single(_dev(Y.contiguous()), _dev(nframes), U, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, _dev(out),
                              _dev(gn) if want_filters else None, cur_stream()))
    return (out, gn) if want_filters else out


def wpe_multi(Y, fftLen, lowerN, upperN, iterationsN=2, loadDb=-20.0, bandWidth=0.0, sampleRate=16000.0, nframes=None, filterChan=-1, gn=None):
    """Multi-channel WPE (dereverberation.cc:281-620): Y cuda complex64 [U][C][N][M/2+1] -> (out, filters [U][C][M/2+1][C*P] complex128).
    filterChan >= 0: all channels through that channel's filter (the reference's getOutput when that channel's feature pulls first).
    gn: the filters of the utterance / block before (reset() keeps them in the reference): used as the start and overwritten."""
    import torch
    load()
    U, Cn, N, F = Y.shape
    if nframes is None:
        nframes = torch.full((U,), N, dtype=torch.int32, device=Y.device)
    out = torch.zeros((U, Cn, N, F), dtype=torch.complex64, device=Y.device)
    if gn is not None:
        if tuple(gn.shape) != (U, Cn, F, Cn * (upperN - lowerN + 1)) or gn.dtype != torch.complex128 or not gn.is_contiguous():
            raise ValueError("gn: contiguous complex128 [U][C][M/2+1][C*P] expected")
        check(_lib.dsr_wpe_multi_continue(_dev(Y.contiguous()), _dev(nframes), U, Cn, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate,
                                          int(filterChan), _dev(out), _dev(gn), cur_stream()))
        return out, gn
    gn = torch.zeros((U, Cn, F, Cn * (upperN - lowerN + 1)), dtype=torch.complex128, device=Y.device)
    check(_lib.dsr_wpe_multi(_dev(Y.contiguous()), _dev(nframes), U, Cn, N, fftLen, lowerN, upperN, iterationsN, loadDb, bandWidth, sampleRate, int(filterChan),
                             _dev(out), _dev(gn), cur_stream()))
    return out, gn


class Aec:
    """Subband echo cancellers of btk/cancelVP (include/dsr.h section 2d): kind "nlms", "kalman", "block", "dtd", "info" (the information filter)
    or "sqrtinfo" (its square-root form).  The handle holds the
    parameters (SWIG defaults of cancelVP.i unless given); the adaptive state is a device buffer of the caller (newState) that apply()
    continues from and leaves behind.  played, recorded: cuda complex64 [U][T][M/2+1]."""
    KINDS = {"nlms": 0, "kalman": 1, "block": 2, "dtd": 3, "info": 8, "sqrtinfo": 9}
    FILTER, K, SIGMA2V, DTD, HISTORY, BAND, INFO, SKIPPED, RESETS = 0, 1, 2, 3, 4, 5, 6, 7, 8

    def __init__(self, kind, fftLen, sampleN=1, delta=100.0, epsilon=1.0e-4, threshold=100.0, beta=0.95, sigma2=5.0, sigmau2=10e-4, sigmak2=5.0,
                 amp4play=1.0, snrTh=2.0, engTh=100.0, smooth=0.9, frameMode=0, loading=1.0e-2):
        L = load(); self.h = vp(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind); self.M = int(fftLen)
        if self.kind in (8, 9):
            check(L.dsr_aec_create_info(int(self.kind == 9), int(fftLen), int(sampleN), C.byref(self.h)))
        else:
            check(L.dsr_aec_create(self.kind, int(fftLen), int(sampleN), C.byref(self.h)))
        self.L = L.dsr_aec_sample_n(self.h); self.F = self.M // 2 + 1
        if self.kind == 0:
            check(L.dsr_aec_set_nlms(self.h, float(delta), float(epsilon), float(threshold)))
        elif self.kind == 1:
            check(L.dsr_aec_set_kalman(self.h, float(beta), float(sigma2), float(threshold)))
        else:
            check(L.dsr_aec_set_block(self.h, float(beta), float(sigmau2), float(sigmak2), float(threshold), float(amp4play)))
        if self.kind == 3:
            check(L.dsr_aec_set_dtd(self.h, float(snrTh), float(engTh), float(smooth)))
            check(L.dsr_aec_set_frame_mode(self.h, int(frameMode)))
        if self.kind in (8, 9):
            check(L.dsr_aec_set_info(self.h, float(snrTh), float(engTh), float(smooth), float(loading)))
            check(L.dsr_aec_set_frame_mode(self.h, int(frameMode)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_aec_destroy(self.h)

    def setFrameMode(self, mode):
        check(_lib.dsr_aec_set_frame_mode(self.h, int(mode)))

    def stateBytes(self, U):
        return int(_lib.dsr_aec_state_bytes(self.h, int(U)))

    def newState(self, U, device="cuda:0"):
        import torch
        st = torch.zeros((self.stateBytes(U) + 7) // 8, dtype=torch.float64, device=device)
        check(_lib.dsr_aec_state_init(self.h, _dev(st), int(U), cur_stream()))
        return st

    def apply(self, played, recorded, nframes=None, state=None, frame0=0):
        """-> the residual E [U][T][M/2+1] complex64; frames from nframes[u] on are zero and leave the state alone.  state None: a fresh one, discarded."""
        import torch
        U, T, F = played.shape
        if F != self.F or tuple(recorded.shape) != (U, T, F) or played.dtype != torch.complex64 or recorded.dtype != torch.complex64:
            raise ValueError("played, recorded: complex64 [U][T][%d] expected" % self.F)
        out = torch.zeros((U, T, F), dtype=torch.complex64, device=played.device)
        check(_lib.dsr_aec_apply(self.h, _dev(played.contiguous()), _dev(recorded.contiguous()), _dev(nframes) if nframes is not None else None, U, T,
                                 int(frame0), _dev(out), _dev(state) if state is not None else None, cur_stream()))
        return out

    def read(self, state, U, what):
        F, L = self.F, self.L
        shape = {0: (U, F, L), 1: (U, F, L, L), 2: (U, F), 3: (U, 3), 4: (U, F, L), 5: (U, F, 3), 6: (U, F, L), 7: (U,), 8: (U,)}[what]
        real = what in (2, 3, 5, 7, 8)
        out = np.zeros(shape, np.float64 if real else np.complex128)
        check(_lib.dsr_aec_state_read(self.h, _dev(state), int(U), int(what), _ptr(out), out.size * (1 if real else 2)))
        return out

    def resetFilter(self, state, U):
        check(_lib.dsr_aec_reset_filter(self.h, _dev(state), int(U), cur_stream()))


class Gcc:
    """The GCC family of btk/localization (include/dsr.h section 2e): kind "raw", "gnnsub", "phat", "gnnsubphat", "mlrraw" or "mlrgnnsub".
    The handle holds the pair list [P][2] and the parameters (defaults of localization.h:123); what the estimator carries from frame to
    frame is a device buffer of the caller (newState) that run() continues from and leaves behind."""
    KINDS = {"raw": 0, "gnnsub": 1, "phat": 2, "gnnsubphat": 3, "mlrraw": 4, "mlrgnnsub": 5}
    HUGE = float(np.finfo(np.float32).max)                       # <math.h> HUGE, findMaximum's default window (localization.h:126)
    NOISE_POWER, NOISE_CROSS, CROSS, CORRELATION = 0, 1, 2, 3

    def __init__(self, kind, pairs, sampleRate=44100.0, fftLen=2048, nChan=16, alpha=0.95, beta=0.5, q=0.3, interpolate=True, noisereduction=True):
        L = load(); self.h = vp(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        self.pairs = _np(pairs, np.int32).reshape(-1, 2); self.P = self.pairs.shape[0]; self.C = int(nChan); self.N = int(fftLen); self.F = self.N // 2 + 1
        self.sampleRate = float(sampleRate)
        check(L.dsr_gcc_create(self.kind, float(sampleRate), int(fftLen), int(nChan), _ptr(self.pairs), self.P, float(alpha), float(beta), float(q),
                               int(bool(interpolate)), int(bool(noisereduction)), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_gcc_destroy(self.h)

    def setAlpha(self, alpha):
        check(_lib.dsr_gcc_set_alpha(self.h, float(alpha)))

    def getAlpha(self):
        return float(_lib.dsr_gcc_alpha(self.h))

    def stateBytes(self, U):
        return int(_lib.dsr_gcc_state_bytes(self.h, int(U)))

    def newState(self, U, device="cuda:0"):
        import torch
        st = torch.zeros((self.stateBytes(U) + 7) // 8, dtype=torch.float64, device=device)
        check(_lib.dsr_gcc_state_init(self.h, _dev(st), int(U), cur_stream()))
        return st

    def run(self, X, sad, timestamp, state, nframes=None, smooth=True, minDelay=None, maxDelay=None, want_corr=False, want_xspec=False):
        """X cuda complex64 or complex128 [U][C][T][fftLen/2+1], sad [U][T] (non-zero = speech), timestamp [U][T] float64 ->
        dict(result [U][T][P][3] = delay, maxCorr, ratio; valid [U][T][P] int32; corr [U][T][P][fftLen] and xspec [U][T][P][fftLen/2+1] on request)"""
        import torch
        U, Cn, T, F = X.shape
        if Cn != self.C or F != self.F or X.dtype not in (torch.complex64, torch.complex128):
            raise ValueError("X: complex64 or complex128 [U][%d][T][%d] expected" % (self.C, self.F))
        dev = X.device
        sad = sad.to(device=dev, dtype=torch.int32).contiguous(); timestamp = timestamp.to(device=dev, dtype=torch.float64).contiguous()
        if tuple(sad.shape) != (U, T) or tuple(timestamp.shape) != (U, T):
            raise ValueError("sad, timestamp: [U][T] expected")
        r = dict(result=torch.zeros((U, T, self.P, 3), dtype=torch.float64, device=dev), valid=torch.zeros((U, T, self.P), dtype=torch.int32, device=dev))
        r["corr"] = torch.zeros((U, T, self.P, self.N), dtype=torch.float64, device=dev) if want_corr else None
        r["xspec"] = torch.zeros((U, T, self.P, F), dtype=torch.complex128, device=dev) if want_xspec else None
        Xc = torch.view_as_real(X.contiguous())
        check(_lib.dsr_gcc_run(self.h, _dev(Xc), int(X.dtype == torch.complex128), _dev(nframes) if nframes is not None else None, _dev(sad), _dev(timestamp),
                               int(bool(smooth)), float(-self.HUGE if minDelay is None else minDelay), float(self.HUGE if maxDelay is None else maxDelay), U, T,
                               _dev(state), _dev(r["result"]), _dev(r["valid"]), _dev(r["corr"]) if want_corr else None,
                               _dev(torch.view_as_real(r["xspec"])) if want_xspec else None, cur_stream()))
        return r

    def findMaximum(self, state, U, minDelay=None, maxDelay=None):
        """findMaximum over the carried correlations -> (result [U][P][3], valid [U][P]) on the device"""
        import torch
        res = torch.zeros((U, self.P, 3), dtype=torch.float64, device=state.device); valid = torch.zeros((U, self.P), dtype=torch.int32, device=state.device)
        check(_lib.dsr_gcc_find_maximum(self.h, float(-self.HUGE if minDelay is None else minDelay), float(self.HUGE if maxDelay is None else maxDelay), int(U),
                                        _dev(state), _dev(res), _dev(valid), cur_stream()))
        return res, valid

    def read(self, state, U, what, u, index):
        """-> (array, exists): noise power [F] float64, noise cross-spectrum / cross-spectrum [F] complex128, correlation [fftLen] float64"""
        cplx = what in (1, 2); n = self.N if what == 3 else self.F
        out = np.zeros(n, np.complex128 if cplx else np.float64); ex = C.c_int32(0)
        check(_lib.dsr_gcc_state_read(self.h, _dev(state), int(U), int(what), int(u), int(index), _ptr(out), n * (2 if cplx else 1), C.byref(ex)))
        return out, bool(ex.value)

    def channelDelays(self, pairDelays):
        """per-channel delays (channel 0 at zero) for dsr_bf_calc_array_manifold / Beamformer.calcArrayManifoldVectors from the P pair delays"""
        d = _np(pairDelays, np.float64).ravel()
        if d.size != self.P:
            raise DsrError(E_DIMENSION, "%d pair delays for %d pairs" % (d.size, self.P))
        out = np.zeros(self.C, np.float64); check(_lib.dsr_gcc_channel_delays(self.h, _ptr(d), _ptr(out))); return out


def cctde(a, b, fftLen, nHeldMaxCC=1, sampleRate=16000):
    """CCTDE::next over a batch of block pairs (dsr_cctde_run): a, b cuda float32 [n][blockLen] -> (delays [n][nHeld] seconds, lags as FFT
    indices [n][nHeld] int32, correlation values [n][nHeld])"""
    import torch
    load()
    a = a.to(torch.float32).contiguous(); b = b.to(torch.float32).contiguous()
    if a.dim() != 2 or a.shape != b.shape:
        raise ValueError("a, b: float32 [n][blockLen] of one shape expected")
    n, bl = a.shape
    d = torch.zeros((n, nHeldMaxCC), dtype=torch.float64, device=a.device); ar = torch.zeros((n, nHeldMaxCC), dtype=torch.int32, device=a.device)
    v = torch.zeros((n, nHeldMaxCC), dtype=torch.float64, device=a.device)
    check(_lib.dsr_cctde_run(_dev(a), _dev(b), int(n), int(bl), int(fftLen), int(nHeldMaxCC), int(sampleRate), _dev(d), _dev(ar), _dev(v), cur_stream()))
    return d, ar, v


class SearchGrid:
    """SGB4LinearArray / SGB4CircularArray (include/dsr.h section 2f): kind "linear" or "circular"; host code, no GPU needed.  Units are
    millimetres.  enumerate() walks the whole far-field grid once."""
    KINDS = {"linear": 0, "circular": 1}

    def __init__(self, kind, nChan, isFarField=True, samplingFreq=16000):
        L = load(); self.h = vp(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind); self.C = int(nChan); self.fs = int(samplingFreq)
        check(L.dsr_sgb_create(self.kind, int(nChan), int(bool(isFarField)), int(samplingFreq), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_sgb_destroy(self.h)

    def setDistanceBtwMicrophones(self, distance):
        check(_lib.dsr_sgb_set_distance(self.h, float(distance)))

    def setPositionsOfMicrophones(self, mpos):
        m = _np(mpos, np.float64); check(_lib.dsr_sgb_set_positions(self.h, _ptr(m), int(m.shape[0])))

    def setRadius(self, radius, height=0.0):
        check(_lib.dsr_sgb_set_radius(self.h, float(radius), float(height)))

    def reset(self):
        check(_lib.dsr_sgb_reset(self.h))

    def nextSearchGrid(self):
        more = C.c_int32(0); check(_lib.dsr_sgb_next(self.h, C.byref(more))); return bool(more.value)

    def getSearchPosition(self):
        out = np.zeros(3); check(_lib.dsr_sgb_position(self.h, _ptr(out))); return out

    def getTimeDelays(self):
        out = np.zeros(self.C); check(_lib.dsr_sgb_time_delays(self.h, _ptr(out))); return out

    def maxTimeDelay(self):
        return float(_lib.dsr_sgb_max_time_delay(self.h))

    def chanN(self):
        return int(_lib.dsr_sgb_chan_n(self.h))

    def samplingFrequency(self):
        return int(_lib.dsr_sgb_sampling_frequency(self.h))

    def microphonePositions(self):
        out = np.zeros((self.C, 3)); check(_lib.dsr_sgb_microphone_positions(self.h, _ptr(out))); return out

    def enumerate(self):
        """-> (positions [G][3], delays [G][C] seconds, tau [G][C] int32)"""
        G = C.c_int32(0); check(_lib.dsr_sgb_enumerate(self.h, 0, C.byref(G), None, None, None)); g = G.value
        pos = np.zeros((g, 3)); d = np.zeros((g, self.C)); tau = np.zeros((g, self.C), np.int32)
        check(_lib.dsr_sgb_enumerate(self.h, g, C.byref(G), _ptr(pos), _ptr(d), _ptr(tau)))
        return pos, d, tau


def mcc_check(sgb, maxSource=1, blockLen=0):
    """what MccLocalizer and its run() refuse, checked on the host (dsr_mcc_check)"""
    load(); check(_lib.dsr_mcc_check(sgb.h, int(maxSource), int(blockLen)))


class MccLocalizer:
    """MCCLocalizer over a batch (include/dsr.h section 2f): the grid of `sgb` is walked once at construction."""

    def __init__(self, sgb, maxSource=1):
        L = load(); self.h = vp(); self.sgb = sgb
        check(L.dsr_mcc_create(sgb.h, int(maxSource), C.byref(self.h)))
        self.C = int(L.dsr_mcc_chan_n(self.h)); self.G = int(L.dsr_mcc_grid_n(self.h)); self.S = int(maxSource); self.D = int(L.dsr_mcc_max_sample_delay(self.h))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_mcc_destroy(self.h)

    def _x(self, x, blockLen):
        import torch
        if x.dim() != 3 or x.shape[1] != self.C or x.dtype != torch.float32:
            raise ValueError("x: float32 [U][%d][N] expected" % self.C)
        x = x.contiguous(); U, _, N = x.shape
        return x, U, N, N // int(blockLen) if blockLen > 0 else 0

    def run(self, x, blockLen, nsamples=None, want_costmap=False, want_R=False, want_eig=True):
        """x cuda float32 [U][C][N] -> dict(valid [U][B], index [U][B][S], cost [U][B][S], tau [U][B][S][C], position [U][B][S][3],
        eig [U][B][S][C], costmap [U][B][G] and R [U][B][C][C] on request)"""
        import torch
        x, U, N, B = self._x(x, blockLen); dev = x.device; S = self.S; Cn = self.C
        z = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
        r = dict(valid=z((U, B), torch.int32), index=z((U, B, S), torch.int32), cost=z((U, B, S)), tau=z((U, B, S, Cn), torch.int32), position=z((U, B, S, 3)),
                 eig=z((U, B, S, Cn)) if want_eig else None, costmap=z((U, B, self.G)) if want_costmap else None, R=z((U, B, Cn, Cn)) if want_R else None)
        if nsamples is not None:
            nsamples = nsamples.to(device=dev, dtype=torch.int32).contiguous()
        opt = lambda t: _dev(t) if t is not None else None
        check(_lib.dsr_mcc_run(self.h, _dev(x), opt(nsamples), U, N, int(blockLen), _dev(r["valid"]), _dev(r["index"]), _dev(r["cost"]), _dev(r["tau"]),
                               _dev(r["position"]), opt(r["eig"]), opt(r["costmap"]), opt(r["R"]), cur_stream()))
        return r

    def calc(self, x, blockLen, delays, normalizeVariance=True, nsamples=None, want_R=False, want_eig=False):
        """MCCCalculator over the batch -> dict(valid [U][B], cost [U][B], tau [C] numpy, eig [U][B][C], R [U][B][C][C])"""
        import torch
        x, U, N, B = self._x(x, blockLen); dev = x.device; Cn = self.C
        d = _np(delays, np.float64).ravel()
        if d.size != Cn:
            raise DsrError(E_DIMENSION, "%d delays for %d channels" % (d.size, Cn))
        r = dict(valid=torch.zeros((U, B), dtype=torch.int32, device=dev), cost=torch.zeros((U, B), dtype=torch.float64, device=dev), tau=np.zeros(Cn, np.int32),
                 eig=torch.zeros((U, B, Cn), dtype=torch.float64, device=dev) if want_eig else None,
                 R=torch.zeros((U, B, Cn, Cn), dtype=torch.float64, device=dev) if want_R else None)
        if nsamples is not None:
            nsamples = nsamples.to(device=dev, dtype=torch.int32).contiguous()
        opt = lambda t: _dev(t) if t is not None else None
        check(_lib.dsr_mcc_calc(self.h, _dev(x), opt(nsamples), U, N, int(blockLen), _ptr(d), int(bool(normalizeVariance)), _dev(r["valid"]), _dev(r["cost"]),
                                _ptr(r["tau"]), opt(r["eig"]), opt(r["R"]), cur_stream()))
        return r

    def channelDelays(self, tau):
        """tau [C] samples -> the delays in seconds that Beamformer.calcArrayManifoldVectors takes"""
        t = _np(tau, np.int32).ravel()
        if t.size != self.C:
            raise DsrError(E_DIMENSION, "%d shifts for %d channels" % (t.size, self.C))
        out = np.zeros(self.C); check(_lib.dsr_mcc_channel_delays(self.h, _ptr(t), _ptr(out))); return out

    def setTiming(self, on=True):
        check(_lib.dsr_mcc_set_timing(self.h, int(bool(on))))

    def kernelMs(self):
        out = np.zeros(3); check(_lib.dsr_mcc_kernel_ms(self.h, _ptr(out))); return out


class MccCalculator(MccLocalizer):
    """MCCCalculator over a batch: one candidate from the caller's delays; calling the object is calc() with the constructor's normalizeVariance."""

    def __init__(self, sgb, normalizeVariance=True):
        MccLocalizer.__init__(self, sgb, 1); self.normalizeVariance = bool(normalizeVariance)

    def __call__(self, x, blockLen, delays, nsamples=None, want_R=False, want_eig=False):
        return self.calc(x, blockLen, delays, self.normalizeVariance, nsamples, want_R, want_eig)


class DoaSRP:
    """DOAEstimatorSRPDSBLA (btk/beamformer/beamformer.h:462-560, beamformer.cc:2920-3283) over a batch: settings and steering table on the
    host, the response powers of X [U][C][T][M/2+1] on the fp64 MFMA (dsr_doa_srp).  The accumulators belong to the caller."""

    def __init__(self, nBest, sampleRate, fftLen, chanN):
        L = load(); self.h = vp(); self.nBest, self.M, self.C = nBest, fftLen, chanN
        check(L.dsr_doa_create(int(nBest), int(sampleRate), int(fftLen), int(chanN), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_doa_destroy(self.h)

    def setArrayGeometry(self, positions):
        p = _np(positions, np.float64).ravel()
        check(_lib.dsr_doa_set_array_geometry(self.h, _ptr(p), p.size))

    def setSearchParam(self, minTheta=-np.pi / 2, maxTheta=np.pi / 2, widthTheta=0.1):
        check(_lib.dsr_doa_set_search_param(self.h, float(minTheta), float(maxTheta), float(widthTheta)))

    def setFrequencyRange(self, fbinMin, fbinMax):
        check(_lib.dsr_doa_set_frequency_range(self.h, int(fbinMin), int(fbinMax)))

    def frequencyRange(self):
        a, b = C.c_int(), C.c_int(); check(_lib.dsr_doa_frequency_range(self.h, C.byref(a), C.byref(b))); return a.value, b.value

    def setEnergyThreshold(self, threshold):
        check(_lib.dsr_doa_set_energy_threshold(self.h, float(threshold)))

    def thetaN(self):
        n = C.c_int(); check(_lib.dsr_doa_theta_n(self.h, C.byref(n))); return n.value

    def thetas(self):
        n = self.thetaN(); out = np.zeros(n, np.float64); check(_lib.dsr_doa_thetas(self.h, _ptr(out), n)); return out

    def lookDelays(self, theta):
        out = np.zeros(self.C, np.float64); check(_lib.dsr_doa_look_delays(self.h, float(theta), _ptr(out))); return out

    def steering(self, thetaX):
        out = np.zeros((self.M // 2 + 1, self.C), np.complex128)
        check(_lib.dsr_doa_steering(self.h, int(thetaX), _ptr(out), out.size * 2)); return out

    def srp(self, X, nframes=None, acc=None, want_rp=False, want_y=False):
        """X cuda complex64 [U][C][T][M/2+1] -> dict(energy [U][T] f32, nbest_rp [U][T][nBest] f64, nbest_idx [U][T][nBest] i32, gated [U][T] i32,
        acc [U][nTheta] f64 (the one passed in, added to), rp [U][T][nTheta] f64 and y [U][T][M/2+1] complex64 on request).  Frames past
        nframes[u] keep the zeros they start with."""
        import torch
        U, Cn, T, F = X.shape
        dev = X.device; nT = self.thetaN()
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=dev)
        if acc is None:
            acc = torch.zeros((U, nT), dtype=torch.float64, device=dev)
        elif tuple(acc.shape) != (U, nT) or acc.dtype != torch.float64 or not acc.is_contiguous():
            raise ValueError("acc: contiguous float64 [U][nTheta] expected")
        r = dict(energy=torch.zeros((U, T), dtype=torch.float32, device=dev), nbest_rp=torch.zeros((U, T, self.nBest), dtype=torch.float64, device=dev),
                 nbest_idx=torch.zeros((U, T, self.nBest), dtype=torch.int32, device=dev), gated=torch.zeros((U, T), dtype=torch.int32, device=dev), acc=acc)
        r["rp"] = torch.zeros((U, T, nT), dtype=torch.float64, device=dev) if want_rp else None
        r["y"] = torch.zeros((U, T, F), dtype=torch.complex64, device=dev) if want_y else None
        Xc = torch.view_as_real(X.contiguous())
        check(_lib.dsr_doa_srp(self.h, _dev(Xc), _dev(nframes), U, T, _dev(r["energy"]), _dev(r["rp"]) if want_rp else None, _dev(r["nbest_rp"]),
                               _dev(r["nbest_idx"]), _dev(acc), _dev(r["y"]) if want_y else None, _dev(r["gated"]), cur_stream()))
        return r

    def finalNBest(self, acc):
        """getFinalNBestHypotheses for each row of acc [U][nTheta] (host or device) -> (rp [U][nBest], theta index [U][nBest], -1 = empty)"""
        a = np.ascontiguousarray(acc.detach().cpu().numpy() if hasattr(acc, "detach") else acc, np.float64)
        a = a.reshape(-1, a.shape[-1]); U = a.shape[0]
        R = np.zeros((U, self.nBest), np.float64); I = np.zeros((U, self.nBest), np.int32)
        check(_lib.dsr_doa_final_nbest(self.h, _ptr(a), U, _ptr(R), _ptr(I)))
        return R, I


class _Sph:
    """the dsr_sph handle (modalBeamformer.{h,cc}): kind "EB" (EigenBeamformer weights), "DS" (SphericalDSBeamformer weights) or one of the
    further beamformers "HWNC", "GSC", "HWNCGSC", "SPATIALDS", "MOEN"; settings, geometry and tables on the host"""
    KINDS = {"EB": 0, "DS": 1, "HWNC": 2, "GSC": 3, "HWNCGSC": 4, "SPATIALDS": 5, "MOEN": 6}

    def __init__(self, kind, nBest, sampleRate, fftLen, chanN, maxOrder, normalizeWeight=False, halfBandShift=False, NC=1):
        L = load(); self.h = vp(); self.nBest, self.M, self.C = nBest, fftLen, chanN
        k = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        check(L.dsr_sph_create(k, int(nBest), int(sampleRate), int(fftLen), int(bool(halfBandShift)), int(NC), int(maxOrder), int(bool(normalizeWeight)),
                               int(chanN), C.byref(self.h)))
        self.dim = L.dsr_sph_dim(self.h); self.NC = int(NC)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_sph_destroy(self.h)

    def setWNG(self, ratio):
        check(_lib.dsr_sph_set_wng(self.h, float(ratio)))

    def setActiveWeights_f(self, fbinX, packedWeight):
        p = _np(packedWeight, np.float64).ravel()
        check(_lib.dsr_sph_set_active_weights_f(self.h, int(fbinX), _ptr(p), p.size))

    def setLevelOfDiagonalLoading(self, fbinX, diagonalWeight):
        check(_lib.dsr_sph_set_diagonal_loading(self.h, int(fbinX), float(diagonalWeight)))

    def fixTerms(self, flag):
        check(_lib.dsr_sph_fix_terms(self.h, int(bool(flag))))

    def wl(self):
        return self._table(_lib.dsr_sph_wl, (self.M // 2 + 1, self.dim))

    def blockingMatrix(self, fbinX):
        return self._table(_lib.dsr_sph_blocking_matrix, (self.dim, self.dim - self.NC), int(fbinX))

    def sensorWeights(self):
        return self._table(_lib.dsr_sph_sensor_weights, (self.M // 2 + 1, self.C))

    def setBeam(self, b, theta, phi):
        check(_lib.dsr_sph_set_beam(self.h, int(b), float(theta), float(phi)))

    def setBeamsFromNBest(self, doa, nbest_idx):
        """beams 0..n-1 = the directions of doa's (a SphDoaSRP) units nbest_idx [n], e.g. one row of finalNBest's indices"""
        idx = np.ascontiguousarray(nbest_idx, np.int32).ravel()
        check(_lib.dsr_sph_set_beams_nbest(self.h, doa.h, _ptr(idx), idx.size)); return idx.size

    def beamWeights(self, NB=1):
        """V [NB][M/2+1][C]: the sensor-domain vectors of dsr_sph_beams, y = v^H x"""
        n = max(1, min(int(NB), 16)); out = np.zeros((n, self.M // 2 + 1, self.C), np.complex128)
        check(_lib.dsr_sph_beam_weights(self.h, int(NB), _ptr(out), out.size * 2)); return out

    def beams(self, X, nframes=None, NB=1):
        """X cuda complex64 [U][C][T][M/2+1] -> y [U][NB][T][M/2+1] complex64, every beam in one pass over X (dsr_sph_beams); rows past
        nframes[u] are zero"""
        import torch
        U, Cn, T, F = X.shape
        dev = X.device
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=dev)
        y = torch.empty((U, max(int(NB), 0), T, F), dtype=torch.complex64, device=dev)
        Xc = torch.view_as_real(X.contiguous())
        check(_lib.dsr_sph_beams(self.h, _dev(Xc), _dev(nframes), U, T, int(NB), _dev(y), cur_stream()))
        return y

    def getBeamPattern(self, fbinX, theta=0.0, phi=0.0, minTheta=-np.pi, maxTheta=np.pi, minPhi=-np.pi, maxPhi=np.pi, widthTheta=0.1, widthPhi=0.1):
        a, b = C.c_int(), C.c_int()
        g = (float(minTheta), float(maxTheta), float(minPhi), float(maxPhi), float(widthTheta), float(widthPhi))
        check(_lib.dsr_sph_beam_pattern_n(*g, C.byref(a), C.byref(b)))
        out = np.zeros((max(a.value, 0), max(b.value, 0)), np.float64)
        check(_lib.dsr_sph_beam_pattern(self.h, int(fbinX), float(theta), float(phi), *g, _ptr(out), out.size)); return out

    def _table(self, fn, shape, *args):
        out = np.zeros(shape, np.complex128); check(fn(self.h, *args, _ptr(out), out.size * 2)); return out

    def setArrayGeometry(self, a, theta_s, phi_s):
        t = _np(theta_s, np.float64).ravel(); p = _np(phi_s, np.float64).ravel()
        if t.size != p.size:
            raise DsrError(E_DIMENSION, "theta_s and phi_s differ in length")
        check(_lib.dsr_sph_set_array_geometry(self.h, float(a), _ptr(t), _ptr(p), t.size))

    def setEigenMikeGeometry(self):
        check(_lib.dsr_sph_set_eigenmike_geometry(self.h))

    def getArrayGeometry(self, type):
        out = np.zeros(self.C, np.float64); check(_lib.dsr_sph_array_geometry(self.h, int(type), _ptr(out), self.C)); return out

    def setLookDirection(self, theta, phi):
        check(_lib.dsr_sph_set_look_direction(self.h, float(theta), float(phi)))

    def setSigma2(self, sigma2):
        check(_lib.dsr_sph_set_sigma2(self.h, float(sigma2)))

    def setWeightGain(self, wgain):
        check(_lib.dsr_sph_set_weight_gain(self.h, float(wgain)))

    def modeAmplitudes(self):
        return self._table(_lib.dsr_sph_mode_amplitudes, (self.M // 2 + 1, _lib.dsr_sph_max_order(self.h)))

    def harmonics(self):
        return self._table(_lib.dsr_sph_harmonics, (self.dim, self.C))

    def lookWeights(self):
        return self._table(_lib.dsr_sph_look_weights, (self.M // 2 + 1, self.dim))

    def calcWNG(self):
        out = np.zeros(self.M // 2 + 1, np.float64); check(_lib.dsr_sph_calc_wng(self.h, _ptr(out), out.size)); return out

    def apply(self, X, nframes=None, want_F=False):
        """X cuda complex64 [U][C][T][M/2+1] -> (y [U][T][M/2+1] complex64, F [U][T][M/2+1][dim] complex64 or None); frames past nframes[u] stay 0"""
        import torch
        U, Cn, T, F = X.shape
        dev = X.device
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=dev)
        y = torch.zeros((U, T, F), dtype=torch.complex64, device=dev)
        Fo = torch.zeros((U, T, F, self.dim), dtype=torch.complex64, device=dev) if want_F else None
        Xc = torch.view_as_real(X.contiguous())
        check(_lib.dsr_sph_apply(self.h, _dev(Xc), _dev(nframes), U, T, _dev(y), _dev(Fo) if want_F else None, cur_stream()))
        return y, Fo


class SphBeamformer(_Sph):
    """EigenBeamformer (kind "EB") / SphericalDSBeamformer (kind "DS") over a batch (dsr_sph_apply); the further kinds ("HWNC", "GSC",
    "HWNCGSC", "SPATIALDS", "MOEN") and several beams at once through beams() (dsr_sph_beams).  ratio: the HWNC kinds' setWNG."""

    def __init__(self, kind, sampleRate, fftLen, chanN, maxOrder, normalizeWeight=False, halfBandShift=False, NC=1, ratio=None):
        _Sph.__init__(self, kind, 1, sampleRate, fftLen, chanN, maxOrder, normalizeWeight, halfBandShift, NC)
        if ratio is not None:
            self.setWNG(ratio)


class SphDoaSRP(_Sph):
    """DOAEstimatorSRPEB (kind "EB") / DOAEstimatorSRPSphDSB (kind "DS") over a batch: the (theta, phi) grid and steering table on the host, the
    response powers of X [U][C][T][M/2+1] on the fp64 MFMA (dsr_sph_srp).  The accumulators belong to the caller."""

    def __init__(self, kind, *args, **kw):
        if (self.KINDS.get(kind, -1) if isinstance(kind, str) else int(kind)) not in (0, 1):
            raise DsrError(1, "SphDoaSRP searches with the EB or DS weights; kind %r has no steering table" % (kind,))
        _Sph.__init__(self, kind, *args, **kw)

    def setSearchParam(self, minTheta=0.0, maxTheta=np.pi, minPhi=-np.pi, maxPhi=np.pi, widthTheta=0.1, widthPhi=0.1):
        check(_lib.dsr_sph_set_search_param(self.h, float(minTheta), float(maxTheta), float(minPhi), float(maxPhi), float(widthTheta), float(widthPhi)))

    def setFrequencyRange(self, fbinMin, fbinMax):
        check(_lib.dsr_sph_set_frequency_range(self.h, int(fbinMin), int(fbinMax)))

    def frequencyRange(self):
        a, b = C.c_int(), C.c_int(); check(_lib.dsr_sph_frequency_range(self.h, C.byref(a), C.byref(b))); return a.value, b.value

    def setEnergyThreshold(self, threshold):
        check(_lib.dsr_sph_set_energy_threshold(self.h, float(threshold)))

    def gridN(self):
        a, b = C.c_int(), C.c_int(); check(_lib.dsr_sph_grid_n(self.h, C.byref(a), C.byref(b))); return a.value, b.value

    def grid(self):
        """(theta [units], phi [units]), unit = iTheta nPhi + iPhi"""
        nT, nP = self.gridN(); th = np.zeros(nT * nP); ph = np.zeros(nT * nP)
        check(_lib.dsr_sph_grid(self.h, _ptr(th), _ptr(ph), nT * nP)); return th, ph

    def units(self):
        nT, nP = self.gridN(); return nT * nP

    def steering(self, unit):
        return self._table(_lib.dsr_sph_steering, (self.M // 2 + 1, self.dim), int(unit))

    def path(self):
        p = _lib.dsr_sph_srp_path(self.h)
        if p < 0:
            raise DsrError(1, (_lib.dsr_last_error() or b"").decode(errors="replace"))
        return ("fused", "folded")[p]

    def srp(self, X, nframes=None, acc=None, want_rp=False, want_y=False):
        """as DoaSRP.srp, units in place of theta: dict(energy, nbest_rp, nbest_idx, gated, acc [U][units], rp, y)"""
        import torch
        U, Cn, T, F = X.shape
        dev = X.device; nU = self.units()
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=dev)
        if acc is None:
            acc = torch.zeros((U, nU), dtype=torch.float64, device=dev)
        elif tuple(acc.shape) != (U, nU) or acc.dtype != torch.float64 or not acc.is_contiguous():
            raise ValueError("acc: contiguous float64 [U][units] expected")
        r = dict(energy=torch.zeros((U, T), dtype=torch.float32, device=dev), nbest_rp=torch.zeros((U, T, self.nBest), dtype=torch.float64, device=dev),
                 nbest_idx=torch.zeros((U, T, self.nBest), dtype=torch.int32, device=dev), gated=torch.zeros((U, T), dtype=torch.int32, device=dev), acc=acc)
        r["rp"] = torch.zeros((U, T, nU), dtype=torch.float64, device=dev) if want_rp else None
        r["y"] = torch.zeros((U, T, F), dtype=torch.complex64, device=dev) if want_y else None
        Xc = torch.view_as_real(X.contiguous())
        check(_lib.dsr_sph_srp(self.h, _dev(Xc), _dev(nframes), U, T, _dev(r["energy"]), _dev(r["rp"]) if want_rp else None, _dev(r["nbest_rp"]),
                               _dev(r["nbest_idx"]), _dev(acc), _dev(r["y"]) if want_y else None, _dev(r["gated"]), cur_stream()))
        return r

    def finalNBest(self, acc):
        """getFinalNBestHypotheses for each row of acc [U][units] -> (rp [U][nBest], unit index [U][nBest], -1 = empty)"""
        a = np.ascontiguousarray(acc.detach().cpu().numpy() if hasattr(acc, "detach") else acc, np.float64)
        a = a.reshape(-1, a.shape[-1]); U = a.shape[0]
        R = np.zeros((U, self.nBest), np.float64); I = np.zeros((U, self.nBest), np.int32)
        check(_lib.dsr_sph_final_nbest(self.h, _ptr(a), U, _ptr(R), _ptr(I)))
        return R, I


class SphTracker:
    """The spherical-array speaker trackers of btk/beamformer/tracker.{h,cc} (include/dsr.h section 2c''): kind "modal" (ModalDecomposition +
    ModalSphericalArrayTracker) or "spatial" (SpatialDecomposition + SpatialSphericalArrayTracker) over a batch.  The handle holds the
    decomposition's tables and the tracker's parameters; the filter's state (position, K) is a device buffer of the caller (newState) that
    run() continues from and leaves behind, so an utterance may come in blocks."""
    KINDS = {"modal": 0, "spatial": 1}
    CLAMP, ERROR = 1 << 8, 1 << 9

    def __init__(self, kind, orderN, fftLen, a=42.0, sampleRate=16000.0, useSubbandsN=0, sigma2_u=10.0, sigma2_v=10.0, sigma2_init=10.0, maxLocalN=1,
                 chanN=32):
        L = load(); self.h = vp(); self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        check(L.dsr_trk_create(self.kind, int(orderN), int(fftLen), float(a), float(sampleRate), int(useSubbandsN), float(sigma2_u), float(sigma2_v),
                               float(sigma2_init), int(maxLocalN), int(chanN), C.byref(self.h)))
        self.M, self.F, self.orderN = int(fftLen), int(fftLen) // 2 + 1, int(orderN)
        self.modesN = L.dsr_trk_modes_n(self.h); self.L = L.dsr_trk_subband_length(self.h); self.useSubbandsN = L.dsr_trk_use_subbands_n(self.h)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_trk_destroy(self.h)

    @staticmethod
    def maxRows(kind, orderN, useSubbandsN):
        return int(load().dsr_trk_max_rows(SphTracker.KINDS[kind] if isinstance(kind, str) else int(kind), int(orderN), int(useSubbandsN)))

    def setV(self, Vk, subbandX):
        v = _np(Vk, np.complex128)
        if v.shape != (self.L, self.L):
            raise DsrError(E_PARAMETER, "Vk: [%d][%d] expected" % (self.L, self.L))
        check(_lib.dsr_trk_set_v(self.h, _ptr(v), v.size * 2, int(subbandX)))

    def getV(self, subbandX):
        out = np.zeros((2 * self.L, 2 * self.L), np.float64); check(_lib.dsr_trk_get_v(self.h, int(subbandX), _ptr(out), out.size)); return out

    def setInitialPosition(self, theta, phi):
        check(_lib.dsr_trk_set_initial_position(self.h, float(theta), float(phi)))

    def nextSpeaker(self):
        check(_lib.dsr_trk_next_speaker(self.h))

    def bn(self):
        out = np.zeros((self.F, self.orderN + 1), np.complex128); check(_lib.dsr_trk_bn(self.h, _ptr(out), out.size * 2)); return out

    def sensorHarmonics(self):
        out = np.zeros((self.modesN, 32), np.complex128); check(_lib.dsr_trk_sensor_harmonics(self.h, _ptr(out), out.size * 2)); return out

    @staticmethod
    def geometry():
        t, p = np.zeros(32), np.zeros(32); check(load().dsr_trk_geometry(_ptr(t), _ptr(p), 32)); return t, p

    @staticmethod
    def _static(fn, *args):
        out = np.zeros(2, np.float64); load(); check(fn(*args, _ptr(out))); return complex(out[0], out[1])

    @staticmethod
    def harmonic(order, degree, theta, phi):
        return SphTracker._static(load().dsr_trk_harmonic, int(order), int(degree), float(theta), float(phi))

    @staticmethod
    def harmonicDerivPolarAngle(order, degree, theta, phi):
        return SphTracker._static(load().dsr_trk_harmonic_deriv_polar, int(order), int(degree), float(theta), float(phi))

    @staticmethod
    def harmonicDerivAzimuth(order, degree, theta, phi):
        return SphTracker._static(load().dsr_trk_harmonic_deriv_azimuth, int(order), int(degree), float(theta), float(phi))

    @staticmethod
    def modalCoefficient(order, ka):
        return SphTracker._static(load().dsr_trk_modal_coefficient, int(order), float(ka))

    def stateDoubles(self):
        return int(_lib.dsr_trk_state_doubles(self.h))

    def newState(self, U, device="cuda:0"):
        import torch
        st = torch.zeros((int(U), self.stateDoubles()), dtype=torch.float64, device=device)
        self.initState(st); return st

    def initState(self, state, positionOnly=False):
        """positionOnly False: as nextSpeaker leaves the tracker (the handle's initial position, the initial K); True: setInitialPosition"""
        check(_lib.dsr_trk_init_state(self.h, _dev(state), int(state.shape[0]), int(bool(positionOnly)), cur_stream()))

    def run(self, X, nframes=None, state=None):
        """X cuda complex64 [U][32][T][M/2+1] -> (pos [U][T][2] float32, pos64 [U][T][2] float64, info [U][T] int32); rows past nframes[u] are
        zero.  state None: a fresh one, discarded."""
        import torch
        U, Cn, T, F = X.shape
        if Cn != 32 or F != self.F or X.dtype != torch.complex64:
            raise ValueError("X: complex64 [U][32][T][%d] expected" % self.F)
        dev = X.device
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=dev)
        if state is None:
            state = self.newState(U, dev)
        pos = torch.zeros((U, T, 2), dtype=torch.float32, device=dev); pos64 = torch.zeros((U, T, 2), dtype=torch.float64, device=dev)
        info = torch.zeros((U, T), dtype=torch.int32, device=dev)
        check(_lib.dsr_trk_run(self.h, _dev(torch.view_as_real(X.contiguous())), _dev(nframes), U, T, _dev(state), _dev(pos), _dev(pos64), _dev(info), cur_stream()))
        return pos, pos64, info


class PlaneWaveSim:
    """PlaneWaveSimulator (tracker.cc:1444-1488) for all 32 channels at once: coefficients on the host (over a SphTracker's decomposition), the
    product with the source spectrum on the device"""

    def __init__(self, tracker, theta, phi):
        self.trk, self.F, self.M = tracker, tracker.F, tracker.M
        self.coef = np.zeros((32, self.F), np.complex128)
        check(_lib.dsr_pws_coefficients(tracker.h, float(theta), float(phi), _ptr(self.coef), self.coef.size * 2))
        self._dev = None

    def apply(self, src, nframes=None, full=False):
        """src cuda complex64 [U][T][M/2+1] -> [U][32][T][M/2+1] complex64, or rows of M bins with the conjugate mirror (full)"""
        import torch
        U, T, F = src.shape
        if F != self.F or src.dtype != torch.complex64:
            raise ValueError("src: complex64 [U][T][%d] expected" % self.F)
        dev = src.device
        if self._dev is None or self._dev.device != dev:
            self._dev = torch.view_as_real(torch.from_numpy(self.coef)).contiguous().to(dev)
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=dev)
        out = torch.zeros((U, 32, T, self.M if full else F), dtype=torch.complex64, device=dev)
        check(_lib.dsr_pws_apply(_dev(self._dev), 32, _dev(torch.view_as_real(src.contiguous())), _dev(nframes), U, T, self.M, int(bool(full)), _dev(out), cur_stream()))
        return out


RLS_STATE_REGS, RLS_STATE_LDS, RLS_STATE_MEM = 0, 1, 2
PF_ZEL_REG, PF_ZEL_SUM, PF_ZEL_SUM_BF, PF_MCCOWAN_REG, PF_MCCOWAN_MEM, PF_WAVE = 0, 1, 2, 3, 4, 5


def bf_rls_path(chanN):
    """-> ((CT, CAP, residence), (bytes of the 64 lanes' state, dynamic LDS of the launch)): the k_gsc_rls<CT, REG, CAP> dsr_bf_gsc_rls launches for
    chanN channels, REG = residence == RLS_STATE_REGS; follows DSR_RLS_NOREGS / DSR_RLS_MEMSTATE; needs no device"""
    L = load()
    out = (C.c_int * 3)(); lds = (C.c_int64 * 2)()
    check(L.dsr_bf_rls_path(int(chanN), out, lds))
    return tuple(out), tuple(lds)


MK_PR, MK_NRM = 0, 1
MK_EXIT_MAX_ITERATIONS, MK_EXIT_GRADIENT, MK_EXIT_DIFFERENCE, MK_EXIT_NO_PROGRESS, MK_EXIT_EVAL_CAP, MK_EXIT_SKIPPED = 0, 1, 2, 3, 4, 5
MK_FRAMES_LDS, MK_FRAMES_STREAMED = 0, 1
MK_EVAL_CAP = 2048


def mk_path(chanN, Tsel):
    """-> ((CT, residence), (frames that fit the LDS residence, dynamic LDS of the launch)): the k_mk_minimize<CT> dsr_mk_estimate launches for chanN
    channels and Tsel selected frames, and where a problem's frames live; needs no device"""
    L = load()
    out = (C.c_int * 2)(); lds = (C.c_int64 * 2)()
    check(L.dsr_mk_path(int(chanN), int(Tsel), out, lds))
    return tuple(out), tuple(lds)


class MkBeamformer:
    """Maximum empirical kurtosis beamforming (btk/lib/mkBeamforming.py: MEKSubbandBeamformer_pr / _nrm) for a batch: every (utterance, bin) is one
    problem, all of them minimised in one launch.  kind: MK_PR (conjugate gradient) or MK_NRM (steepest descent, |wa| clipped to |gamma|); the
    defaults of alpha and DIFFSTOPTOLERANCE are the reference's for that kind."""

    def __init__(self, fftLen, chanN, kind=MK_PR, alpha=None, beta=3.0, gamma=-1.0, NC=1, nSource=1, halfBandShift=False):
        L = load()
        self.h = vp(); self.M, self.C, self.F, self.kind = fftLen, chanN, fftLen // 2 + 1, kind
        check(L.dsr_mk_create(fftLen, chanN, int(NC), int(nSource), int(bool(halfBandShift)), C.byref(self.h)))
        self.config(kind, (1.0e-2 if kind == MK_PR else 0.1) if alpha is None else alpha, beta, gamma)
        self.minimizer()

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_mk_destroy(self.h)

    def config(self, kind, alpha, beta=3.0, gamma=-1.0):
        check(_lib.dsr_mk_config(self.h, int(kind), alpha, beta, gamma)); self.kind, self.alpha = kind, alpha

    def minimizer(self, MAXITNS=40, TOLERANCE=1.0e-3, STOPTOLERANCE=1.0e-2, DIFFSTOPTOLERANCE=None, STEPSIZE=0.01):
        if DIFFSTOPTOLERANCE is None:
            DIFFSTOPTOLERANCE = 1.0e-5 if self.kind == MK_PR else 1.0e-10
        check(_lib.dsr_mk_minimizer(self.h, int(MAXITNS), TOLERANCE, STOPTOLERANCE, DIFFSTOPTOLERANCE, STEPSIZE))

    def setFixedWeightsFromBeamformer(self, bf):
        """the quiescent vectors and blocking matrices of a Beamformer after calcGSCWeights"""
        check(_lib.dsr_mk_set_fixed_weights_from_bf(self.h, bf.h))

    def setFixedWeights(self, wq, B=None):
        """wq [F][C]; B [F][C][C-1] or None for the blocking matrices of wq"""
        w = _np(wq, np.complex128)
        if w.shape != (self.F, self.C):
            raise DsrError(5, "wq must be %d x %d" % (self.F, self.C))
        b = None
        if B is not None:
            b = _np(B, np.complex128)
            if b.shape != (self.F, self.C, self.C - 1):
                raise DsrError(5, "B must be %d x %d x %d" % (self.F, self.C, self.C - 1))
        check(_lib.dsr_mk_set_fixed_weights(self.h, _ptr(w), _ptr(b) if b is not None else None))

    def getFixedWeights(self):
        wq = np.zeros((self.F, self.C), np.complex128); B = np.zeros((self.F, self.C, self.C - 1), np.complex128)
        check(_lib.dsr_mk_get_fixed_weights(self.h, _ptr(wq), _ptr(B)))
        return wq, B

    def forceStreamed(self, on=True):
        check(_lib.dsr_mk_force_streamed(self.h, int(bool(on))))

    def _args(self, X, nframes, sFrame, eFrame, R, fbinX):
        import torch
        U, Cn, T, F = X.shape
        if Cn != self.C or F != self.F or X.dtype != torch.complex64:
            raise DsrError(5, "X must be complex64 [U][%d][T][%d]" % (self.C, self.F))
        self._keep = (torch.view_as_real(X.contiguous()), nframes)
        return (_dev(self._keep[0]), _dev(nframes) if nframes is not None else None, U, T, int(sFrame), int(T if eFrame is None else eFrame), int(R), int(fbinX))

    def _wa(self, wa, X):
        import torch
        U, n = X.shape[0], self.C - 1
        if wa is None:
            return torch.zeros((U, self.F, n), dtype=torch.complex128, device=X.device)
        wa = torch.as_tensor(wa).to(device=X.device, dtype=torch.complex128)
        if tuple(wa.shape) != (U, self.F, n):
            raise DsrError(5, "the active weights must be %d x %d x %d" % (U, self.F, n))
        return wa.contiguous().clone()

    def eval(self, X, wa, nframes=None, sFrame=0, eFrame=None, R=1, stats=None, fbinX=-1):
        """X: cuda complex64 [U][C][T][F]; wa [U][F][C-1] complex128; nframes: cuda int32 [U]; stats: cuda fp64 [3][U][F]
        -> (cost [U][F], packed gradient [U][F][2 (C-1)]) fp64"""
        import torch
        a = self._args(X, nframes, sFrame, eFrame, R, fbinX); w = self._wa(wa, X); U = X.shape[0]
        cost = torch.zeros((U, self.F), dtype=torch.float64, device=X.device)
        grad = torch.zeros((U, self.F, 2 * (self.C - 1)), dtype=torch.float64, device=X.device)
        check(_lib.dsr_mk_eval(self.h, *a, _dev(torch.view_as_real(w)), _dev(stats) if stats is not None else None, _dev(cost), _dev(grad), cur_stream()))
        return cost, grad

    def estimate(self, X, wa=None, nframes=None, sFrame=0, eFrame=None, R=1, stats=None, fbinX=-1):
        """-> (wa [U][F][C-1] complex128, info [U][F][4] int32: iterations, evaluations, failed trials, exit reason, final cost [U][F]).  wa: the
        starting point (None: zero).  stats (cuda fp64 [3][U][F]: prevAvgY2, prevAvgY4, prevFrameN) is read, and for MK_NRM updated in place."""
        import torch
        a = self._args(X, nframes, sFrame, eFrame, R, fbinX); w = self._wa(wa, X); U = X.shape[0]
        info = torch.zeros((U, self.F, 4), dtype=torch.int32, device=X.device)
        cost = torch.zeros((U, self.F), dtype=torch.float64, device=X.device)
        check(_lib.dsr_mk_estimate(self.h, *a, _dev(torch.view_as_real(w)), _dev(stats) if stats is not None else None, _dev(info), _dev(cost), cur_stream()))
        return w, info, cost

    def apply(self, X, wa):
        """Y [U][T][F] = (wq - B wa[u][f])^H X, per-utterance active weights"""
        import torch
        U, Cn, T, F = X.shape
        w = self._wa(wa, X)
        Y = torch.empty((U, T, F, 2), dtype=torch.float32, device=X.device)
        check(_lib.dsr_mk_apply(self.h, _dev(torch.view_as_real(X.contiguous())), U, T, _dev(torch.view_as_real(w)), _dev(Y), cur_stream()))
        return torch.view_as_complex(Y)


def zelinski_path(kind, chanN, bf=None):
    """-> (cell, template argument): the kernels a post-filter of that kind (0 Zelinski, 1 McCowan, 2 Lefkimmiatis) launches, behind the beamformer bf
    (apply_bf) or on its own (apply); PF_*; follows DSR_PF_SUM / DSR_PF_NOFUSE / DSR_PF_WAVE / DSR_PF_MEMSTATE; needs no device"""
    L = load()
    out = (C.c_int * 2)()
    check(L.dsr_zelinski_path(int(kind), int(chanN), bf.h if bf is not None else None, out))
    return tuple(out)


class ZelinskiPostFilter:
    kind = 0
    """Zelinski post-filter (postfilter.cc:8-221,350-493); manifold [M/2+1][C] complex = arrayManifold() (or wq() with type | 8)."""

    def __init__(self, fftLen, chanN, manifold, alpha=0.6, type=2, minFrames=0):
        L = load(); self.h = vp(); self.M, self.C = fftLen, chanN
        check(L.dsr_zelinski_create(fftLen, chanN, alpha, type, minFrames, C.byref(self.h)))
        m = np.ascontiguousarray(manifold, np.complex128)
        for f in range(fftLen // 2 + 1):
            check(L.dsr_zelinski_set_manifold(self.h, f, _ptr(m[f])))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_zelinski_destroy(self.h)

    def apply(self, X, Y, nframes=None, want_weights=False):
        """X: cuda complex64 [U][C][T][F], Y: [U][T][F] -> out [U][T][F] (and the weights [U][T][F] fp32)"""
        import torch
        U, Cn, T, F = X.shape
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=X.device)
        out = torch.zeros((U, T, F), dtype=torch.complex64, device=X.device)
        w = torch.zeros((U, T, F), dtype=torch.float32, device=X.device) if want_weights else None
        check(_lib.dsr_zelinski_apply(self.h, _dev(X.contiguous()), _dev(Y.contiguous()), _dev(nframes), U, T, _dev(out), _dev(w) if want_weights else None, cur_stream()))
        return (out, w) if want_weights else out

    def apply_bf(self, bf, X, nframes=None, want_weights=False, want_bf_output=False):
        """The post-filter behind its beamformer (setBeamformer, postfilter.cc:376): out = postfilter(X, bf(X)); the beamformer's sum is formed in the filter's own
        pass over the snapshots where it streams them.  X: cuda complex64 [U][C][T][F] -> out [U][T][F] (+ the weights, + bf(X))"""
        import torch
        U, Cn, T, F = X.shape
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=X.device)
        out = torch.zeros((U, T, F), dtype=torch.complex64, device=X.device)
        w = torch.zeros((U, T, F), dtype=torch.float32, device=X.device) if want_weights else None
        Y = torch.zeros((U, T, F), dtype=torch.complex64, device=X.device) if want_bf_output else None
        check(_lib.dsr_zelinski_apply_bf(self.h, bf.h, _dev(X.contiguous()), _dev(nframes), U, T, _dev(out), _dev(w) if want_weights else None,
                                         _dev(Y) if want_bf_output else None, cur_stream()))
        r = (out,) + ((w,) if want_weights else ()) + ((Y,) if want_bf_output else ())
        return r if len(r) > 1 else out

    def carry(self, on=True):
        """keep the spectral densities from call to call (block streaming)"""
        check(_lib.dsr_zelinski_carry(self.h, int(bool(on))))

    def resetState(self):
        check(_lib.dsr_zelinski_reset_state(self.h))

    def path(self, bf=None):
        """zelinski_path of this filter: what apply (bf None) / apply_bf(bf) launches"""
        return zelinski_path(self.kind, self.C, bf)


def _nf(nframes):
    return _dev(nframes) if nframes is not None else None


def _state(nbytes, device):
    import torch
    return torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=device)


class SpectralSubtractor:
    """SpectralSubtractor with its averagePSDEstimators (spectralsubtraction.cc:52-267) over dsr_specsub_* (include/dsr.h 6a-2).  The noise
    estimates are a device buffer of the caller (newState), as with Gcc."""

    def __init__(self, fftLen, halfBandShift=False, ft=1.0, flooringV=0.001):
        L = load(); self.h = vp(); self.M = int(fftLen); self.F = self.M // 2 + 1
        check(L.dsr_specsub_create(self.M, int(bool(halfBandShift)), float(ft), float(flooringV), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_specsub_destroy(self.h)

    def setChannel(self, alpha=-1.0):
        check(_lib.dsr_specsub_set_channel(self.h, float(alpha)))

    def chanN(self):
        return int(_lib.dsr_specsub_chan_n(self.h))

    def newState(self, U, device="cuda:0"):
        st = _state(_lib.dsr_specsub_state_bytes(self.h, int(U)), device); st.U = int(U)
        check(_lib.dsr_specsub_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def setNoiseOverEstimationFactor(self, ft):
        check(_lib.dsr_specsub_set_noise_over_estimation_factor(self.h, float(ft)))

    def startTraining(self):
        check(_lib.dsr_specsub_start_training(self.h))

    def stopTraining(self, state=None):
        check(_lib.dsr_specsub_stop_training(self.h, _dev(state) if state is not None else None, state.U if state is not None else 0, cur_stream() if state is not None else None))

    def startNoiseSubtraction(self):
        check(_lib.dsr_specsub_set_noise_subtraction(self.h, 1))

    def stopNoiseSubtraction(self):
        check(_lib.dsr_specsub_set_noise_subtraction(self.h, 0))

    def clear(self, state):
        check(_lib.dsr_specsub_clear(self.h, _dev(state), state.U, cur_stream()))

    def clearNoiseSamples(self, state):
        check(_lib.dsr_specsub_clear_noise_samples(self.h, _dev(state), state.U, cur_stream()))

    def readNoiseFile(self, fn, state, idx=0):
        check(_lib.dsr_specsub_read_noise_file(self.h, str(fn).encode(), int(idx), _dev(state), state.U)); return True

    def writeNoiseFile(self, fn, state, idx=0, u=0):
        check(_lib.dsr_specsub_write_noise_file(self.h, str(fn).encode(), int(idx), _dev(state), state.U, int(u))); return True

    def apply(self, X, state, nframes=None, full=False, train_only=False):
        """X cuda complex64 [U][C][T][F] -> [U][T][F] complex64 ([U][T][fftLen] with full); train_only: addSample alone, no output"""
        import torch
        U, Cn, T, F = X.shape
        if Cn != self.chanN() or F != self.F or X.dtype != torch.complex64:
            raise ValueError("X: complex64 [U][%d][T][%d] expected" % (self.chanN(), self.F))
        nb = self.M if full else self.F
        out = None if train_only else torch.zeros((U, T, nb), dtype=torch.complex64, device=X.device)
        check(_lib.dsr_specsub_apply(self.h, _dev(X.contiguous()), _nf(nframes), U, T, _dev(out) if out is not None else None, nb, 0, _dev(state), cur_stream()))
        return out

    def read(self, state, what, u, chan):
        out = np.zeros(2 if what == 2 else self.F); check(_lib.dsr_specsub_state_read(self.h, _dev(state), state.U, int(what), int(u), int(chan), _ptr(out), out.size))
        return out


class WienerFilter:
    """WienerFilter (spectralsubtraction.cc:269-347) over dsr_wiener_*"""

    def __init__(self, fftLen, halfBandShift=False, alpha=0.0, flooringV=0.001, beta=1.0, noiseLen=None):
        L = load(); self.h = vp(); self.M = int(fftLen); self.F = self.M // 2 + 1
        check(L.dsr_wiener_create(self.M, int(self.M if noiseLen is None else noiseLen), int(bool(halfBandShift)), float(alpha), float(flooringV), float(beta), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_wiener_destroy(self.h)

    def setNoiseAmplificationFactor(self, beta):
        check(_lib.dsr_wiener_set_noise_amplification_factor(self.h, float(beta)))

    def startUpdatingNoisePSD(self):
        check(_lib.dsr_wiener_set_updating_noise_psd(self.h, 1))

    def stopUpdatingNoisePSD(self):
        check(_lib.dsr_wiener_set_updating_noise_psd(self.h, 0))

    def carry(self, on=True):
        check(_lib.dsr_wiener_carry(self.h, int(bool(on))))

    def newState(self, U, device="cuda:0"):
        st = _state(_lib.dsr_wiener_state_bytes(self.h, int(U)), device); st.U = int(U)
        check(_lib.dsr_wiener_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def resetState(self, state):
        check(_lib.dsr_wiener_reset_state(self.h, _dev(state), state.U, cur_stream()))

    def apply(self, S, N, state, nframes=None, full=False):
        """S, N cuda complex64 [U][T][F] -> [U][T][F] (or [U][T][fftLen])"""
        import torch
        U, T, F = S.shape; nb = self.M if full else self.F
        out = torch.zeros((U, T, nb), dtype=torch.complex64, device=S.device)
        check(_lib.dsr_wiener_apply(self.h, _dev(S.contiguous()), _dev(N.contiguous()) if N is not None else None, _nf(nframes), U, T, _dev(out), nb, 0, _dev(state), cur_stream()))
        return out

    def read(self, state, what, u):
        out = np.zeros(1 if what == 2 else self.F); check(_lib.dsr_wiener_state_read(self.h, _dev(state), state.U, int(what), int(u), _ptr(out), out.size)); return out


class BinaryMask:
    """BinaryMaskFilter ("base"), KimBinaryMaskFilter ("kim"), IIDBinaryMaskFilter ("iid") (binauralprocessing.cc:47-211, 431-520) over dsr_binmask_*"""
    KINDS = {"base": 0, "kim": 1, "iid": 2}

    def __init__(self, kind, chanX, fftLen, threshold, alpha, dEta=0.01, dPowerCoeff=0.0):
        L = load(); self.h = vp(); self.M = int(fftLen); self.F = self.M // 2 + 1; self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        check(L.dsr_binmask_create(self.kind, int(chanX), self.M, float(threshold), float(alpha), float(dEta), float(dPowerCoeff), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_binmask_destroy(self.h)

    def setThreshold(self, threshold):
        check(_lib.dsr_binmask_set_threshold(self.h, float(threshold)))

    def getThreshold(self):
        return float(_lib.dsr_binmask_threshold(self.h))

    def setThresholds(self, thresholds):
        t = _np(thresholds, np.float64); check(_lib.dsr_binmask_set_thresholds(self.h, _ptr(t), t.size))

    def getThresholds(self):
        out = np.zeros(self.F); ex = C.c_int32(0); check(_lib.dsr_binmask_thresholds(self.h, _ptr(out), out.size, C.byref(ex)))
        return out if ex.value else None

    def carry(self, on=True):
        check(_lib.dsr_binmask_carry(self.h, int(bool(on))))

    def newState(self, U, device="cuda:0"):
        import torch
        st = torch.zeros((int(U), self.F), dtype=torch.float32, device=device); st.U = int(U)
        check(_lib.dsr_binmask_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def resetState(self, state):
        check(_lib.dsr_binmask_reset_state(self.h, _dev(state), state.U, cur_stream()))

    def apply(self, L, R, state, nframes=None, full=False, want_mu=False, want_itd=False):
        """L, R cuda complex64 [U][T][F] -> dict(out [U][T][F] or [U][T][fftLen], mu float32 [U][T][F], itd float64 [U][T][F])"""
        import torch
        U, T, F = L.shape; nb = self.M if full else self.F; dev = L.device
        r = dict(out=torch.zeros((U, T, nb), dtype=torch.complex64, device=dev), mu=torch.zeros((U, T, F), dtype=torch.float32, device=dev) if want_mu else None,
                 itd=torch.zeros((U, T, F), dtype=torch.float64, device=dev) if want_itd else None)
        check(_lib.dsr_binmask_apply(self.h, _dev(L.contiguous()), _dev(R.contiguous()), _nf(nframes), U, T, _dev(r["out"]), nb, 0,
                                     _dev(r["mu"]) if want_mu else None, _dev(r["itd"]) if want_itd else None, _dev(state), cur_stream()))
        return r

    def read(self, state, u):
        out = np.zeros(self.F, np.float32); check(_lib.dsr_binmask_state_read(self.h, _dev(state), state.U, int(u), _ptr(out), out.size)); return out


class ThresholdEstimator:
    """KimITDThresholdEstimator ("kim"), IIDThresholdEstimator ("iid"), FDIIDThresholdEstimator ("fdiid") (binauralprocessing.cc:232-426, 525-683,
    702-928) over dsr_thest_*: run() adds to the caller's accumulators (newState), calcThreshold() finalises one utterance's on the host."""
    KINDS = {"kim": 0, "iid": 1, "fdiid": 2}

    def __init__(self, kind, fftLen, minThreshold=0.0, maxThreshold=0.0, width=0.02, minFreq=-1.0, maxFreq=-1.0, sampleRate=-1, dEta=0.01, dPowerCoeff=0.0):
        L = load(); self.h = vp(); self.M = int(fftLen); self.F = self.M // 2 + 1; self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind)
        check(L.dsr_thest_create(self.kind, self.M, float(minThreshold), float(maxThreshold), float(width), float(minFreq), float(maxFreq), int(sampleRate),
                                 float(dEta), float(dPowerCoeff), C.byref(self.h)))
        self.nCand = int(L.dsr_thest_n_cand(self.h)); self.nLoop = int(L.dsr_thest_n_loop(self.h)); self.accDoubles = int(L.dsr_thest_acc_doubles(self.h))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_thest_destroy(self.h)

    def candidates(self):
        out = np.zeros(self.nLoop, np.float32); check(_lib.dsr_thest_candidates(self.h, _ptr(out), out.size)); return out

    def binRange(self):
        out = np.zeros(2, np.int32); check(_lib.dsr_thest_bin_range(self.h, _ptr(out))); return int(out[0]), int(out[1])

    def newState(self, U, device="cuda:0"):
        st = _state(_lib.dsr_thest_state_bytes(self.h, int(U)), device); st.U = int(U)
        check(_lib.dsr_thest_state_init(self.h, _dev(st), int(U), cur_stream())); return st

    def resetState(self, state):
        check(_lib.dsr_thest_reset_state(self.h, _dev(state), state.U, cur_stream()))

    def run(self, L, R, state, nframes=None):
        U, T, F = L.shape
        check(_lib.dsr_thest_run(self.h, _dev(L.contiguous()), _dev(R.contiguous()), _nf(nframes), U, T, _dev(state), cur_stream()))

    def read(self, state, u):
        out = np.zeros(self.accDoubles); check(_lib.dsr_thest_state_read(self.h, _dev(state), state.U, int(u), _ptr(out), out.size)); return out

    def calcThreshold(self, acc, inPlace=False):
        """-> dict(threshold, index, cost [nCand] or [F][nCand], thresholds [F] (FDIID)) from one utterance's accumulators (numpy, host side)"""
        a = acc if inPlace else _np(acc, np.float64).copy()
        th = C.c_double(0.0); ix = C.c_int32(0); cost = np.zeros((self.F, self.nCand) if self.kind == 2 else self.nCand); ths = np.zeros(self.F)
        check(_lib.dsr_thest_calc_threshold(self.h, _ptr(a), a.size, int(bool(inPlace)), C.byref(th), C.byref(ix), _ptr(cost), cost.size, _ptr(ths), ths.size))
        return dict(threshold=th.value, index=ix.value, cost=cost, thresholds=ths if self.kind == 2 else None)


def psdFileWrite(fn, est):
    e = _np(est, np.float64); load(); check(_lib.dsr_psd_file_write(str(fn).encode(), _ptr(e), e.size))


def psdFileRead(fn, n):
    out = np.zeros(int(n)); load(); check(_lib.dsr_psd_file_read(str(fn).encode(), _ptr(out), out.size)); return out


class SubbandMMI:
    """SubbandMMI (beamformer.h:264-312, beamformer.cc:1753-2319) over dsr_mmi_*; the reference's method names."""

    def __init__(self, fftLen=512, chanN=2, halfBandShift=False, targetSourceX=0, nSource=2, pfType=0, alpha=0.9):
        L = load(); self.h = vp(); self.M, self.C, self.nSource, self.NC = fftLen, chanN, nSource, 1
        check(L.dsr_mmi_create(fftLen, chanN, int(bool(halfBandShift)), targetSourceX, nSource, pfType, alpha, C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_mmi_destroy(self.h)

    def bins(self):
        return _lib.dsr_mmi_bins(self.h)

    def outBins(self):
        """bins per output frame: bins(), or fftLen with the APAB post-filter (whose frames are not conjugate-symmetric)"""
        return _lib.dsr_mmi_out_bins(self.h)

    def useBinaryMask(self, avgFactor=-1.0, fwidth=1, type=0):
        check(_lib.dsr_mmi_use_binary_mask(self.h, avgFactor, fwidth, type))

    def calcWeights(self, sampleRate, delays):
        d = np.ascontiguousarray(delays, np.float64)
        if d.shape != (self.nSource, self.C):
            raise DsrError(5, "delays must be [%d][%d]" % (self.nSource, self.C))
        check(_lib.dsr_mmi_calc_weights(self.h, sampleRate, _ptr(d))); self.NC = 1

    def calcWeightsN(self, sampleRate, delays, NC=2):
        d = np.ascontiguousarray(delays, np.float64)
        if d.shape != (self.nSource, self.C):
            raise DsrError(5, "delays must be [%d][%d]" % (self.nSource, self.C))
        check(_lib.dsr_mmi_calc_weights_n(self.h, sampleRate, _ptr(d), NC)); self.NC = NC

    def setActiveWeights_f(self, fbinX, packedWeights, option=0):
        w = np.ascontiguousarray(packedWeights, np.float64)
        if w.ndim != 2:
            raise DsrError(5, "packedWeights must be a matrix")
        check(_lib.dsr_mmi_set_active_weights_f(self.h, fbinX, _ptr(w), w.shape[0], w.shape[1], option))

    def setHiActiveWeights_f(self, fbinX, pkdWa, pkdwb, option=0):
        a = np.ascontiguousarray(pkdWa, np.float64).ravel(); b = np.ascontiguousarray(pkdwb, np.float64).ravel()
        check(_lib.dsr_mmi_set_hi_active_weights_f(self.h, fbinX, _ptr(a), a.size, _ptr(b), b.size, option))

    def get(self, srcX, kind):
        """kind: 'wq' [M][C], 'wl' [M][C], 'B' [M][C][C-NC], 'ta' [M][C], 'wa' [M][C-NC] (complex128)"""
        k = {"wq": 0, "wl": 1, "B": 2, "ta": 3, "wa": 4}[kind]; bs = self.C - self.NC
        shape = {0: (self.M, self.C), 1: (self.M, self.C), 2: (self.M, self.C, bs), 3: (self.M, self.C), 4: (self.M, bs)}[k]
        out = np.zeros(shape, np.complex128)
        check(_lib.dsr_mmi_get(self.h, srcX, k, _ptr(out), 2 * out.size))
        return out

    def apply(self, X, nframes=None):
        """X: cuda complex64 [U][C][T][bins] -> [U][T][outBins]"""
        import torch
        U, Cn, T, F = X.shape
        if Cn != self.C or F != self.bins():
            raise DsrError(5, "snapshots must be [U][%d][T][%d]" % (self.C, self.bins()))
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=X.device)
        out = torch.zeros((U, T, self.outBins()), dtype=torch.complex64, device=X.device)
        check(_lib.dsr_mmi_apply(self.h, _dev(X.contiguous()), _dev(nframes), U, T, _dev(out), cur_stream()))
        return out


class McCowanPostFilter(ZelinskiPostFilter):
    """McCowan post-filter (postfilter.cc:502-945): Zelinski's recursions + a noise coherence matrix per bin."""
    kind = 1

    def __init__(self, fftLen, chanN, manifold, alpha=0.6, type=2, minFrames=0, threshold=0.99):
        L = load(); self.h = vp(); self.M, self.C = fftLen, chanN
        check(L.dsr_mccowan_create(fftLen, chanN, alpha, type, minFrames, threshold, C.byref(self.h)))
        m = np.ascontiguousarray(manifold, np.complex128)
        for f in range(fftLen // 2 + 1):
            check(L.dsr_zelinski_set_manifold(self.h, f, _ptr(m[f])))

    def setDiffuseNoiseModel(self, micPositions, sampleRate, sspeed=343740.0):
        mp = _np(micPositions, np.float64); check(_lib.dsr_mccowan_set_diffuse_noise_model(self.h, _ptr(mp), sampleRate, sspeed)); return True

    def setNoiseSpatialSpectralMatrix(self, fbinX, Rnn):
        r = np.ascontiguousarray(Rnn, np.complex128); check(_lib.dsr_mccowan_set_noise_matrix(self.h, fbinX, _ptr(r))); return True

    def setAllLevelsOfDiagonalLoading(self, w):
        check(_lib.dsr_mccowan_diagonal_loading(self.h, -1, w))

    def setLevelOfDiagonalLoading(self, fbinX, w):
        check(_lib.dsr_mccowan_diagonal_loading(self.h, fbinX, w))

    def divideAllNonDiagonalElements(self, myu):
        check(_lib.dsr_mccowan_divide_nondiagonal(self.h, myu))


class LefkimmiatisPostFilter(McCowanPostFilter):
    """Lefkimmiatis post-filter (postfilter.cc:948-1210): McCowan's clean-signal estimate against the coherence-based noise estimate,
    divided by d^H pinv(R) d from bin fbinX1 on."""
    kind = 2

    def __init__(self, fftLen, chanN, manifold, minSV=1e-8, fbinX1=0, alpha=0.6, type=2, minFrames=0, threshold=0.99):
        L = load(); self.h = vp(); self.M, self.C = fftLen, chanN
        check(L.dsr_lefkimmiatis_create(fftLen, chanN, minSV, fbinX1, alpha, type, minFrames, threshold, C.byref(self.h)))
        m = np.ascontiguousarray(manifold, np.complex128)
        for f in range(fftLen // 2 + 1):
            check(L.dsr_zelinski_set_manifold(self.h, f, _ptr(m[f])))


class LpcEnvelope:
    """WarpMVDR/BurgMVDR (kind 0) and WarpLPC/BurgLPC (kind 1) envelopes of windowed frames, lpc.h:134-195,291-331."""

    def __init__(self, dim, order=60, warp=0.0, method=0, kind=0, correlate=0):
        L = load(); self.h = vp(); self.dim = dim
        check(L.dsr_lpc_create(dim, order, correlate, warp, method, kind, C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_lpc_destroy(self.h)

    def run(self, frames):
        """frames: cuda float32 [T][dim] -> float64 [T][dim/2+1]"""
        import torch
        T, dim = frames.shape
        assert dim == self.dim
        out = torch.zeros((T, dim // 2 + 1), dtype=torch.float64, device=frames.device)
        check(_lib.dsr_lpc_run(self.h, _dev(frames), T, _dev(out), cur_stream()))
        return out


class WtMvdrEnvelope:
    """WarpedTwiceMVDRFeature envelopes of windowed frames, lpc.h:205-246, lpc.cc:212-468."""

    def __init__(self, dim, order=60, correlate=0, warp=0.0, warp_factor_fixed=False, sensibility=0.1):
        L = load(); self.h = vp(); self.dim = dim
        check(L.dsr_wtmvdr_create(dim, order, correlate, warp, int(bool(warp_factor_fixed)), sensibility, C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_wtmvdr_destroy(self.h)

    def run(self, frames, warps=None, want_pa=False):
        """frames: cuda float32 [T][dim], warps: cuda float32 [T] (each frame's first-stage warp) or None -> float64 [T][dim/2+1];
        with want_pa also PA float32 [T][dim+1] and rewarp float32 [T]"""
        import torch
        T, dim = frames.shape
        assert dim == self.dim and frames.dtype == torch.float32 and frames.is_contiguous()
        assert warps is None or (warps.dtype == torch.float32 and warps.numel() == T and warps.is_contiguous())
        out = torch.zeros((T, dim // 2 + 1), dtype=torch.float64, device=frames.device)
        pa = torch.zeros((T, dim + 1), dtype=torch.float32, device=frames.device) if want_pa else None
        rw = torch.zeros((T,), dtype=torch.float32, device=frames.device) if want_pa else None
        check(_lib.dsr_wtmvdr_run(self.h, _dev(frames), _dev(warps) if warps is not None else None, T, _dev(out),
                                  _dev(pa) if want_pa else None, _dev(rw) if want_pa else None, cur_stream()))
        return (out, pa, rw) if want_pa else out


def spectral_smoothing(to, frm):
    """SpectralSmoothing::next on a batch (lpc.cc:485-529): to, frm cuda float64 [T][size] -> float64 [T][size]"""
    import torch
    load()
    if tuple(to.shape) != tuple(frm.shape):
        raise DsrError(E_DIMENSION, "Feature sizes (%d vs. %d) do not match." % (to.shape[-1], frm.shape[-1]))
    assert to.dtype == torch.float64 and frm.dtype == torch.float64 and to.is_contiguous() and frm.is_contiguous()
    T, size = to.shape
    out = torch.zeros_like(to)
    check(_lib.dsr_specsmooth_run(_dev(to), _dev(frm), T, size, _dev(out), cur_stream()))
    return out


class BlockConvolver:
    """OverlapAdd / OverlapSave of btk/convolution on batches (include/dsr.h section 2g): kind "add" or "save", blocks of L samples, C impulse
    responses [C][P] (one source gives C output channels).  OverlapAdd's fp32 buffer is a device tensor of the caller (state) that apply()
    continues from and leaves behind."""
    KINDS = {"add": 0, "save": 1}

    def __init__(self, kind, L, response, fftLen=0):
        L_ = load(); self.h = vp()
        if response is None:
            raise DsrError(E_PARAMETER, "null impulse response")
        h = np.ascontiguousarray(np.atleast_2d(np.asarray(response, dtype=np.float64)))
        self.kind = self.KINDS[kind] if isinstance(kind, str) else int(kind); self.L = int(L); self.C, self.P = h.shape
        check(L_.dsr_conv_create(self.kind, self.L, self.P, int(fftLen), self.C, C.byref(self.h)))
        check(L_.dsr_conv_set_response(self.h, _ptr(h)))
        self.size = int(L_.dsr_conv_size(self.h)); self.fftLen = int(L_.dsr_conv_fft_len(self.h))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_conv_destroy(self.h)

    def update(self, delta, c=0):
        """OverlapSave::update: delta complex [L], its bins 0..L/2 are added to response c's spectrum"""
        d = np.ascontiguousarray(np.asarray(delta, dtype=np.complex128).reshape(-1))
        if d.size != self.L:
            raise DsrError(E_DIMENSION, "Dimension of udpate vector (%d) does not match frequency response (%d)." % (d.size, self.L))
        check(_lib.dsr_conv_update(self.h, int(c), _ptr(d)))

    def state(self, U, device="cuda:0"):
        import torch
        st = torch.zeros(max(1, int(_lib.dsr_conv_state_bytes(self.h, int(U))) // 4), dtype=torch.float32, device=device)
        check(_lib.dsr_conv_state_init(self.h, _dev(st), int(U), cur_stream()))
        return st

    def apply(self, x, state=None, nframes=None):
        """x: cuda float32 [U][Tmax][L], nframes: cuda int32 [U] or None, state: from state(U) (OverlapAdd; None starts from zeros and drops
        what is left) -> float32 [U][C][Tmax][size]"""
        import torch
        U, T, L = x.shape
        assert L == self.L and x.dtype == torch.float32 and x.is_contiguous()
        assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
        if self.kind == 0 and state is None:
            state = self.state(U, x.device)
        y = torch.zeros((U, self.C, T, self.size), dtype=torch.float32, device=x.device)
        check(_lib.dsr_conv_apply(self.h, _dev(x), _dev(nframes) if nframes is not None else None, U, T, _dev(state) if state is not None else None,
                                  _dev(y), cur_stream()))
        return y

    def set_timing(self, on=True):
        check(_lib.dsr_conv_set_timing(self.h, int(bool(on))))

    def kernel_ms(self):
        """ms of the last apply() in the transform kernel and in the fold"""
        two = (C.c_double * 2)(); check(_lib.dsr_conv_kernel_ms(self.h, two))
        return tuple(two)


def fir_frames(x, coeffA, nframes=None):
    """FilterFeature over whole utterances (feature.cc:3206-3313): x cuda float32 [U][Tmax][dim], coeffA odd-length taps, nframes cuda int32 [U] or
    None -> float32 [U][Tmax + (lenA == 1)][dim]; utterance u has fir_frames_count(nframes[u], lenA) frames, the rest are zero"""
    import torch
    load()
    a = np.ascontiguousarray(np.asarray(coeffA, dtype=np.float64).reshape(-1))
    U, T, dim = x.shape
    assert x.dtype == torch.float32 and x.is_contiguous()
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    y = torch.zeros((U, T + (1 if a.size == 1 else 0), dim), dtype=torch.float32, device=x.device)
    check(_lib.dsr_fir_frames_run(_dev(x), _dev(nframes) if nframes is not None else None, _ptr(a), int(a.size), U, T, dim, _dev(y), cur_stream()))
    return y


def fir_frames_count(T, lenA):
    return int(load().dsr_fir_frames_count(int(T), int(lenA)))


# ---- the scalar feature operators of btk/feature (include/dsr.h section 6c, csrc/k_featops.hip)
def _batch(x, nframes, dtype=None):
    import torch
    assert x.dim() == 3 and x.dtype == (dtype or torch.float32) and x.is_contiguous()
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == x.shape[0] and nframes.is_contiguous())
    return x.shape, (_dev(nframes) if nframes is not None else None)


def signal_power(x, nframes=None):
    """SignalPowerFeature over whole utterances: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1]"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_lib.dsr_signal_power_run(_dev(x), nf, U, T, dim, _dev(y), cur_stream()))
    return y


def zero_crossing_rate(x, nframes=None):
    """ZeroCrossingRateHammingFeature: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1]"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_lib.dsr_zcr_hamming_run(_dev(x), nf, U, T, dim, _dev(y), cur_stream()))
    return y


def yin_pitch(x, samplerate=16000, threshold=0.5, nframes=None, return_value=False, return_chunks=False):
    """YINPitchFeature: x cuda float32 [U][Tmax][dim] -> pitch float32 [U][Tmax][1]; return_value adds float32 [U][Tmax], y(tau) at the lag where
    the reference's search returned (y(W-1) where it ran to the end); return_chunks adds int32 [U][Tmax], the chunks of 64 lags evaluated"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    p = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    v = torch.zeros((U, T), dtype=torch.float32, device=x.device) if return_value else None
    c = torch.zeros((U, T), dtype=torch.int32, device=x.device) if return_chunks else None
    check(_lib.dsr_yin_pitch_run(_dev(x), nf, U, T, dim, int(samplerate), float(threshold), _dev(p), _dev(v) if return_value else None,
                                 _dev(c) if return_chunks else None, cur_stream()))
    out = (p,) + ((v,) if return_value else ()) + ((c,) if return_chunks else ())
    return out if len(out) > 1 else p


def yin_kernel(dim):
    """frames a workgroup of the YIN kernel a frame length selects (the frame's copies in LDS), 0: the kernel that reads global memory"""
    return int(load().dsr_yin_kernel(int(dim)))


def spike_filter(x, tapN=3, nframes=None):
    """SpikeFilter: the running median of tapN samples within each block; the last tapN-1 samples of a block stay zero as in the reference"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_lib.dsr_spike_filter_run(_dev(x), nf, U, T, dim, int(tapN), _dev(y), cur_stream()))
    return y


def spike_filter2_state(U, startslope=100.0, device="cuda:0"):
    """(meanslope float32 [U], count int32 [U]) as SpikeFilter2::reset() leaves them"""
    import torch
    return torch.full((U,), float(startslope), dtype=torch.float32, device=device), torch.zeros((U,), dtype=torch.int32, device=device)


def spike_filter2(x, width=3, maxslope=7000.0, startslope=100.0, thresh=15.0, alpha=0.2, state=None, nframes=None):
    """SpikeFilter2 over the blocks of each utterance in order: x cuda float32 [U][Tmax][dim] -> (y, (meanslope, count)); state: the pair a
    previous call returned (None: reset())"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    if state is None:
        state = spike_filter2_state(U, startslope, x.device)
    ms, cnt = state
    assert ms.dtype == torch.float32 and cnt.dtype == torch.int32 and ms.numel() == U and cnt.numel() == U
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_lib.dsr_spike_filter2_run(_dev(x), nf, U, T, dim, int(width), float(maxslope), float(thresh), float(alpha), _dev(ms), _dev(cnt), _dev(y), cur_stream()))
    return y, (ms, cnt)


def minmax_state(U, device="cuda:0"):
    """(min, max) of ALog / Normalize after nextSpeaker(): float64 [U][2] = (HUGE, -HUGE)"""
    import torch
    load(); st = torch.zeros((U, 2), dtype=torch.float64, device=device)
    check(_lib.dsr_minmax_state_init(_dev(st), U, cur_stream()))
    return st


def alog(x, m=1.0, a=4.0, runon=False, state=None, nframes=None):
    """ALogFeature: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1].  runon: the running (min, max) continue from state (minmax_state) and
    are left there; otherwise they are taken over the whole utterance"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_lib.dsr_alog_run(_dev(x), nf, U, T, dim, float(m), float(a), int(bool(runon)), _dev(state) if state is not None else None, _dev(y), cur_stream()))
    return y


def normalize(x, min=0.0, max=1.0, runon=False, state=None, nframes=None):
    """NormalizeFeature: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][dim]; runon and state as in alog"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_lib.dsr_normalize_run(_dev(x), nf, U, T, dim, float(min), float(max), int(bool(runon)), _dev(state) if state is not None else None, _dev(y),
                                 cur_stream()))
    return y


def threshold(x, value=0.0, thresh=1.0, mode="upper", nframes=None):
    """ThresholdFeature: mode "upper", "lower" or "both" (any other: a key error)"""
    import torch
    load(); cmp_ = C.c_int(0)
    check(_lib.dsr_threshold_mode(mode.encode() if isinstance(mode, str) else mode, C.byref(cmp_)))
    (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_lib.dsr_threshold_run(_dev(x), nf, U, T, dim, float(value), float(thresh), cmp_.value, _dev(y), cur_stream()))
    return y


def amplify(x, amplify=1.0, nframes=None):
    """AmplificationFeature: float(double(x) * amplify)"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_lib.dsr_amplify_run(_dev(x), nf, U, T, dim, float(amplify), _dev(y), cur_stream()))
    return y


SPECTRAL_SAMPLE_RATIO = 16.0 / 22.05


def spectral_resample(x, ratio=SPECTRAL_SAMPLE_RATIO, len=0, nframes=None):
    """SpectralResamplingFeature: x cuda float64 [U][Tmax][srcN] -> float64 [U][Tmax][len or srcN]"""
    import torch
    load(); (U, T, srcN), nf = _batch(x, nframes, torch.float64)
    outN = C.c_int(0)
    check(_lib.dsr_spectral_resample_size(srcN, float(ratio), int(len), C.byref(outN)))
    y = torch.zeros((U, T, outN.value), dtype=torch.float64, device=x.device)
    check(_lib.dsr_spectral_resample_run(_dev(x), nf, U, T, srcN, float(ratio), int(len), _dev(y), cur_stream()))
    return y


class SphinxMel:
    """SphinxMelFeature's filter bank: .filters is the host-built [filterN][powerN] fp64 matrix, apply() multiplies frames by it"""

    def __init__(self, fftN=512, powerN=257, sampleRate=16000.0, lowerF=0.0, upperF=0.0, filterN=30):
        L_ = load(); self.h = vp()
        check(L_.dsr_sphinx_mel_create(int(fftN), int(powerN), float(sampleRate), float(lowerF), float(upperF), int(filterN), C.byref(self.h)))
        self.powerN, self.filterN = int(powerN), int(filterN)
        self.filters = np.zeros((self.filterN, self.powerN), np.float64)
        check(L_.dsr_sphinx_mel_filters(self.h, _ptr(self.filters)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_sphinx_mel_destroy(self.h)

    def apply(self, x, nframes=None):
        """x cuda float64 [U][Tmax][powerN] -> float64 [U][Tmax][filterN]"""
        import torch
        (U, T, dim), nf = _batch(x, nframes, torch.float64)
        assert dim == self.powerN
        y = torch.zeros((U, T, self.filterN), dtype=torch.float64, device=x.device)
        check(_lib.dsr_sphinx_mel_apply(self.h, _dev(x), nf, U, T, _dev(y), cur_stream()))
        return y


MFCC_FRAMES_PLAIN, MFCC_FRAMES_W = 0, 1
MFCC_CMN_NONE, MFCC_CMN_PLAIN, MFCC_CMN_LDS = 0, 1, 2
MFCC_LDA_TOO_LARGE, MFCC_LDA_SPLICE, MFCC_LDA_PLAIN, MFCC_LDA_B = -1, 0, 1, 2


def mfcc_cfg_paths(Tmax, **kw):
    """-> ((frames, cmn, lda), dict of the LDS bytes the gates compare) for the configuration Mfcc(**kw) would have; needs no device"""
    L = load()
    cfg = MfccCfg(); L.dsr_mfcc_default_cfg(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    out = (C.c_int * 3)(); lds = (C.c_int64 * 4)()
    check(L.dsr_mfcc_cfg_paths(C.byref(cfg), int(Tmax), out, lds))
    return tuple(out), dict(zip(("ldsW", "ldsC", "ldsB", "lds2"), lds))


class Mfcc:
    def __init__(self, lda=None, **kw):
        L = load()
        self.cfg = MfccCfg(); L.dsr_mfcc_default_cfg(C.byref(self.cfg))
        for k, v in kw.items():
            setattr(self.cfg, k, v)
        if lda is None and "outDim" not in kw:
            self.cfg.outDim = 0
        a = _np(lda, np.float32) if lda is not None else None
        self.h = vp()
        check(L.dsr_mfcc_create(C.byref(self.cfg), _ptr(a) if a is not None else None, C.byref(self.h)))
        self.outDim = L.dsr_mfcc_out_dim(self.h)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_mfcc_destroy(self.h)

    def frames(self, nsamp):
        return _lib.dsr_mfcc_frames(self.h, int(nsamp))

    def paths(self, Tmax):
        """(frames, cmn, lda) kernels dsr_mfcc_run launches for a batch of Tmax frames: MFCC_FRAMES_*, MFCC_CMN_*, MFCC_LDA_*"""
        out = (C.c_int * 3)()
        check(_lib.dsr_mfcc_paths(self.h, int(Tmax), out))
        return tuple(out)

    def run(self, y, nsamp=None, stage=0):
        """y: cuda float32 [U][N] -> float32 [U][Tmax][dim]"""
        import torch
        U, N = y.shape
        if nsamp is None:
            nsamp = torch.full((U,), N, dtype=torch.int32, device=y.device)
        c = self.cfg
        raw = lambda n: ((n + c.shiftLen - 1) // c.shiftLen) if c.padZeros else max(0, -(-(n - c.blockLen) // c.shiftLen))
        Tmax = max(1, max(raw(int(n)) for n in nsamp.tolist()))
        dim = {0: self.outDim, 1: c.ncep, 2: c.ncep, 3: c.filterN, 4: c.powN}[stage]
        out = torch.zeros((U, Tmax, dim), dtype=torch.float32, device=y.device)
        check(_lib.dsr_mfcc_run(self.h, _dev(y), _dev(nsamp), U, N, Tmax, stage, _dev(out), cur_stream()))
        return out


class Gmm:
    def __init__(self, refN=None, mean=None, ivar=None, det=None, val=None, scale=None, files=None):
        L = load(); self.h = vp()
        if files is not None:
            check(L.dsr_gmm_load(files[0].encode(), files[1].encode(), C.byref(self.h)))
        else:
            r = _np(refN, np.int32); m = _np(mean, np.float32); iv = _np(ivar, np.float32); d = _np(det, np.float32); v = _np(val, np.float32)
            s = _np(scale, np.float32) if scale is not None else None
            check(L.dsr_gmm_create(len(r), m.shape[1], _ptr(r), _ptr(m), _ptr(iv), _ptr(d), _ptr(v), _ptr(s) if s is not None else None, C.byref(self.h)))
        self.K = L.dsr_gmm_num_dists(self.h); self.D = L.dsr_gmm_dim(self.h)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_gmm_destroy(self.h)

    def save(self, cbFile, dsFile):
        check(_lib.dsr_gmm_save(self.h, cbFile.encode(), dsFile.encode()))

    def score(self, x, mode=0, want_argmin=True):
        """x: cuda float32 [N][D] -> (score [N][K] float32, argmin [N][K] uint8)"""
        import torch
        N = x.shape[0]
        sc = torch.empty((N, self.K), dtype=torch.float32, device=x.device)
        am = torch.zeros((N, self.K), dtype=torch.uint8, device=x.device) if want_argmin and mode != 1 else None
        check(_lib.dsr_gmm_score(self.h, _dev(x), N, mode, _dev(sc), _dev(am) if am is not None else None, cur_stream()))
        return sc, am

    @property
    def G(self):
        return _lib.dsr_gmm_num_gaussians(self.h)

    def set_reg_classes(self, classes):
        """one regression class per Gaussian [G], or one class for every Gaussian (CodebookSetBasic::setRegClasses)"""
        if np.isscalar(classes):
            check(_lib.dsr_gmm_set_reg_class_all(self.h, int(classes)))
        else:
            c = _np(classes, np.uint16); assert c.shape == (self.G,)
            check(_lib.dsr_gmm_set_reg_classes(self.h, _ptr(c)))

    def reg_classes(self):
        """the classes [G] (0 where there is none), or None for a model without the table"""
        c = np.zeros(self.G, np.uint16); present = C.c_int(0)
        check(_lib.dsr_gmm_get_reg_classes(self.h, _ptr(c), C.byref(present)))
        return c if present.value else None

    def params(self):
        """the model's host parameters as the training updates left them: refN [K], mean, cv [G][D], det, val, count [G]"""
        r = np.zeros(self.K, np.int32); check(_lib.dsr_gmm_get_params(self.h, _ptr(r), None, None, None, None, None))
        G = int(r.sum())
        d = dict(refN=r, mean=np.zeros((G, self.D), np.float32), cv=np.zeros((G, self.D), np.float32), det=np.zeros(G, np.float32),
                 val=np.zeros(G, np.float32), count=np.zeros(G, np.float32))
        check(_lib.dsr_gmm_get_params(self.h, None, *[_ptr(d[k]) for k in ("mean", "cv", "det", "val", "count")]))
        return d


class Trainer:
    """CodebookSetTrain + DistribSetTrain over one Gmm (asr/train/codebookTrain.cc, distribTrain.cc; include/dsr.h section 9): accumulation on
    the device, updates and accumulator files on the host.  The Gmm is changed by update / split and must outlive the trainer (kept here)."""

    NAMES = ("count", "den", "sumO", "sumOsq", "dcount", "dden")

    def __init__(self, gmm, massThreshold=5.0):
        L = load(); self.h = vp(); self.gmm = gmm
        check(L.dsr_train_create(gmm.h, float(massThreshold), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_train_destroy(self.h)

    @property
    def G(self):
        return _lib.dsr_train_num_gaussians(self.h)

    def zero(self, what=3, nParts=1, part=1):
        check(_lib.dsr_train_zero(self.h, int(what), int(nParts), int(part)))

    def accumulate(self, x, frame, dist, factor, want_score=True):
        """x: cuda float32 [N][D]; frame, dist, factor: host arrays [M] -> float32 scores [M] (or None)"""
        fr = _np(frame, np.int32); ds = _np(dist, np.int32); fa = _np(factor, np.float32); M = len(fr)
        assert len(ds) == M and len(fa) == M and x.dtype.is_floating_point and x.element_size() == 4 and x.is_contiguous() and x.shape[1] == self.gmm.D
        sc = np.zeros(M, np.float32) if want_score else None
        check(_lib.dsr_train_accumulate(self.h, _dev(x), x.shape[0], _ptr(fr), _ptr(ds), _ptr(fa), M, _ptr(sc) if want_score else None, cur_stream()))
        return sc

    def accumulate_path(self, x, distIds, factor=1.0):
        ids = _np(distIds, np.int32); s = C.c_double(0.0)
        assert x.is_contiguous() and x.shape[1] == self.gmm.D and x.shape[0] >= len(ids)
        check(_lib.dsr_train_accumulate_path(self.h, _dev(x), len(ids), _ptr(ids), float(factor), C.byref(s), cur_stream()))
        return s.value

    def accumulate_lattice(self, lattice, x, factor=1.0):
        """lattice: a Lattice (after gammaProbs) -> the number of links accumulated"""
        n = C.c_uint(0); assert x.is_contiguous() and x.shape[1] == self.gmm.D
        check(_lib.dsr_train_accumulate_lattice(self.h, lattice.h, _dev(x), x.shape[0], float(factor), C.byref(n), cur_stream()))
        return n.value

    def get(self):
        G, D = self.G, self.gmm.D
        d = dict(count=np.zeros(G), den=np.zeros(G), sumO=np.zeros((G, D)), sumOsq=np.zeros((G, D)), dcount=np.zeros(G), dden=np.zeros(G))
        check(_lib.dsr_train_get(self.h, *[_ptr(d[k]) for k in self.NAMES]))
        return d

    def set(self, **kw):
        G, D = self.G, self.gmm.D; a = []
        for k in self.NAMES:
            v = kw.get(k)
            if v is not None:
                v = _np(v, np.float64); assert v.shape == ((G, D) if k in ("sumO", "sumOsq") else (G,)), k
            a.append(v)
        check(_lib.dsr_train_set(self.h, *[_ptr(v) if v is not None else None for v in a]))

    def add(self, other, factor=1.0):
        check(_lib.dsr_train_add(self.h, other.h, float(factor)))

    def save_codebook_accus(self, fileName, totalPr=0.0, totalT=0, countsOnly=False):
        check(_lib.dsr_train_save_codebook_accus(self.h, fileName.encode(), float(totalPr), int(totalT), int(countsOnly)))

    def load_codebook_accus(self, fileName, factor=1.0, nParts=1, part=1):
        pr = C.c_float(0.0); tt = C.c_uint(0)
        check(_lib.dsr_train_load_codebook_accus(self.h, fileName.encode(), C.byref(pr), C.byref(tt), float(factor), int(nParts), int(part)))
        return pr.value, tt.value

    def save_distrib_accus(self, fileName):
        check(_lib.dsr_train_save_distrib_accus(self.h, fileName.encode()))

    def load_distrib_accus(self, fileName, factor=1.0, nParts=1, part=1):
        check(_lib.dsr_train_load_distrib_accus(self.h, fileName.encode(), float(factor), int(nParts), int(part)))

    def update(self, what=3, nParts=1, part=1):
        check(_lib.dsr_train_update(self.h, int(what), int(nParts), int(part)))

    def update_mmi(self, what=3, E=1.0, merialdo=False, nParts=1, part=1):
        check(_lib.dsr_train_update_mmi(self.h, int(what), float(E), int(merialdo), int(nParts), int(part)))

    def floor_variances(self, nParts=1, part=1):
        t = C.c_uint(0); f = C.c_uint(0)
        check(_lib.dsr_train_floor_variances(self.h, int(nParts), int(part), C.byref(t), C.byref(f)))
        return t.value, f.value

    def fix_gconsts(self, nParts=1, part=1):
        check(_lib.dsr_train_fix_gconsts(self.h, int(nParts), int(part)))

    def invert_variances(self, nParts=1, part=1):
        check(_lib.dsr_train_invert_variances(self.h, int(nParts), int(part)))

    def split(self, distX, minCount=0.0, splitFactor=0.2):
        r = C.c_uint(0); check(_lib.dsr_train_split(self.h, int(distX), float(minCount), float(splitFactor), C.byref(r)))
        return r.value

    def set_timing(self, on=True):
        check(_lib.dsr_train_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 2)(); check(_lib.dsr_train_kernel_ms(self.h, ms)); return ms[0], ms[1]


def is_ancestor(ancestor, child):
    r = C.c_int(0); load(); check(_lib.dsr_is_ancestor(int(ancestor), int(child), C.byref(r))); return bool(r.value)


class ParamTree:
    """ParamTree of MLLR parameters (asr/adapt/transform.cc:789-950; include/dsr.h section 10).  Host only."""

    def __init__(self, fileName="", handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle; return
        self.h = vp(); check(L.dsr_param_tree_create(fileName.encode(), C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None) and self._owner is None:
            _lib.dsr_param_tree_destroy(self.h)

    def clear(self):
        check(_lib.dsr_param_tree_clear(self.h))

    def read(self, fileName):
        check(_lib.dsr_param_tree_read(self.h, fileName.encode()))

    def write(self, fileName):
        check(_lib.dsr_param_tree_write(self.h, fileName.encode()))

    def copy_from(self, other):
        check(_lib.dsr_param_tree_copy(self.h, other.h))

    def type(self):
        return _lib.dsr_param_tree_type(self.h)

    def hasIndex(self, rc):
        return bool(_lib.dsr_param_tree_has_index(self.h, int(rc)))

    def indices(self):
        n = _lib.dsr_param_tree_indices(self.h, None, 0); a = np.zeros(n, np.uint32)
        _lib.dsr_param_tree_indices(self.h, _ptr(a), n); return [int(x) for x in a]

    def _W(self, rc, size):
        W = np.zeros((size, size + 1)); check(_lib.dsr_param_tree_get(self.h, int(rc), _ptr(W))); return W

    def find(self, rc, useAncestor=True):
        """-> W [size][size + 1] of the class, inserted as a copy of its nearest ancestor when missing"""
        n = C.c_int(0); check(_lib.dsr_param_tree_find(self.h, int(rc), int(useAncestor), 0, C.byref(n))); return self._W(rc, n.value)

    def findMLLR(self, rc, useAncestor=True):
        n = C.c_int(0); check(_lib.dsr_param_tree_find(self.h, int(rc), int(useAncestor), 1, C.byref(n))); return self._W(rc, n.value)

    def set(self, rc, W):
        W = _np(W, np.float64); assert W.ndim == 2 and W.shape[1] == W.shape[0] + 1
        check(_lib.dsr_param_tree_set(self.h, int(rc), W.shape[0], _ptr(W)))


class Mllr:
    """MLLR mean transforms for S speakers at once (csrc/k_mllr.hip; include/dsr.h section 10): statistics on fp64 MFMA, back-off on the host,
    Jacobi solves and the transformed means on the device.  Made from a Gmm with regression classes (Gmm.set_reg_classes or a codebook file
    that carries the table); the handle keeps that model's means as the originals."""

    def __init__(self, gmm, S=1):
        L = load(); self.h = vp(); self.gmm = gmm; self.D = gmm.D; self.G = gmm.G
        check(L.dsr_mllr_create(gmm.h, int(S), C.byref(self.h))); self.S = L.dsr_mllr_num_speakers(self.h)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_mllr_destroy(self.h)

    def set_stats(self, s, trainer=None, c=None, sumO=None):
        """the statistics of slot s: a Trainer (count - denCount and sumO, device to device) or host arrays c [G], sumO [G][D]"""
        if trainer is not None:
            check(_lib.dsr_mllr_set_stats(self.h, int(s), trainer.h)); return
        c = _np(c, np.float64); sumO = _np(sumO, np.float64); assert c.shape == (self.G,) and sumO.shape == (self.G, self.D)
        check(_lib.dsr_mllr_set_stats_arrays(self.h, int(s), _ptr(c), _ptr(sumO)))

    def estimate(self, threshold=1500.0):
        check(_lib.dsr_mllr_estimate(self.h, float(threshold), cur_stream()))

    def speaker_status(self, s):
        return _lib.dsr_mllr_speaker_status(self.h, int(s))

    def plan(self):
        """the steps of the last estimate: rows (speaker, node, leaf, copy)"""
        n = C.c_int(0); check(_lib.dsr_mllr_get_plan(self.h, C.byref(n), None))
        a = np.zeros((n.value, 4), np.int32); check(_lib.dsr_mllr_get_plan(self.h, C.byref(n), _ptr(a))); return a

    def nodes(self):
        n = C.c_int(0); check(_lib.dsr_mllr_get_nodes(self.h, C.byref(n), None, None))
        a = np.zeros(n.value, np.uint32); leaf = np.zeros(n.value, np.int32); check(_lib.dsr_mllr_get_nodes(self.h, C.byref(n), _ptr(a), _ptr(leaf)))
        return [int(x) for x in a], [bool(x) for x in leaf]

    def stats(self, s, node, row):
        """-> G_i [D + 1][D + 1], z_i [D + 1] of the last estimate"""
        n = self.D + 1; Gi = np.zeros((n, n)); z = np.zeros(n)
        check(_lib.dsr_mllr_get_stats(self.h, int(s), int(node), int(row), _ptr(Gi), _ptr(z))); return Gi, z

    def ttl_frames(self, s, node):
        t = C.c_double(0.0); check(_lib.dsr_mllr_ttl_frames(self.h, int(s), int(node), C.byref(t))); return t.value

    def tree(self, s):
        h = _lib.dsr_mllr_tree(self.h, int(s))
        if not h:
            raise DsrError(E_INDEX, "speaker %d of %d" % (s, self.S))
        return ParamTree(handle=vp(h), owner=self)

    def transform(self, s, rc):
        W = np.zeros((self.D, self.D + 1)); check(_lib.dsr_mllr_get_transform(self.h, int(s), int(rc), _ptr(W))); return W

    def write(self, s, fileName):
        check(_lib.dsr_mllr_write(self.h, int(s), fileName.encode()))

    def read(self, s, fileName):
        check(_lib.dsr_mllr_read(self.h, int(s), fileName.encode()))

    def adapt(self, s, target=None):
        check(_lib.dsr_mllr_adapt(self.h, int(s), (target or self.gmm).h))

    def adapt_all(self, out=None):
        """-> cuda float32 [S][G][D]: every speaker's transformed means"""
        import torch
        if out is None:
            out = torch.empty((self.S, self.G, self.D), dtype=torch.float32, device="cuda")
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (self.S, self.G, self.D)
        check(_lib.dsr_mllr_adapt_all(self.h, _dev(out), cur_stream())); return out

    def reset_mean(self, target=None):
        check(_lib.dsr_mllr_reset_mean(self.h, (target or self.gmm).h))

    def set_timing(self, on=True):
        check(_lib.dsr_mllr_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 3)(); check(_lib.dsr_mllr_kernel_ms(self.h, ms)); return ms[0], ms[1], ms[2]


class Fsa:
    """Feature-space adaptation (constrained MLLR) for several accumulators and transformations (csrc/k_fsa.hip, csrc/fsa.cpp; include/dsr.h
    section 11): statistics on fp64 MFMA, Jacobi pseudo-inverses and the row updates on the device, the transform bit-exact.
    Made from a Gmm, or around the handle a FeatureSpaceAdaptationFeature stream owns (handle=, owner=)."""

    def __init__(self, gmm=None, nAccu=1, nTran=1, handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle
        else:
            self.h = vp(); check(L.dsr_fsa_create(gmm.h, int(nAccu), int(nTran), C.byref(self.h)))
        self.gmm = gmm; self.D = L.dsr_fsa_dim(self.h); self.nAccu = L.dsr_fsa_num_accus(self.h); self.nTran = L.dsr_fsa_num_transforms(self.h)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None) and self._owner is None:
            _lib.dsr_fsa_destroy(self.h)

    def add(self, dsX):
        check(_lib.dsr_fsa_add(self.h, int(dsX)))

    def add_all(self):
        check(_lib.dsr_fsa_add_all(self.h))

    def set_top_n(self, topN):
        check(_lib.dsr_fsa_set_top_n(self.h, int(topN)))

    def top_n(self):
        return _lib.dsr_fsa_top_n(self.h)

    def set_shift(self, shift):
        check(_lib.dsr_fsa_set_shift(self.h, float(shift)))

    def shift(self):
        return _lib.dsr_fsa_shift(self.h)

    def count(self, accuX=0):
        c = C.c_double(0.0); check(_lib.dsr_fsa_count(self.h, int(accuX), C.byref(c))); return c.value

    def _frames(self, xScore, xSrc):
        xSrc = xScore if xSrc is None else xSrc
        for x in (xScore, xSrc):
            assert x.is_cuda and x.is_contiguous() and x.dtype.is_floating_point and x.element_size() == 4 and x.shape[1] == self.D
        assert xScore.shape[0] == xSrc.shape[0]
        return xScore, xSrc

    def accumulate(self, xScore, frame, dist, gamma, accu, xSrc=None, want_nearest=False):
        """xScore, xSrc: cuda float32 [N][D] (xSrc None: the same frames); frame, dist, gamma, accu: host arrays [M] -> accepted items [nAccu]
        (with want_nearest also the Gaussian each item chose inside its codebook, -1 for a distribution that is not switched on)"""
        xScore, xSrc = self._frames(xScore, xSrc)
        fr = _np(frame, np.int32); ds = _np(dist, np.int32); ga = _np(gamma, np.float32); ac = _np(accu, np.int32); M = len(fr)
        assert len(ds) == M and len(ga) == M and len(ac) == M
        acc = np.zeros(self.nAccu, np.int64); near = np.full(M, -1, np.int32) if want_nearest else None
        check(_lib.dsr_fsa_accumulate(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(fr), _ptr(ds), _ptr(ga), _ptr(ac), M, _ptr(acc),
                                      _ptr(near) if want_nearest else None, cur_stream()))
        return (acc, near) if want_nearest else acc

    def accumulate_path(self, xScore, distIds, accuX=0, factor=1.0, xSrc=None):
        """distIds: one distribution per frame, negative for a name the set does not know -> the frames the reference reports"""
        xScore, xSrc = self._frames(xScore, xSrc); ids = _np(distIds, np.int32); n = C.c_uint(0)
        check(_lib.dsr_fsa_accumulate_path(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(ids), len(ids), int(accuX), float(factor), C.byref(n), cur_stream()))
        return n.value

    def accumulate_lattice(self, lattice, xScore, accuX=0, factor=1.0, xSrc=None):
        """lattice: a Lattice (after gammaProbs) -> the number of links accumulated"""
        xScore, xSrc = self._frames(xScore, xSrc); n = C.c_uint(0)
        check(_lib.dsr_fsa_accumulate_lattice(self.h, lattice.h, _dev(xScore), _dev(xSrc), xScore.shape[0], int(accuX), float(factor), C.byref(n), cur_stream()))
        return n.value

    def zero(self, accuX=0):
        check(_lib.dsr_fsa_zero(self.h, int(accuX)))

    def scale(self, scale, accuX=0):
        check(_lib.dsr_fsa_scale(self.h, float(scale), int(accuX)))

    def add_accu(self, accuX, accuY, factor=1.0):
        check(_lib.dsr_fsa_add_accu(self.h, int(accuX), int(accuY), float(factor)))

    def get_accu(self, accuX=0):
        """-> dict(count, beta (float32), z [D][D + 1], G [D][D + 1][D + 1] with the triangle as the reference holds it)"""
        D = self.D; c = C.c_double(0.0); b = C.c_float(0.0); z = np.zeros((D, D + 1)); G = np.zeros((D, D + 1, D + 1))
        check(_lib.dsr_fsa_get_accu(self.h, int(accuX), C.byref(c), C.byref(b), _ptr(z), _ptr(G)))
        return dict(count=c.value, beta=np.float32(b.value), z=z, G=G)

    def set_accu(self, accuX=0, count=None, beta=None, z=None, G=None):
        D = self.D
        c = C.byref(C.c_double(float(count))) if count is not None else None
        b = C.byref(C.c_float(float(beta))) if beta is not None else None
        if z is not None:
            z = _np(z, np.float64); assert z.shape == (D, D + 1)
        if G is not None:
            G = _np(G, np.float64); assert G.shape == (D, D + 1, D + 1)
        check(_lib.dsr_fsa_set_accu(self.h, int(accuX), c, b, _ptr(z) if z is not None else None, _ptr(G) if G is not None else None))

    def save_accu(self, fileName, accuX=0):
        check(_lib.dsr_fsa_save_accu(self.h, fileName.encode(), int(accuX)))

    def load_accu(self, fileName, accuX=0, factor=1.0):
        check(_lib.dsr_fsa_load_accu(self.h, fileName.encode(), int(accuX), float(factor)))

    def estimate(self, iterN=1, accuX=0, tranX=0):
        """accuX, tranX: ints or equally long lists: the pairs are estimated concurrently"""
        a = _np(np.atleast_1d(accuX), np.int32); t = _np(np.atleast_1d(tranX), np.int32); assert len(a) == len(t)
        check(_lib.dsr_fsa_estimate(self.h, int(iterN), _ptr(a), _ptr(t), len(a), cur_stream()))

    def transform_status(self, tranX=0):
        return _lib.dsr_fsa_transform_status(self.h, int(tranX))

    def transform(self, tranX=0):
        W = np.zeros((self.D, self.D + 1)); check(_lib.dsr_fsa_get_transform(self.h, int(tranX), _ptr(W))); return W

    def set_transform(self, W, tranX=0):
        W = _np(W, np.float64); assert W.shape == (self.D, self.D + 1)
        check(_lib.dsr_fsa_set_transform(self.h, int(tranX), _ptr(W)))

    def clear(self, tranX=0):
        check(_lib.dsr_fsa_clear(self.h, int(tranX)))

    def compare(self, tranX, tranY):
        s = C.c_float(0.0); check(_lib.dsr_fsa_compare(self.h, int(tranX), int(tranY), C.byref(s))); return np.float32(s.value)

    def save(self, fileName, tranX=0):
        check(_lib.dsr_fsa_save(self.h, fileName.encode(), int(tranX)))

    def load(self, fileName, tranX=0):
        check(_lib.dsr_fsa_load(self.h, fileName.encode(), int(tranX)))

    def apply(self, x, tranOfRow=None, shift=1.0, out=None):
        """x: cuda float32 [N][D]; tranOfRow: cuda int32 [N] or None (transformation 0) -> cuda float32 [N][D]"""
        import torch
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.D
        if out is None:
            out = torch.empty_like(x)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == x.shape
        if tranOfRow is not None:
            assert tranOfRow.is_cuda and tranOfRow.is_contiguous() and tranOfRow.dtype == torch.int32 and tranOfRow.shape[0] == x.shape[0]
        check(_lib.dsr_fsa_apply(self.h, _dev(x), x.shape[0], _dev(tranOfRow) if tranOfRow is not None else None, float(shift), _dev(out), cur_stream()))
        return out

    def set_timing(self, on=True):
        check(_lib.dsr_fsa_set_timing(self.h, int(on)))

    def kernel_ms(self):
        ms = (C.c_float * 5)(); check(_lib.dsr_fsa_kernel_ms(self.h, ms)); return tuple(ms)


class _Estimators:
    """what Stc and Lda share: frames, items, timing"""

    def _frames(self, xScore, xSrc):
        xSrc = xScore if xSrc is None else xSrc
        for x in (xScore, xSrc):
            assert x.is_cuda and x.is_contiguous() and x.dtype.is_floating_point and x.element_size() == 4 and x.shape[1] == self.D
        assert xScore.shape[0] == xSrc.shape[0]
        return xScore, xSrc

    def _items(self, fn, xScore, frame, dist, factor, est, xSrc, want):
        xScore, xSrc = self._frames(xScore, xSrc)
        fr = _np(frame, np.int32); ds = _np(dist, np.int32); fa = _np(factor, np.float32); es = _np(est, np.int32); M = len(fr)
        assert len(ds) == M and len(fa) == M and len(es) == M
        near = np.full(M, -1, np.int32); score = np.zeros(M, np.float32)
        check(fn(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(fr), _ptr(ds), _ptr(fa), _ptr(es), M, _ptr(near), _ptr(score), cur_stream()))
        return (near, score) if want else None

    def _mat(self, M, shape):
        M = _np(M, np.float64); assert M.shape == shape
        return M

    def kernel_ms(self):
        ms = (C.c_float * 5)(); check(self._kernel_ms(self.h, ms)); return tuple(ms)


class Stc(_Estimators):
    """Semi-tied covariance transforms for nEst estimators over one Gmm (csrc/k_stc.hip, csrc/stc.cpp; include/dsr.h section 12): statistics
    on fp64 MFMA, makePosDef's eigenvalues, the inverses and the row updates on the device, the transform bit-exact.  Made from a Gmm, as a
    bare transformer (dimN=), or around the handle an STCTransformer stream owns (handle=, owner=)."""

    def __init__(self, gmm=None, nEst=1, cascade=False, mmiEstimation=False, dimN=None, handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle
        elif gmm is not None:
            self.h = vp(); check(L.dsr_stc_create(gmm.h, int(nEst), int(bool(cascade)), int(bool(mmiEstimation)), C.byref(self.h)))
        else:
            self.h = vp(); check(L.dsr_stc_create_transformer(int(dimN), C.byref(self.h)))
        self.gmm = gmm; self.D = L.dsr_stc_dim(self.h); self.nEst = L.dsr_stc_num_estimators(self.h); self._kernel_ms = L.dsr_stc_kernel_ms

    def __del__(self):
        if _lib is not None and getattr(self, "h", None) and self._owner is None:
            _lib.dsr_stc_destroy(self.h)

    def accumulate(self, xScore, frame, dist, factor, est, xSrc=None, want_nearest=False):
        """xScore, xSrc: cuda float32 [N][D] (xSrc None: the same frames); frame, dist, factor, est: host arrays [M]; with want_nearest ->
        (the Gaussian each item chose inside its codebook, the distribution's score of each item)"""
        return self._items(_lib.dsr_stc_accumulate, xScore, frame, dist, factor, est, xSrc, want_nearest)

    def accumulate_path(self, xScore, distIds, estX=0, factor=1.0, xSrc=None):
        """distIds: one distribution per frame -> the number of frames"""
        xScore, xSrc = self._frames(xScore, xSrc); ids = _np(distIds, np.int32); n = C.c_uint(0)
        check(_lib.dsr_stc_accumulate_path(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(ids), len(ids), int(estX), float(factor), C.byref(n), cur_stream()))
        return n.value

    def increment(self, totalPr, totalT=0, estX=0):
        check(_lib.dsr_stc_increment(self.h, int(estX), float(totalPr), int(totalT)))

    def zero(self, estX=0):
        check(_lib.dsr_stc_zero(self.h, int(estX)))

    def get_accu(self, estX=0, through_accessor=False):
        """-> dict(count, denCount, totalPr, totalT, sumOsq [D][D][D], regSq [D][D][D]); through_accessor: after copyUpperTriangle, as the
        reference's sumOsq() / regSq() return them (and leave them); else the triangle as accumulation left it"""
        D = self.D; c = C.c_double(0.0); dc = C.c_double(0.0); pr = C.c_double(0.0); T = C.c_uint(0); S = np.zeros((D, D, D)); R = np.zeros((D, D, D))
        check(_lib.dsr_stc_get_accu(self.h, int(estX), int(bool(through_accessor)), C.byref(c), C.byref(dc), C.byref(pr), C.byref(T), _ptr(S), _ptr(R)))
        return dict(count=c.value, denCount=dc.value, totalPr=pr.value, totalT=T.value, sumOsq=S, regSq=R)

    def set_accu(self, estX=0, count=None, denCount=None, totalPr=None, totalT=None, sumOsq=None, regSq=None):
        D = self.D; dbl = lambda v: C.byref(C.c_double(float(v))) if v is not None else None      # noqa: E731
        S = self._mat(sumOsq, (D, D, D)) if sumOsq is not None else None; R = self._mat(regSq, (D, D, D)) if regSq is not None else None
        check(_lib.dsr_stc_set_accu(self.h, int(estX), dbl(count), dbl(denCount), dbl(totalPr), C.byref(C.c_uint(int(totalT))) if totalT is not None else None,
                                    _ptr(S) if S is not None else None, _ptr(R) if R is not None else None))

    def save_accu(self, fileName, estX=0):
        check(_lib.dsr_stc_save_accu(self.h, fileName.encode(), int(estX)))

    def load_accu(self, fileName, estX=0):
        check(_lib.dsr_stc_load_accu(self.h, fileName.encode(), int(estX)))

    def estimate(self, estX=0, minE=1.0, multE=1.0):
        """estX: an int or a list: the estimators are estimated concurrently"""
        e = _np(np.atleast_1d(estX), np.int32)
        check(_lib.dsr_stc_estimate(self.h, _ptr(e), len(e), float(minE), float(multE), cur_stream()))

    def status(self, estX=0):
        return _lib.dsr_stc_status(self.h, int(estX))

    def E(self, estX=0):
        e = C.c_double(0.0); check(_lib.dsr_stc_E(self.h, int(estX), C.byref(e))); return e.value

    def aux(self, estX=0, A=None, E=None):
        """the auxiliary function the row update maximises, of A (None: the estimator's matrix) at E (None: the last estimate's)"""
        q = C.c_double(0.0); A = self._mat(A, (self.D, self.D)) if A is not None else None
        check(_lib.dsr_stc_aux(self.h, int(estX), _ptr(A) if A is not None else None, float(self.E(estX) if E is None else E), C.byref(q))); return q.value

    def transform(self, estX=0):
        A = np.zeros((self.D, self.D)); check(_lib.dsr_stc_get_transform(self.h, int(estX), _ptr(A), None)); return A

    def inverse(self, estX=0):
        A = np.zeros((self.D, self.D)); check(_lib.dsr_stc_get_transform(self.h, int(estX), None, _ptr(A))); return A

    def set_transform(self, A, estX=0):
        check(_lib.dsr_stc_set_transform(self.h, int(estX), _ptr(self._mat(A, (self.D, self.D)))))

    def trans_matrix(self, estX=0):
        T = np.zeros((self.D, self.D), np.float32); check(_lib.dsr_stc_trans_matrix(self.h, int(estX), _ptr(T))); return T

    def save(self, fileName, estX=0):
        check(_lib.dsr_stc_save(self.h, fileName.encode(), int(estX)))

    def load(self, fileName, estX=0):
        check(_lib.dsr_stc_load(self.h, fileName.encode(), int(estX)))

    def save_float(self, fileName, trans=None, estX=0):
        if trans is not None:
            trans = _np(trans, np.float32); assert trans.shape == (self.D, self.D)
        check(_lib.dsr_stc_save_float(self.h, fileName.encode(), int(estX), _ptr(trans) if trans is not None else None))

    def apply(self, x, estX=0, out=None):
        """x: cuda float32 [N][D] -> cuda float32 [N][D]"""
        import torch
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.D
        if out is None:
            out = torch.empty_like(x)
        assert out.is_contiguous() and out.dtype == torch.float32 and out.shape == x.shape
        check(_lib.dsr_stc_apply(self.h, _dev(x), x.shape[0], int(estX), _dev(out), cur_stream()))
        return out

    def set_timing(self, on=True):
        check(_lib.dsr_stc_set_timing(self.h, int(on)))


class Lda(_Estimators):
    """LDA matrices for nEst estimators over one Gmm (csrc/k_stc.hip, csrc/stc.cpp; include/dsr.h section 12): the three scatter matrices on
    fp64 MFMA, the simultaneous diagonalisation by Jacobi on the device.  globalGmm: a Gmm whose codebook 0 is the global codebook.  Made
    from two Gmms, as a bare transformer (dimN=), or around the handle an LDATransformer stream owns (handle=, owner=)."""

    def __init__(self, gmm=None, globalGmm=None, nEst=1, dimN=None, handle=None, owner=None):
        L = load(); self._owner = owner
        if handle is not None:
            self.h = handle
        elif gmm is not None:
            self.h = vp(); check(L.dsr_lda_create(gmm.h, globalGmm.h, int(nEst), C.byref(self.h)))
        else:
            self.h = vp(); check(L.dsr_lda_create_transformer(int(dimN), C.byref(self.h)))
        self.gmm, self.globalGmm = gmm, globalGmm; self.D = L.dsr_lda_dim(self.h); self.nEst = L.dsr_lda_num_estimators(self.h); self._kernel_ms = L.dsr_lda_kernel_ms

    def __del__(self):
        if _lib is not None and getattr(self, "h", None) and self._owner is None:
            _lib.dsr_lda_destroy(self.h)

    def accumulate(self, xScore, frame, dist, factor, est, xSrc=None, want_nearest=False):
        return self._items(_lib.dsr_lda_accumulate, xScore, frame, dist, factor, est, xSrc, want_nearest)

    def accumulate_path(self, xScore, distIds, estX=0, factor=1.0, xSrc=None):
        """-> the summed score of the path's distributions"""
        xScore, xSrc = self._frames(xScore, xSrc); ids = _np(distIds, np.int32); s = C.c_double(0.0)
        check(_lib.dsr_lda_accumulate_path(self.h, _dev(xScore), _dev(xSrc), xScore.shape[0], _ptr(ids), len(ids), int(estX), float(factor), C.byref(s), cur_stream()))
        return s.value

    def zero(self, estX=0):
        check(_lib.dsr_lda_zero(self.h, int(estX)))

    def get_accu(self, estX=0, through_accessor=False):
        """-> dict(count, within, between, mixture [D][D])"""
        D = self.D; c = C.c_double(0.0); W = np.zeros((D, D)); B = np.zeros((D, D)); M = np.zeros((D, D))
        check(_lib.dsr_lda_get_accu(self.h, int(estX), int(bool(through_accessor)), C.byref(c), _ptr(W), _ptr(B), _ptr(M)))
        return dict(count=c.value, within=W, between=B, mixture=M)

    def set_accu(self, estX=0, count=None, within=None, between=None, mixture=None):
        D = self.D; m = [self._mat(x, (D, D)) if x is not None else None for x in (within, between, mixture)]
        check(_lib.dsr_lda_set_accu(self.h, int(estX), C.byref(C.c_double(float(count))) if count is not None else None,
                                    *[_ptr(x) if x is not None else None for x in m]))

    def save_accu(self, fileName, estX=0):
        check(_lib.dsr_lda_save_accu(self.h, fileName.encode(), int(estX)))

    def load_accu(self, fileName, estX=0):
        check(_lib.dsr_lda_load_accu(self.h, fileName.encode(), int(estX)))

    def estimate(self, estX=0):
        e = _np(np.atleast_1d(estX), np.int32)
        check(_lib.dsr_lda_estimate(self.h, _ptr(e), len(e), cur_stream()))

    def status(self, estX=0):
        return _lib.dsr_lda_status(self.h, int(estX))

    def eigenvalues(self, estX=0):
        """-> (eigenvalues of within as found, eigenvalues of the whitened between, descending) of the last estimate"""
        w = np.zeros(self.D); b = np.zeros(self.D); check(_lib.dsr_lda_eigenvalues(self.h, int(estX), _ptr(w), _ptr(b))); return w, b

    def transform(self, estX=0):
        L = np.zeros((self.D, self.D)); check(_lib.dsr_lda_get_transform(self.h, int(estX), _ptr(L))); return L

    def set_transform(self, L, estX=0):
        check(_lib.dsr_lda_set_transform(self.h, int(estX), _ptr(self._mat(L, (self.D, self.D)))))

    def save(self, fileName, estX=0):
        check(_lib.dsr_lda_save(self.h, fileName.encode(), int(estX)))

    def load(self, fileName, estX=0):
        check(_lib.dsr_lda_load(self.h, fileName.encode(), int(estX)))

    def apply(self, x, outDim=None, estX=0, out=None):
        """x: cuda float32 [N][D] -> cuda float32 [N][outDim]: the first outDim rows of the matrix"""
        import torch
        outDim = self.D if outDim is None else int(outDim)
        assert x.is_cuda and x.is_contiguous() and x.dtype == torch.float32 and x.shape[1] == self.D
        if out is None:
            out = torch.empty((x.shape[0], outDim), dtype=torch.float32, device=x.device)
        assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (x.shape[0], outDim)
        check(_lib.dsr_lda_apply(self.h, _dev(x), x.shape[0], int(estX), outDim, _dev(out), cur_stream()))
        return out

    def set_timing(self, on=True):
        check(_lib.dsr_lda_set_timing(self.h, int(on)))


class Wfst:
    """WFSTFlyWeight (asr/decoder/wfstFlyWeight.h:47-119)."""

    def __init__(self):
        L = load(); self.h = vp(); check(L.dsr_wfst_create(C.byref(self.h)))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_wfst_destroy(self.h)

    def read(self, fileName, binary=False):
        check(_lib.dsr_wfst_read(self.h, fileName.encode(), int(binary)))

    def read_dynamic(self, fileName, noSelfLoops=False):
        """WFSTransducer::read (asr/fsm/fsm.cc:901-986)"""
        check(_lib.dsr_wfst_read_dynamic(self.h, fileName.encode(), int(noSelfLoops)))

    def write(self, fileName, binary=True):
        check(_lib.dsr_wfst_write(self.h, fileName.encode(), int(binary)))

    def add_arc(self, s1, s2, i, o, cost=0.0):
        check(_lib.dsr_wfst_add_arc(self.h, s1, s2, i, o, cost))

    def add_final(self, s, cost=0.0):
        check(_lib.dsr_wfst_add_final(self.h, s, cost))

    def export(self):
        n = _lib.dsr_wfst_num_nodes(self.h); a = _lib.dsr_wfst_num_arcs(self.h)
        d = dict(nodeState=np.zeros(n, np.uint32), nodeFinal=np.zeros(n, np.int32), nodeCost=np.zeros(n, np.float32),
                 arcOff=np.zeros(n + 1, np.int32), arcDst=np.zeros(max(a, 1), np.int32), arcIn=np.zeros(max(a, 1), np.uint32),
                 arcOut=np.zeros(max(a, 1), np.uint32), arcCost=np.zeros(max(a, 1), np.float32))
        check(_lib.dsr_wfst_export(self.h, *[_ptr(d[k]) for k in ("nodeState", "nodeFinal", "nodeCost", "arcOff", "arcDst", "arcIn", "arcOut", "arcCost")]))
        for k in ("arcDst", "arcIn", "arcOut", "arcCost"):
            d[k] = d[k][:a]
        return d


class Decoder:
    """DecoderFlyWeight (asr/decoder/decoder.i:147-199) for batches of score matrices."""

    def __init__(self, beam=100.0, lmScale=12.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0xFFFFFFFF, maxActive=0,
                 maxCandidates=0, arenaTokens=0, streams=0, latticeTokens=0, topN=0, wordTrace=0, generateLattice=True, propagateN=5, fastHash=False,
                 insertSilence=False, wordTraces=0):
        L = load(); c = DecoderCfg(); L.dsr_decoder_default_cfg(C.byref(c))
        c.wordTrace, c.wordTraceLattice, c.propagateN, c.fastHash, c.insertSilence, c.wordTraces = int(wordTrace), int(generateLattice), propagateN, int(fastHash), int(insertSilence), wordTraces
        c.beam, c.lmScale, c.lmPenalty, c.silPenalty, c.silenceX = beam, lmScale, lmPenalty, silPenalty, silenceX
        c.maxActive, c.maxCandidates, c.arenaTokens, c.streams, c.latticeTokens, c.topN = maxActive, maxCandidates, arenaTokens, streams, latticeTokens, topN
        self.h = vp(); check(L.dsr_decoder_create(C.byref(c), C.byref(self.h))); self._g = None

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_decoder_destroy(self.h)

    def set(self, wfst):
        check(_lib.dsr_decoder_set(self.h, wfst.h)); self._g = wfst

    def setBeam(self, beam):
        check(_lib.dsr_decoder_set_beam(self.h, beam))

    def enable_dump(self, on=True):
        check(_lib.dsr_decoder_enable_dump(self.h, int(on)))

    def decode_batch(self, scores, nframes=None, maxPath=None):
        """scores: cuda float32 [U][T][nDist].  Returns list of dicts."""
        import torch
        U, T, nDist = scores.shape
        if nframes is None:
            nframes = torch.full((U,), T, dtype=torch.int32, device=scores.device)
        if maxPath is None:
            maxPath = 4 * T + 64
        res = (DecodeResult * U)()
        arcs = np.zeros((U, maxPath), np.int32); words = np.zeros((U, maxPath), np.uint32)
        check(_lib.dsr_decoder_decode_batch(self.h, _dev(scores), _dev(nframes), U, T, nDist, C.byref(res), _ptr(arcs), _ptr(words), maxPath, cur_stream()))
        out = []
        for u in range(U):
            r = res[u]
            out.append(dict(status=r.status, score=r.score, ac=r.ac, lm=r.lm, frames=r.frames, reachedFinal=bool(r.reachedFinal),
                            arcs=arcs[u, :min(r.nArcs, maxPath)].copy(), words=words[u, :min(r.nWords, maxPath)].copy(),
                            activeHypos=r.activeHypos, maxActive=r.maxActiveSeen, placements=r.placements, registerFrames=r.registerFrames, laidOutFrames=r.laidOutFrames_, finalStatesN=r.finalStatesN))
        return out

    def lattice(self, u=0, eosX=0):
        """_Decoder::lattice() (decoder.h:805-860) of utterance u of the last decode (needs latticeTokens > 0)"""
        h = vp(); check(_lib.dsr_decoder_lattice(self.h, int(u), int(eosX), C.byref(h)))
        return Lattice(h)

    def writeGMM(self, u, conv, channel, spk, utt, cfrom, score, fileName="", frameInterval=0.01):
        """_Decoder::writeGMM (decoder.h:1018-1102) of utterance u of the last decode (needs latticeTokens > 0 and set_symbols)"""
        check(_lib.dsr_decoder_write_gmm(self.h, int(u), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                         (fileName or "").encode(), float(frameInterval)))

    def get_dump(self):
        n = i64(); fo = C.POINTER(i64)(); nd = C.POINTER(i32)(); ac = C.POINTER(f32)(); lm = C.POINTER(f32)(); arc = C.POINTER(i32)()
        check(_lib.dsr_decoder_get_dump(self.h, C.byref(n), C.byref(fo), C.byref(nd), C.byref(ac), C.byref(lm), C.byref(arc)))
        nf = n.value
        off = np.array([fo[i] for i in range(nf + 1)], np.int64) if nf > 0 else np.zeros(1, np.int64)
        N = int(off[-1])
        g = lambda p, dt: np.ctypeslib.as_array(p, (N,)).astype(dt).copy() if N > 0 else np.zeros(0, dt)
        return dict(frameOff=off, node=g(nd, np.int32), ac=g(ac, np.float32), lm=g(lm, np.float32), arc=g(arc, np.int32))


def _lexh(lex):
    """handle of a lexicon object (asr.dictionary.LexiconPtr keeps it in _h) or None"""
    if lex is None:
        return None
    return getattr(lex, "_h", None) or getattr(lex, "h", None)


class Lattice:
    """asr/lattice Lattice as the decoder builds it: nodes numbered as the reference numbers them (0 = initial), edges in creation order."""

    def __init__(self, handle):
        self.h = handle
        n, e = _lib.dsr_lattice_num_nodes(self.h), _lib.dsr_lattice_num_edges(self.h)
        d = {"nodeFinal": np.zeros(n, np.int32), "from": np.zeros(e, np.int32), "to": np.zeros(e, np.int32), "in": np.zeros(e, np.uint32),
             "out": np.zeros(e, np.uint32), "start": np.zeros(e, np.int32), "end": np.zeros(e, np.int32), "ac": np.zeros(e, np.float64), "lm": np.zeros(e, np.float64)}
        check(_lib.dsr_lattice_get(self.h, *[_ptr(d[k]) for k in ("nodeFinal", "from", "to", "in", "out", "start", "end", "ac", "lm")]))
        self.data = d; self.finalStatesN = _lib.dsr_lattice_final_states_n(self.h)

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_lattice_destroy(self.h)

    def write(self, fileName, useSymbols=False, writeData=False):
        """Lattice::write (lattice.cc:715-757); useSymbols needs the lexica and is not offered here"""
        if useSymbols:
            raise DsrError(13, "useSymbols: write the numeric form and map the symbols with the lexica")
        check(_lib.dsr_lattice_write(self.h, fileName.encode(), int(writeData)))

    # ---- asr/lattice operations (lattice.i:79-123); symbols cross the boundary as indices, asr/lattice.py joins them with the lexica
    @staticmethod
    def read(fileName, noSelfLoops=False, readData=False, inlex=None, outlex=None):
        """WFST::read(fileName, noSelfLoops, readData) (fsm.h:3787-3873); inlex/outlex: Lexicon objects (or None) for symbolic files"""
        load(); h = vp()
        check(_lib.dsr_lattice_read(fileName.encode(), int(noSelfLoops), int(readData), _lexh(inlex), _lexh(outlex), C.byref(h)))
        return Lattice(h)

    def rescore(self, lmScale=30.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0):
        sc = C.c_float(0.0)
        check(_lib.dsr_lattice_rescore(self.h, float(lmScale), float(lmPenalty), float(silPenalty), int(silenceX), C.byref(sc)))
        return np.float32(sc.value)

    def bestHypo(self, useInputSymbols=False):
        n = C.c_int(0); check(_lib.dsr_lattice_best_hypo(self.h, int(useInputSymbols), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        check(_lib.dsr_lattice_best_hypo(self.h, int(useInputSymbols), _ptr(out), out.size, C.byref(n)))
        return out[:n.value].copy()

    def gammaProbs(self, acScale=1.0, lmScale=12.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0):
        p = C.c_double(0.0)
        check(_lib.dsr_lattice_gamma_probs(self.h, float(acScale), float(lmScale), float(lmPenalty), float(silPenalty), int(silenceX), C.byref(p)))
        return p.value

    def gammaProbsDist(self, distribset, acScale=1.0, lmScale=12.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0):
        """Lattice::gammaProbsDist (lattice.cc:331-341): distribset = a dsr_distribset handle (asr.gaussian.DistribSetBasicPtr keeps it in _ds)"""
        p = C.c_double(0.0)
        check(_lib.dsr_lattice_gamma_probs_dist(self.h, distribset, float(acScale), float(lmScale), float(lmPenalty), float(silPenalty), int(silenceX), C.byref(p)))
        return p.value

    def prune(self, threshold=100.0):
        check(_lib.dsr_lattice_prune(self.h, float(threshold)))

    def pruneEdges(self, edgesN=0):
        check(_lib.dsr_lattice_prune_edges(self.h, int(edgesN)))

    def purge(self):
        check(_lib.dsr_lattice_purge(self.h))

    def state(self):
        """per link (creation order): gamma, still on its node's list; per node (creation order): printed index, still held, forward, backward"""
        n, e = _lib.dsr_lattice_num_nodes(self.h), _lib.dsr_lattice_num_edges(self.h)
        d = dict(gamma=np.zeros(e, np.float64), edgeLive=np.zeros(e, np.int32), nodeIndex=np.zeros(n, np.int32), nodeLive=np.zeros(n, np.int32),
                 fwd=np.zeros(n, np.float64), bwd=np.zeros(n, np.float64))
        check(_lib.dsr_lattice_get_state(self.h, *[_ptr(d[k]) for k in ("gamma", "edgeLive", "nodeIndex", "nodeLive", "fwd", "bwd")]))
        return d

    def writeCTM(self, outlex, conv, channel, spk, utt, cfrom, score, fileName="", frameInterval=0.01, endMarker="</s>"):
        check(_lib.dsr_lattice_write_ctm(self.h, _lexh(outlex), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                         fileName.encode(), float(frameInterval), endMarker.encode()))

    def writePhoneCTM(self, inlex, conv, channel, spk, utt, cfrom, score, fileName="", frameInterval=0.01, endMarker="</s>"):
        check(_lib.dsr_lattice_write_phone_ctm(self.h, _lexh(inlex), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                               fileName.encode(), float(frameInterval), endMarker.encode()))

    def writeHypoHTK(self, outlex, conv, channel, spk, utt, cfrom, score, fileName="", flag=0, frameInterval=0.01, endMarker="</s>"):
        check(_lib.dsr_lattice_write_hypo_htk(self.h, _lexh(outlex), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                              fileName.encode(), int(flag), float(frameInterval), endMarker.encode()))

    def writeWordConfs(self, outlex, fileName, uttId, endMarker="</s>"):
        check(_lib.dsr_lattice_write_word_confs(self.h, _lexh(outlex), fileName.encode(), uttId.encode(), endMarker.encode()))

    def pack(self):
        n = _lib.dsr_lattice_pack_size(self.h); b = np.zeros(n, np.uint8)
        check(_lib.dsr_lattice_pack(self.h, _ptr(b), n)); return b

    @staticmethod
    def unpack(buf):
        load(); b = np.ascontiguousarray(buf, np.uint8); h = vp()
        check(_lib.dsr_lattice_unpack(_ptr(b), b.size, C.byref(h))); return Lattice(h)


class Pipe:
    def __init__(self, ana, syn, bf, mfcc, gmm, dec, gmmMode=0, fused=False):
        """fused: analysis bank and fixed-weight beamformer as one kernel where supported (the channel snapshots are then never written)"""
        L = load(); self.h = vp(); self._keep = (ana, syn, bf, mfcc, gmm, dec)
        check(L.dsr_pipe_create(ana.h, syn.h, bf.h, mfcc.h, gmm.h, dec.h, gmmMode, C.byref(self.h)))
        if fused:
            check(L.dsr_pipe_set_fused(self.h, 1))

    def __del__(self):
        if _lib is not None and getattr(self, "h", None):
            _lib.dsr_pipe_destroy(self.h)

    def run(self, x, nsamp_dev, nsamp_host, maxPath=4096, want_paths=True):
        U, Cn, N = x.shape
        res = (DecodeResult * U)()
        ns = _np(nsamp_host, np.int32)
        arcs = np.zeros((U, maxPath), np.int32) if want_paths else None
        words = np.zeros((U, maxPath), np.uint32) if want_paths else None
        check(_lib.dsr_pipe_run(self.h, _dev(x), _dev(nsamp_dev), _ptr(ns), U, Cn, N, C.byref(res),
                                _ptr(arcs) if want_paths else None, _ptr(words) if want_paths else None, maxPath, cur_stream()))
        return res, arcs, words

    def submit(self, x, nsamp_dev, nsamp_host, maxPath=4096, want_paths=True):
        """Enqueue one batch on the current stream and return; collect() waits for it.  One batch in flight per Pipe."""
        U, Cn, N = x.shape
        ns = _np(nsamp_host, np.int32)
        self._inflight = (U, maxPath, want_paths, x, nsamp_dev, ns)              # keep the inputs alive until collected
        check(_lib.dsr_pipe_submit(self.h, _dev(x), _dev(nsamp_dev), _ptr(ns), U, Cn, N, maxPath, 1 if want_paths else 0, cur_stream()))

    def collect(self, reuse=False):
        """reuse: hand out the same host arrays call after call (rows are valid up to nArcs / nWords, the rest is whatever the call before left):
        a fresh zero-filled pair is 16 MB of page faults per 1000-utterance batch"""
        U, maxPath, want_paths = self._inflight[:3]
        res = (DecodeResult * U)()
        if reuse and want_paths:
            h = getattr(self, "_host", None)
            if h is None or h[0].shape != (U, maxPath):
                h = self._host = (np.zeros((U, maxPath), np.int32), np.zeros((U, maxPath), np.uint32))
            arcs, words = h
        else:
            arcs = np.zeros((U, maxPath), np.int32) if want_paths else None
            words = np.zeros((U, maxPath), np.uint32) if want_paths else None
        check(_lib.dsr_pipe_collect(self.h, C.byref(res), _ptr(arcs) if want_paths else None, _ptr(words) if want_paths else None))
        self._inflight = None
        return res, arcs, words

    def stage_ms(self):
        ms = (f32 * 6)(); check(_lib.dsr_pipe_stage_ms(self.h, ms)); return list(ms)

    def intermediate(self, which):
        p = vp(); n = i64(); check(_lib.dsr_pipe_intermediate(self.h, which, C.byref(p), C.byref(n))); return p.value, n.value

    def intermediate_host(self, which, dtype=np.float32):
        p, n = self.intermediate(which)
        out = np.zeros(n // np.dtype(dtype).itemsize, dtype)
        check(_lib.dsr_memcpy_dtoh(_ptr(out), vp(p), n, cur_stream()))
        return out


# ---- speech activity detection, btk/sad (include/dsr.h section 7b, csrc/k_sad.hip)
def _sad_out(U, T, device):
    import torch
    return torch.zeros((U, T), dtype=torch.float64, device=device), torch.zeros((U, T), dtype=torch.float64, device=device)


def sad_energy_state(U, energiesN=200, initialEnergy=5.0e+07, device="cuda:0"):
    """EnergyVADMetric after nextSpeaker(): (history float64 [U][energiesN] -- a ring --, counters int32 [U][4] = (aboveThresholdN,
    belowThresholdN, recognizing, ring position))"""
    import torch
    load(); hist = torch.zeros((U, energiesN), dtype=torch.float64, device=device); cnt = torch.zeros((U, 4), dtype=torch.int32, device=device)
    check(_lib.dsr_sad_energy_state_init(_dev(hist), _dev(cnt), U, int(energiesN), float(initialEnergy), 0, cur_stream()))
    return hist, cnt


def sad_energy_reset(state):
    """EnergyVADMetric::reset(): the counters are cleared, the history and its ring position stay"""
    hist, cnt = state
    check(load().dsr_sad_energy_state_init(_dev(hist), _dev(cnt), hist.shape[0], hist.shape[1], 0.0, 1, cur_stream()))
    return state


def sad_energy(x, threshold=0.5, headN=4, tailN=10, state=None, initialEnergy=5.0e+07, energiesN=200, nframes=None, return_updates=False):
    """EnergyVADMetric over the blocks of each utterance in order: x cuda float32 [U][Tmax][dim] -> (decision float64 [U][Tmax], score (the
    blocks' energies) float64 [U][Tmax], state).  state: the pair a previous call returned (None: nextSpeaker()); it is updated in place."""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    if state is None:
        state = sad_energy_state(U, energiesN, initialEnergy, x.device)
    hist, cnt = state
    assert hist.dtype == torch.float64 and cnt.dtype == torch.int32 and hist.dim() == 2 and hist.shape[0] == U and cnt.numel() == 4 * U
    dec, score = _sad_out(U, T, x.device)
    upd = torch.zeros((U,), dtype=torch.int32, device=x.device) if return_updates else None
    check(_lib.dsr_sad_energy_run(_dev(x), nf, U, T, dim, float(threshold), int(headN), int(tailN), int(hist.shape[1]), _dev(hist), _dev(cnt), _dev(dec), _dev(score),
                                  _dev(upd) if return_updates else None, cur_stream()))
    return (dec, score, state) + ((upd,) if return_updates else ())


def sad_energy_percentile(state, percentile=50.0, u=0):
    """EnergyVADMetric::energyPercentile of utterance u's history"""
    h = np.ascontiguousarray(state[0][u].cpu().numpy()); v = f64(0.0)
    check(load().dsr_sad_energy_percentile(_ptr(h), int(h.size), float(percentile), C.byref(v)))
    return v.value


def sad_simple_energy(X, threshold, gamma=0.98, state=None, nframes=None):
    """SimpleEnergyVAD: X cuda complex128 [U][Tmax][fftLen] -> (decision float64 [U][Tmax] (1.0 speech, 0.0 not), score = e / E, state);
    state: E float64 [U] (None: zeros, nextSpeaker()), updated in place"""
    import torch
    load(); (U, T, N), nf = _batch(X, nframes, torch.complex128)
    if state is None:
        state = torch.zeros((U,), dtype=torch.float64, device=X.device)
    assert state.dtype == torch.float64 and state.numel() == U
    dec, score = _sad_out(U, T, X.device)
    check(_lib.dsr_sad_simple_energy_run(_dev(X), nf, U, T, N, float(threshold), float(gamma), _dev(state), _dev(dec), _dev(score), cur_stream()))
    return dec, score, state


def sad_band(fftLen, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0):
    """(lowX, highX, binN) of MultiChannelVADMetric; a cutoff at or above sampleRate / 2 is a dimension error as there"""
    lo, hi, bn = C.c_uint(0), C.c_uint(0), C.c_uint(0)
    check(load().dsr_sad_band(int(fftLen), float(sampleRate), float(lowCutoff), float(highCutoff), C.byref(lo), C.byref(hi), C.byref(bn)))
    return lo.value, hi.value, bn.value


SAD_POWER_RATIO, SAD_ENERGY_RATIO, SAD_TSPS = 0, 1, 2


def sad_power(P, fftLen, kind=SAD_POWER_RATIO, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, E0=None, nframes=None):
    """PowerSpectrumVADMetric (kind 0), NormalizedEnergyMetric (1), TSPSVADMetric (2): P cuda float32 [U][C][Tmax][fftLen/2+1], channel 0 the
    target -> (decision float64 [U][Tmax] +-1, powers float64 [U][Tmax][C], score float64 [U][Tmax])"""
    import torch
    load()
    assert P.dim() == 4 and P.dtype == torch.float32 and P.is_contiguous() and P.shape[3] == fftLen // 2 + 1
    U, Cn, T, F = P.shape
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    lo, hi, _ = sad_band(fftLen, sampleRate, lowCutoff, highCutoff)
    if E0 is None:
        E0 = 5000.0 if kind == SAD_TSPS else 1.0
    dec, score = _sad_out(U, T, P.device)
    pw = torch.zeros((U, T, Cn), dtype=torch.float64, device=P.device)
    check(_lib.dsr_sad_power_run(_dev(P), _dev(nframes) if nframes is not None else None, U, Cn, T, int(fftLen), lo, hi, int(kind), float(E0), _dev(dec), _dev(pw),
                                 _dev(score), cur_stream()))
    return dec, pw, score


def sad_ccc(X, nCand, threshold=0.1, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, band=None, nframes=None, return_candidates=False):
    """CCCVADMetric: X cuda complex64 or complex128 [U][C][Tmax][fftLen], channel 0 the reference -> (decision float64 [U][Tmax] (1.0 where
    score < threshold, else -1.0), score float64 [U][Tmax]).  band = (lowX, highX) overrides the cutoffs."""
    import torch
    load()
    assert X.dim() == 4 and X.dtype in (torch.complex64, torch.complex128) and X.is_contiguous()
    U, Cn, T, N = X.shape
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    lo, hi = band if band is not None else sad_band(N, sampleRate, lowCutoff, highCutoff)[:2]
    dec, score = _sad_out(U, T, X.device)
    cands = torch.zeros((U, T, int(nCand)), dtype=torch.float64, device=X.device) if return_candidates else None
    check(_lib.dsr_sad_ccc_run(_dev(X), 1 if X.dtype == torch.complex128 else 0, _dev(nframes) if nframes is not None else None, U, Cn, T, N, int(lo), int(hi),
                               int(nCand), float(threshold), _dev(dec), _dev(score), _dev(cands) if return_candidates else None, cur_stream()))
    return (dec, score) + ((cands,) if return_candidates else ())


SAD_HANGOVER, SAD_HANGOVER_MI, SAD_HANGOVER_MULTISTAGE = 0, 1, 2


def sad_hangover(decisions, thresholds=(0.5,), headN=4, tailN=10, kind=SAD_HANGOVER, nframes=None):
    """The hangover segmenters' rule over K metrics' decisions: cuda float64 [K][U][Tmax] -> (start, length, consumed int32 [U],
    decisionMetric int32 [U][Tmax])"""
    import torch
    load()
    assert decisions.dim() == 3 and decisions.dtype == torch.float64 and decisions.is_contiguous()
    K, U, T = decisions.shape
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == U and nframes.is_contiguous())
    thr = _np(list(thresholds) + [0.5] * (K - len(thresholds)), np.float64)
    out = [torch.zeros((U,), dtype=torch.int32, device=decisions.device) for _ in range(3)]
    dm = torch.zeros((U, T), dtype=torch.int32, device=decisions.device)
    check(_lib.dsr_sad_hangover_run(_dev(decisions), _dev(nframes) if nframes is not None else None, K, U, T, _ptr(thr), int(headN), int(tailN), int(kind),
                                    _dev(out[0]), _dev(out[1]), _dev(out[2]), _dev(dm), cur_stream()))
    return out[0], out[1], out[2], dm


def sad_gather(x, start, length):
    """the segment's frames packed: x cuda float32 [U][Tmax][dim] -> [U][Tmax][dim], rows start[u] .. start[u] + length[u] - 1 first, zeros after"""
    import torch
    load(); (U, T, dim), _ = _batch(x, None)
    assert start.dtype == torch.int32 and length.dtype == torch.int32 and start.numel() == U and length.numel() == U
    y = torch.zeros((U, T, dim), dtype=torch.float32, device=x.device)
    check(_lib.dsr_sad_gather_run(_dev(x), _dev(start), _dev(length), U, T, dim, _dev(y), cur_stream()))
    return y


SAD_ENERGY_DIFFUSION, SAD_BAND_ENERGY_RATIO, SAD_NEGATIVE_ENTROPY, SAD_SIGNIFICANT_SUBBANDS = 0, 1, 2, 3


def sad_shape(x, op, sampleRate=16000.0, thresh=0.0, nframes=None):
    """The spectral-shape operators of btk/sad/sadFeature.cc: x cuda float32 [U][Tmax][dim] -> float32 [U][Tmax][1].  op: SAD_ENERGY_DIFFUSION,
    SAD_BAND_ENERGY_RATIO (thresh = threshF in Hz, 0: sampleRate / 4), SAD_NEGATIVE_ENTROPY, SAD_SIGNIFICANT_SUBBANDS (thresh on the normalised frame)"""
    import torch
    load(); (U, T, dim), nf = _batch(x, nframes)
    y = torch.zeros((U, T, 1), dtype=torch.float32, device=x.device)
    check(_lib.dsr_sad_shape_run(_dev(x), nf, U, T, dim, int(op), float(sampleRate), float(thresh), _dev(y), cur_stream()))
    return y


SAD_NEGENTROPY, SAD_MUTUAL_INFORMATION, SAD_LIKELIHOOD_RATIO = 0, 1, 2


def sad_read_shape_factors(directory, fftLen):
    """the per-bin shape factors of the reference's directory of _M-%04d files: float64 [fftLen/2+1]"""
    sf = np.zeros(fftLen // 2 + 1, np.float64)
    check(load().dsr_sad_gg_read_shape_factors(str(directory).encode(), int(fftLen), _ptr(sf)))
    return sf


class SadGG(object):
    """The host-side model of NegentropyVADMetric / MutualInformationVADMetric / LikelihoodRatioVADMetric: shapeFactors float64 [fftLen/2+1], a
    directory of _M-%04d files, or None (all 2.0, the Gaussian).  joint: also the matched joint pdfs and the fixed threshold of the mutual
    information (DsrError JNUMERIC where the bisection does not converge in 200 steps)."""

    def __init__(self, fftLen, shapeFactors=None, sampleRate=16000.0, lowCutoff=-1.0, highCutoff=-1.0, joint=True):
        load(); self.h = vp(); self.fftLen = int(fftLen); self.F = self.fftLen // 2 + 1
        if isinstance(shapeFactors, (str, bytes, os.PathLike)):
            shapeFactors = None if str(shapeFactors) == "" else sad_read_shape_factors(shapeFactors, fftLen)
        sf = None if shapeFactors is None else _np(shapeFactors, np.float64)
        assert sf is None or sf.size == self.F
        check(_lib.dsr_sad_gg_create(_ptr(sf) if sf is not None else None, self.fftLen, float(sampleRate), float(lowCutoff), float(highCutoff), 1 if joint else 0,
                                     C.byref(self.h)))
        self.table = np.zeros((self.F, 6), np.float64); ft = f64(0.0)
        check(_lib.dsr_sad_gg_table(self.h, _ptr(self.table), C.byref(ft))); self.fixedThreshold = ft.value

    def __del__(self):
        try:
            if getattr(self, "h", None):
                _lib.dsr_sad_gg_destroy(self.h)
        except Exception:
            pass

    def rho_state(self, U, device="cuda:0"):
        """rho after nextSpeaker(): complex128 zeros [U][fftLen/2+1]"""
        import torch
        return torch.zeros((U, self.F), dtype=torch.complex128, device=device)

    def run(self, kind, X1, env1, X2=None, env2=None, twiddle=-1.0, threshold=None, beta=0.95, rho=None, nframes=None, return_threshold=False):
        """X cuda complex128 [U][Tmax][fftLen], env cuda float32 [U][Tmax][>= fftLen/2+1] -> (decision, score) float64 [U][Tmax]; the mutual
        information also returns rho (updated in place; None: zeros) and, with return_threshold, the threshold of every frame"""
        import torch
        (U, T, N), nf = _batch(X1, nframes, torch.complex128)
        assert N == self.fftLen and env1.dim() == 3 and env1.dtype == torch.float32 and env1.is_contiguous() and env1.shape[:2] == (U, T)
        if kind != SAD_NEGENTROPY:
            assert X2.shape == X1.shape and X2.dtype == torch.complex128 and X2.is_contiguous() and env2.shape == env1.shape and env2.dtype == torch.float32 and env2.is_contiguous()
        if threshold is None:
            threshold = (0.5, 1.3, 0.0)[kind]
        if kind == SAD_MUTUAL_INFORMATION and rho is None:
            rho = self.rho_state(U, X1.device)
        assert rho is None or (rho.dtype == torch.complex128 and rho.shape == (U, self.F) and rho.is_contiguous())
        dec, score = _sad_out(U, T, X1.device)
        thr = torch.zeros((U, T), dtype=torch.float64, device=X1.device) if return_threshold else None
        check(_lib.dsr_sad_gg_run(self.h, int(kind), _dev(X1), _dev(X2) if X2 is not None else None, _dev(env1), _dev(env2) if env2 is not None else None, env1.shape[2], nf,
                                  U, T, float(twiddle), float(threshold), float(beta), _dev(rho) if rho is not None else None, _dev(dec), _dev(score),
                                  _dev(thr) if return_threshold else None, cur_stream()))
        out = (dec, score) + ((rho,) if kind == SAD_MUTUAL_INFORMATION else ()) + ((thr,) if return_threshold else ())
        return out
