"""What every module of the binding shares: the library and its signatures (both from include/dsr.h), the error type, the handle base and the
marshalling helpers.  The modules reach the loaded library as _core._lib: load() rebinds it, a from-import would keep the None."""
import ctypes as C
import os
import re

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.dirname(os.path.dirname(_HERE))
_LIBPATH = os.path.join(_PKG, "lib", "libdsr_hip.so")
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


_HEADER = os.path.join(os.path.dirname(_PKG), "include", "dsr.h")
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


_STRUCT = r"typedef\s+struct\s*\{(.*?)\}\s*(\w+)\s*;"


def _code(text):
    """the header without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^\s*#.*$", " ", text, flags=re.M)


def header_prototypes(path=None):
    """{name: (restype, [argtypes])} for every function include/dsr.h declares -- the single source of the ctypes signatures, so that no
    entry point is ever called with libffi's default int promotion (a 64-bit stride passed as a 32-bit int reads stack garbage)."""
    text = _code(open(path or _HEADER).read())
    text = re.sub(_STRUCT, " ", text, flags=re.S)
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


def header_structs(text=None):
    """{name: _fields_} for every `typedef struct { ... } name;` of include/dsr.h (or of the header text given) -- the single source of the
    records' layouts, as header_prototypes is of the signatures.  Scalar fields only; `double a, b; int c;` declares three."""
    out = {}
    for m in re.finditer(_STRUCT, _code(open(_HEADER).read() if text is None else text), flags=re.S):
        fields = []
        for decl in filter(str.strip, m.group(1).split(";")):
            if "*" in decl or "[" in decl:
                raise ValueError("include/dsr.h: cannot map field %r of %s" % (decl.strip(), m.group(2)))
            first, *more = decl.split(",")                 # the type stands with the first name
            t = _ctype_of(first)
            fields += [(n.strip(), t) for n in [first.split()[-1]] + more]
        out[m.group(2)] = fields
    return out


_STRUCTS = header_structs()


class MfccCfg(C.Structure):
    _fields_ = _STRUCTS["dsr_mfcc_cfg"]


class DecoderCfg(C.Structure):
    _fields_ = _STRUCTS["dsr_decoder_cfg"]


class DecodeResult(C.Structure):
    _fields_ = _STRUCTS["dsr_decode_result"]


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


class Handle:
    """Owner of one opaque handle of the library.  A subclass names its destroy entry in _destroy and makes the handle with _create, or
    takes one over by assigning self.h; one that wraps a handle something else owns sets self._owner to that owner, which also keeps the
    owner alive.  Destroyed is what was created and is owned: nothing after a constructor that raised before or inside its create call,
    nothing for a borrowed handle, nothing once the library is gone at interpreter exit."""
    _destroy = None
    _owner = None
    h = None

    def _create(self, fn, *args):
        """call a create entry, whose last parameter is the handle it returns"""
        h = vp(); check(fn(*args, C.byref(h))); self.h = h

    def __del__(self):
        if _lib is not None and self.h and self._owner is None:
            getattr(_lib, self._destroy)(self.h)


class _Torch:
    """torch, imported at first use: importing the binding does not import it (load() does, just before it opens the library)"""

    def __getattr__(self, name):
        import torch
        return getattr(torch, name)


torch = _Torch()


def cur_stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _np(a, dt):
    return np.ascontiguousarray(a, dtype=dt)


def _ptr(a):
    return a.ctypes.data_as(vp)


def _dev(t):
    return C.c_void_p(t.data_ptr())


def _nf(nframes):
    return _dev(nframes) if nframes is not None else None


def _counts(n, U, full, device):
    """a per-utterance count vector, cuda int32 [U]; None: every utterance is full length"""
    return torch.full((U,), full, dtype=torch.int32, device=device) if n is None else n


def _state(nbytes, device):
    return torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=device)


def _batch(x, nframes, dtype=None):
    """shape and count pointer of a batch of whole utterances [U][Tmax][dim] (the operators of btk/feature and btk/sad)"""
    assert x.dim() == 3 and x.dtype == (dtype or torch.float32) and x.is_contiguous()
    assert nframes is None or (nframes.dtype == torch.int32 and nframes.numel() == x.shape[0] and nframes.is_contiguous())
    return x.shape, _nf(nframes)
