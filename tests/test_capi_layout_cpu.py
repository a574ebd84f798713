"""CPU tests of the binding's layout: dsr._capi is a package of one module per reference module behind a façade that keeps every name the
single file had (test_capi_layout_cpu_names.txt, recorded from that file), importing it does not import torch, the three records take their
fields from include/dsr.h, and the ownership of a handle is stated once, in the handle base."""
import ctypes as C
import importlib
import inspect
import os
import pkgutil
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT, PKG

CAPI_DIR = os.path.join(PKG, "dsr", "_capi")
PARENT_LINES = 3157                                       # dsr/_capi.py when it was one file

i, u, q, f, d = C.c_int, C.c_uint32, C.c_int64, C.c_float, C.c_double
MFCC_CFG = [("blockLen", i), ("shiftLen", i), ("padZeros", i), ("mu", d), ("fftLen", i), ("powN", i), ("vtlnRatio", d), ("vtlnEdge", d),
            ("vtlnVersion", i), ("rate", f), ("low", f), ("up", f), ("filterN", i), ("melVersion", i), ("logM", d), ("logA", d),
            ("sphinxFlooring", i), ("ncep", i), ("dctType", i), ("cmnMode", i), ("devNormFactor", d), ("delta", i), ("outDim", i)]
DECODER_CFG = [("beam", d), ("lmScale", d), ("lmPenalty", d), ("silPenalty", d), ("silenceX", u), ("maxActive", i), ("maxCandidates", i),
               ("arenaTokens", q), ("streams", i), ("topN", i), ("latticeTokens", q), ("wordTrace", i), ("propagateN", i), ("fastHash", i),
               ("insertSilence", i), ("wordTraceLattice", i), ("wordTraces", q)]
DECODE_RESULT = [("score", d), ("ac", f), ("lm", f), ("frames", i), ("reachedFinal", i), ("nArcs", i), ("nWords", i), ("status", i),
                 ("maxActiveSeen", i), ("activeHypos", q), ("placements", q), ("registerFrames", q), ("finalStatesN", i), ("laidOutFrames_", i)]


def _kind(v):
    return "class" if inspect.isclass(v) else "function" if inspect.isfunction(v) else "other"


def _modules():
    return [importlib.import_module("dsr._capi." + m.name) for m in pkgutil.iter_modules([CAPI_DIR])]


def test_facade_keeps_every_name_of_the_single_file(dsr):
    recorded = [line.split() for line in open(os.path.join(ROOT, "tests", "test_capi_layout_cpu_names.txt")).read().splitlines()]
    assert len(recorded) == 169 and sum(not n.startswith("_") for n, _ in recorded) == 153
    missing = [n for n, _ in recorded if n != "C_" and not hasattr(dsr, n)]
    assert missing == []
    changed = [(n, k, _kind(getattr(dsr, n))) for n, k in recorded if n != "C_" and _kind(getattr(dsr, n)) != k]
    assert changed == []
    assert isinstance(dsr._lib, C.CDLL) and dsr._lib is dsr.load()                     # live: what load() bound, not the None of import time


def test_import_binds_no_library_and_no_torch():
    code = ("import sys; sys.path.insert(0, %r); import dsr._capi as K; assert 'torch' not in sys.modules, 'torch imported'; "
            "assert K._lib is None; print('ok')" % PKG)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr


@pytest.mark.parametrize("cls,fields,size", [("MfccCfg", MFCC_CFG, 120), ("DecoderCfg", DECODER_CFG, 104), ("DecodeResult", DECODE_RESULT, 72)])
def test_records_come_from_the_header_with_the_layout_they_had(dsr, cls, fields, size):
    S = getattr(dsr, cls)
    assert [n for n, _ in S._fields_] == [n for n, _ in fields]
    assert list(S._fields_) == fields and C.sizeof(S) == size


def test_default_configurations_through_header_derived_records(dsr):
    L = dsr.load()
    m = dsr.MfccCfg(); L.dsr_mfcc_default_cfg(C.byref(m))
    assert (m.blockLen, m.shiftLen, m.fftLen, m.ncep) == (320, 160, 512, 13)
    c = dsr.DecoderCfg(); L.dsr_decoder_default_cfg(C.byref(c))
    assert (c.beam, c.lmScale) == (100.0, 12.0)


def test_struct_parser(dsr):
    from dsr._capi import _core
    s = _core.header_structs("typedef struct { double a, b; int c;  /* two declarations */\n  uint32_t d; // one\n} rec;\ntypedef struct x x;\n")
    assert s == {"rec": [("a", d), ("b", d), ("c", i), ("d", u)]}
    for text in ("typedef struct { int a; wchar_t b; } rec;", "typedef struct { int a; float* p; } rec;", "typedef struct { int a[3]; } rec;"):
        with pytest.raises(ValueError):
            _core.header_structs(text)


def _counted(monkeypatch, L, name):
    real, calls = getattr(L, name), []
    monkeypatch.setattr(L, name, lambda h: (calls.append(h.value), real(h))[1])       # the entry on the loaded library object, counted
    return calls


def test_constructor_that_raised_leaves_nothing_to_destroy(dsr, monkeypatch, tmp_path):
    L = dsr.load()
    fb, fsa, pt = _counted(monkeypatch, L, "dsr_fb_destroy"), _counted(monkeypatch, L, "dsr_fsa_destroy"), _counted(monkeypatch, L, "dsr_param_tree_destroy")
    o = dsr.FilterBank.__new__(dsr.FilterBank)
    with pytest.raises(dsr.DsrError):
        o.__init__(np.zeros(1000), 256, 4, 1)                                       # refused before the create call
    assert not o.h
    o.__del__(); del o
    o = dsr.Fsa.__new__(dsr.Fsa)
    with pytest.raises(AttributeError):
        o.__init__(gmm=None)                                                        # raises before the create call, _owner already set
    o.__del__(); del o
    o = dsr.ParamTree.__new__(dsr.ParamTree)
    with pytest.raises(dsr.DsrError):
        o.__init__(str(tmp_path / "missing.mllr"))                                  # the create call itself fails
    assert not o.h
    o.__del__(); del o
    assert fb == [] and fsa == [] and pt == []


def test_created_handle_is_destroyed_once_and_borrowed_never(dsr, monkeypatch):
    L = dsr.load()
    wf, pt = _counted(monkeypatch, L, "dsr_wfst_destroy"), _counted(monkeypatch, L, "dsr_param_tree_destroy")
    w = dsr.Wfst(); w.add_arc(0, 1, 1, 1, 0.5); hw = w.h.value
    del w
    assert wf == [hw]
    t = dsr.ParamTree(); t.set(2, np.eye(2, 3)); ht = t.h.value
    b = dsr.ParamTree(handle=t.h, owner=t)
    assert b.hasIndex(2) and b._owner is t
    del b
    assert pt == []                                                                 # borrowed: the owner destroys it
    del t
    assert pt == [ht]


def test_ownership_is_written_once(dsr):
    from dsr._capi import _core
    protos = dsr.header_prototypes()
    owners = 0
    for m in _modules():
        for name, cls in inspect.getmembers(m, inspect.isclass):
            if cls.__module__ != m.__name__:
                continue
            assert "__del__" not in vars(cls) or cls is _core.Handle, name
            if issubclass(cls, _core.Handle) and cls is not _core.Handle and "_destroy" in vars(cls):
                owners += 1
                assert cls._destroy in protos and cls._destroy.endswith("_destroy"), name
    assert owners == 36                                                             # the classes that each had a __del__ of their own


def test_no_module_is_large_and_the_package_is_smaller_than_the_file_was():
    sizes = {fn: len(open(os.path.join(CAPI_DIR, fn)).read().splitlines()) for fn in os.listdir(CAPI_DIR) if fn.endswith(".py")}
    assert len(sizes) >= 10 and max(sizes.values()) <= 800, sizes
    assert sum(sizes.values()) < PARENT_LINES, sizes
