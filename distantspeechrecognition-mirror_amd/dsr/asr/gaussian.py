"""asr.gaussian: CodebookSetBasicPtr / DistribSetBasicPtr (gaussian.i:281-283,465-467) for 1:1 distribution/codebook models, over dsr_gmm_* and
dsr_distribset_* (include/dsr.h sections 4 and 8); DistribMapPtr / DistribMultiStreamPtr / DistribSetMultiStreamPtr (distribBasic.h:135-158, 390-408)
over section 8b."""
import ctypes as C

import numpy as np

from .. import _capi as K


def _desc(path):
    rows = []
    for line in open(path):
        if line[:1] == ";" or not line.split():
            continue
        rows.append(line.split())
    return rows


class CodebookSetBasicPtr(object):
    """descFile lines: name featureName refN dimN covType (codebookBasic.cc:804-828); cbkFile: big-endian set file."""

    def __init__(self, descFile="", fs=None, cbkFile=""):
        self._desc = _desc(descFile) if descFile else []
        self._fs, self._cbkFile = fs, cbkFile
        self.names = [r[0] for r in self._desc]
        self.featureName = self._desc[0][1] if self._desc else None

    def ncbks(self):
        return len(self._desc)

    def feature(self):
        return self._fs.feature(self.featureName)


class DistribBasicPtr(object):
    """Distrib::score(frameX) (distribBasic.h:48-50) of one distribution of a set"""

    def __init__(self, dss, distX):
        self._dss, self._x = dss, distX

    def name(self):
        return K.load().dsr_distribset_name(self._dss._ds, self._x).decode()

    def score(self, frameX):
        s = C.c_float(); st = K.load().dsr_distribset_score(self._dss._ds, self._x, int(frameX), C.byref(s))
        if st == K.E_ITERATOR:
            raise StopIteration
        K.check(st); return s.value


class DistribSetBasicPtr(object):
    """descFile lines: name codebookName (distribBasic.cc:218-232); distFile: big-endian set file."""

    def __init__(self, cbs, descFile="", distFile="", gmmMode=0):
        self._cbs = cbs; self._desc = _desc(descFile) if descFile else []
        self.names = [r[0] for r in self._desc]
        self.gmm = K.Gmm(files=(cbs._cbkFile, distFile)); cbs._gmm = self.gmm
        if self._desc and len(self._desc) != self.gmm.K:
            raise K.DsrError(4, "%d distributions described, %d in the file" % (len(self._desc), self.gmm.K))
        self._feat = cbs.feature(); self._ds = C.c_void_p()
        K.check(K.load().dsr_distribset_create(self.gmm.h, self._feat._h, int(gmmMode), C.byref(self._ds)))

    def __del__(self):
        try:
            if getattr(self, "_ds", None):
                K.load().dsr_distribset_destroy(self._ds)
        except Exception:
            pass

    def ndists(self):
        return self.gmm.K

    def index(self, name):
        x = C.c_int(); K.check(K.load().dsr_distribset_find(self._ds, name.encode(), C.byref(x))); return x.value

    def find(self, key):
        """find(name) / find(dsX) (distribBasic.h:183-190)"""
        x = self.index(key) if isinstance(key, str) else int(key)
        if not 0 <= x < self.gmm.K:
            raise K.DsrError(6, "distribution %d of %d" % (x, self.gmm.K))
        return DistribBasicPtr(self, x)

    def resetCache(self):
        K.check(K.load().dsr_distribset_reset_cache(self._ds))

    def resetFeature(self):
        K.check(K.load().dsr_distribset_reset_feature(self._ds))

    def score_all_frames(self, feats, mode=0):
        """feats: cuda float32 [T][dimN] -> costs [T][ndists] (row t = Distrib::score(t) of every distribution)."""
        return self.gmm.score(feats, mode=mode, want_argmin=False)[0]


class DistribMapPtr(object):
    """DistribMap (distribBasic.h:390-408, gaussian.i): add / mapped / read / write over dsr_distribmap_* (include/dsr.h section 8b)"""

    def __init__(self):
        from .. import _ms
        self._map = _ms.DistribMap()

    def add(self, fromName, toName):
        self._map.add(fromName, toName)

    def mapped(self, name):
        return self._map.mapped(name)

    __getitem__ = mapped

    def __len__(self):
        return len(self._map)

    def read(self, fileName):
        self._map.read(fileName)

    def write(self, fileName):
        self._map.write(fileName)


class DistribMultiStreamPtr(DistribBasicPtr):
    """DistribMultiStream (distribBasic.h:135-158): score(frameX) = audioWeight * audio score + videoWeight * video score"""

    def audioWeight(self):
        return self._dss.weights()[0]

    def videoWeight(self):
        return self._dss.weights()[1]


class DistribSetMultiStreamPtr(object):
    """DistribSetMultiStream(audioDistSet, videoDistSet[, distribMap], audioWeight, videoWeight) (distribBasic.cc:381-410): the audio set's
    distributions, names and order; the partner of `name` is videoDistSet.find(name), or videoDistSet.find(distribMap.mapped(name)).  Decoders and
    lattices take it wherever they take a DistribSetBasicPtr."""

    def __init__(self, audioDss, videoDss, distribMap=None, audioWeight=0.95, videoWeight=0.05):
        self._audio, self._video, self._map = audioDss, videoDss, distribMap          # kept: the set's children outlive it
        self.names = [audioDss.find(k).name() for k in range(audioDss.ndists())]
        self._ds = C.c_void_p()
        K.check(K.load().dsr_distribset_create_multistream(audioDss._ds, videoDss._ds, distribMap._map.h if distribMap is not None else None,
                                                           float(audioWeight), float(videoWeight), C.byref(self._ds)))

    def __del__(self):
        try:
            if getattr(self, "_ds", None):
                K.load().dsr_distribset_destroy(self._ds)
        except Exception:
            pass

    def ndists(self):
        return K.load().dsr_distribset_ndists(self._ds)

    def index(self, name):
        x = C.c_int(); K.check(K.load().dsr_distribset_find(self._ds, name.encode(), C.byref(x))); return x.value

    def find(self, key):
        x = self.index(key) if isinstance(key, str) else int(key)
        if not 0 <= x < self.ndists():
            raise K.DsrError(6, "distribution %d of %d" % (x, self.ndists()))
        return DistribMultiStreamPtr(self, x)

    __getitem__ = find

    def __iter__(self):
        return (self.find(k) for k in range(self.ndists()))

    def weights(self):
        a, v = C.c_double(), C.c_double(); K.check(K.load().dsr_distribset_get_weights(self._ds, C.byref(a), C.byref(v))); return a.value, v.value

    def setWeights(self, audioWeight, videoWeight):
        K.check(K.load().dsr_distribset_set_weights(self._ds, float(audioWeight), float(videoWeight)))

    def resetCache(self):
        K.check(K.load().dsr_distribset_reset_cache(self._ds))

    def resetFeature(self):
        K.check(K.load().dsr_distribset_reset_feature(self._ds))
