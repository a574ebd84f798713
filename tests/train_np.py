"""numpy restatement of asr/train's CodebookTrain / DistribTrain for diagonal 1:1 models (asr/train/codebookTrain.cc "cT",
asr/train/distribTrain.cc "dT", asr/gaussian/codebookBasic.cc "cB"): the yardstick of the training tests.

Float / double placement is spelled out: np.float32 products where the reference multiplies floats, Python floats (fp64) for its double
accumulators, sums sequential in item order, exp / log from the C library through `math`.  Nothing here is taken from the reference's text.
Layout as in the library: Gaussians of all codebooks in one run, codebook k owning rows off[k]..off[k+1]."""
import math
import struct

import numpy as np

f32 = np.float32
PADDING = 1.0e-4                     # dT:144
VAR_FLOOR = f32(1.0e-4)              # cT:732
CB_MARKER, DS_MARKER = 123456789, 987654321
END_OF_ACCS = "EndOfAccumulators"    # distribTrain.h:230-233


class NumericError(Exception):
    """jnumeric_error of cT:97-98 (and the zero / non-finite posterior sum the library refuses as well)"""


class ConsistencyError(Exception):
    pass


class ParameterError(Exception):
    pass


class DimensionError(Exception):
    pass


class Model(object):
    def __init__(self, refN, mean, cv, det, val, scale=None, count=None, cbNames=None, dsNames=None):
        self.refN = [int(r) for r in refN]; self.K = len(self.refN)
        self.mean = np.array(mean, f32).reshape(sum(self.refN), -1); self.D = self.mean.shape[1]
        self.cv = np.array(cv, f32).reshape(self.mean.shape); self.det = np.array(det, f32).reshape(-1); self.val = np.array(val, f32).reshape(-1)
        self.scale = np.ones(self.K, f32) if scale is None else np.array(scale, f32)
        self.count = np.ones(len(self.det), f32) if count is None else np.array(count, f32)
        self.cbNames = list(cbNames) if cbNames else ["cb%d" % k for k in range(self.K)]
        self.dsNames = list(dsNames) if dsNames else ["ds%d" % k for k in range(self.K)]
        self._off()

    def _off(self):
        self.off = [0]
        for r in self.refN:
            self.off.append(self.off[-1] + r)
        self.G = self.off[-1]

    def copy(self):
        return Model(self.refN, self.mean.copy(), self.cv.copy(), self.det.copy(), self.val.copy(), self.scale.copy(), self.count.copy(), self.cbNames, self.dsNames)

    def as_kwargs(self):
        return dict(refN=np.array(self.refN, np.int32), mean=self.mean, ivar=self.cv, det=self.det, val=self.val, scale=self.scale)


def posterior(m, x, k, info=None):
    """_scoreAll with addCount (cB:645-766) + the normalisation of cT:100-105 -> (float score, float32 posteriors [refN]).
    info (a dict) collects the exponents compared with the -100 cutoff."""
    a, b = m.off[k], m.off[k + 1]; R = b - a; sc = m.scale[k]
    x = np.asarray(x, f32)
    pi = f32(math.log(2.0 * math.pi) * m.D)                                  # float _pi (cB:170)
    dist = (pi + m.det[a:b]).astype(np.float64)                              # float + float, then the double accumulator
    for d in range(m.D):
        diff = (m.mean[a:b, d] - x[d]).astype(np.float64)                    # float difference into a double
        dist = dist + diff * diff * m.cv[a:b, d].astype(np.float64)
    logdist = (0.5 * dist).astype(f32)
    minlog = 1e20
    for r in range(R):
        if float(logdist[r]) < minlog:
            minlog = float(logdist[r])
    mix = np.zeros(R, f32)
    if R == 1:
        mix[0] = 1.0
        score = f32(sc * f32(logdist[0] + m.val[a]))
        s = 1.0
    else:
        s = 0.0
        for r in range(R):
            e = float(sc) * (minlog - float(logdist[r]))
            if info is not None:
                info.setdefault("exps", []).append(e)
            if e > -100.0:
                mix[r] = f32(math.exp(e - float(f32(sc * m.val[a + r]))))
                s += float(mix[r])
        if not (s > 0.0) or math.isinf(s):
            raise NumericError("posterior sum %r" % s)
        score = f32(float(sc) * minlog - math.log(s))
    if math.isnan(float(score)):
        raise NumericError("Utterance log-likelihood is NaN")
    tot = 0.0
    for r in range(R):
        tot += float(mix[r])
    for r in range(R):
        mix[r] = f32(float(mix[r]) / tot)
    return score, mix


class Accu(object):
    """the six accumulators of a model (fp64), optionally with the sums of the terms' magnitudes and the item counts the tolerance needs"""

    NAMES = ("count", "den", "sumO", "sumOsq", "dcount", "dden")

    def __init__(self, m, minCount=5.0, track=False):
        self.m, self.minCount, self.track = m, float(minCount), track
        self.zero()

    def zero(self):
        G, D = self.m.G, self.m.D
        self.count = np.zeros(G); self.den = np.zeros(G); self.sumO = np.zeros((G, D)); self.sumOsq = np.zeros((G, D))
        self.dcount = np.zeros(G); self.dden = np.zeros(G)
        if self.track:
            self.absG = np.zeros(G); self.absO = np.zeros((G, D)); self.absOsq = np.zeros((G, D)); self.n = np.zeros(G, np.int64)

    def arrays(self):
        return [getattr(self, n) for n in self.NAMES]

    # ---- one item: DistribTrain::accumulate (dT:74-80)
    def accumulate(self, x, k, factor, info=None):
        m = self.m; x = np.asarray(x, f32); factor = f32(factor)
        score, mix = posterior(m, x, k, info)
        a = m.off[k]
        for r in range(len(mix)):                                             # cT:520-540
            gamma = f32(mix[r] * factor)
            if gamma == 0.0:
                continue
            g = a + r
            if gamma > 0.0:
                self.count[g] += float(gamma)
            elif gamma < 0.0:
                self.den[g] -= float(gamma)
            t1 = (x * gamma).astype(np.float64); t2 = ((gamma * x) * x).astype(np.float64)     # float products, double adds
            self.sumO[g] += t1; self.sumOsq[g] += t2
            if self.track:
                self.absG[g] += abs(float(gamma)); self.absO[g] += np.abs(t1); self.absOsq[g] += np.abs(t2); self.n[g] += 1
        b = m.off[k + 1]
        if factor > 0.0:                                                      # dT:133-142
            self.dcount[a:b] += (factor * mix).astype(np.float64)
        else:
            self.dden[a:b] -= (factor * mix).astype(np.float64)
        return score

    def accumulate_items(self, x, frame, dist, factor, info=None):
        return np.array([self.accumulate(x[f], k, w, info) for f, k, w in zip(frame, dist, factor)], f32)

    def accumulate_path(self, x, ids, factor):
        """DistribSetTrain::accumulate (dT:515-526)"""
        score = 0.0
        for t, k in enumerate(ids):
            score += float(self.accumulate(x[t], int(k), factor))
        return score

    @staticmethod
    def lattice_items(edges, gamma, live, factor, K, T):
        """the items of accumulateLattice (dT:528-561): edges = dict of start / end / in arrays, live = the links the edge iterator sees"""
        frame, dist, fac, cnt = [], [], [], 0
        for e in range(len(gamma)):
            if not live[e] or edges["in"][e] == 0 or gamma[e] > 10.0:
                continue
            post = f32(float(f32(factor)) * math.exp(-float(gamma[e])))
            assert 0 <= edges["start"][e] and edges["end"][e] < T and edges["in"][e] - 1 < K
            cnt += 1
            for f in range(int(edges["start"][e]), int(edges["end"][e]) + 1):
                frame.append(f); dist.append(int(edges["in"][e]) - 1); fac.append(post)
        return np.array(frame, np.int32), np.array(dist, np.int32), np.array(fac, f32), cnt

    def add(self, o, factor):
        """cT:392-405 (scaled), dT:254-262 (the factor is ignored)"""
        f = float(factor)
        dc, dd = o.dcount.copy(), o.dden.copy()
        self.count += f * o.count; self.den += f * o.den; self.sumO += f * o.sumO; self.sumOsq += f * o.sumOsq
        self.dcount += dc; self.dden += dd

    # ---- updates
    def _range(self, nParts, part):
        if nParts < 1 or part < 1 or part > nParts:
            raise ParameterError("nParts/part")
        seg = self.m.K // nParts
        return (part - 1) * seg, (self.m.K if part == nParts else part * seg)

    def update(self, what=3, nParts=1, part=1):
        m = self.m; k0, k1 = self._range(nParts, part)
        if what & 1:                                                          # cT:448-490
            for g in range(m.off[k0], m.off[k1]):
                cnt = f32(self.count[g]); m.count[g] = cnt
                if float(cnt) <= self.minCount:
                    continue
                m.mean[g] = (self.sumO[g] / float(cnt)).astype(f32)
                mu = m.mean[g].astype(np.float64)
                m.cv[g] = ((self.sumOsq[g] / float(cnt)) - (mu * mu)).astype(f32)
        if what & 2:                                                          # dT:146-156
            for k in range(k0, k1):
                ttl = 0.0
                for g in range(m.off[k], m.off[k + 1]):
                    ttl += (float(self.dcount[g]) + PADDING)
                for g in range(m.off[k], m.off[k + 1]):
                    m.val[g] = f32(-math.log((float(self.dcount[g]) + PADDING) / ttl))

    def update_mmi(self, what=3, E=1.0, merialdo=False, nParts=1, part=1):
        m = self.m; k0, k1 = self._range(nParts, part)
        val = m.val.copy()
        if what & 2:
            for k in range(k0, k1):
                G = range(m.off[k], m.off[k + 1])
                num = [float(self.dcount[g]) for g in G]; den = [float(self.dden[g]) for g in G]; v = [float(val[g]) for g in G]
                n = len(num)
                if not merialdo:                                              # dT:166-190
                    C = PADDING
                    for i in range(n):
                        deriv = -(1.0 + PADDING) * ((num[i] - den[i]) * math.exp(v[i]))
                        if deriv > C:
                            C = deriv
                    cnts = [(num[i] - den[i]) + C * math.exp(-v[i]) for i in range(n)]
                else:                                                         # dT:192-222
                    tn = td = 0.0
                    for i in range(n):
                        tn += num[i] + PADDING; td += den[i] + PADDING
                    C = 0.0
                    for i in range(n):
                        deriv = -(1.0 + PADDING) * (((num[i] + PADDING) / tn) - ((den[i] + PADDING) / td))
                        if deriv > C:
                            C = deriv
                    cnts = [(((num[i] + PADDING) / tn) - ((den[i] + PADDING) / td) + C) * math.exp(-v[i]) + PADDING for i in range(n)]
                ttl = 0.0
                for c in cnts:
                    if c < 0.0:
                        raise ConsistencyError("Count (%g) is negative" % c)
                    ttl += c
                for i, g in enumerate(G):
                    q = cnts[i] / ttl
                    val[g] = f32(-math.log(q)) if q > 0.0 else (f32(np.inf) if q == 0.0 else f32(np.nan))
                    if math.isnan(float(val[g])):
                        raise ConsistencyError("Weight is NaN")
        if what & 1:                                                          # cT:448-456, 492-518
            for g in range(m.off[k0], m.off[k1]):
                cnt = f32(self.count[g]); m.count[g] = cnt
                if float(cnt) <= self.minCount:
                    m.cv[g] = (1.0 / m.cv[g].astype(np.float64)).astype(f32)
                    continue
                Dd = float(E) * float(self.den[g]); denom = float(self.count[g]) - float(self.den[g]) + Dd
                mu = m.mean[g].copy(); sigma = (1.0 / m.cv[g].astype(np.float64)).astype(f32)
                musum = (self.sumO[g] + mu.astype(np.float64) * Dd).astype(f32)
                muhat = (musum.astype(np.float64) / denom).astype(f32)
                sigmasum = (self.sumOsq[g] + (sigma + mu * mu).astype(np.float64) * Dd).astype(f32)
                sigmahat = (sigmasum.astype(np.float64) / denom - (muhat * muhat).astype(np.float64)).astype(f32)
                m.mean[g] = muhat; m.cv[g] = sigmahat
        m.val = val

    def floor_variances(self, nParts=1, part=1):
        """cT:786-798 -> (total, floored)"""
        m = self.m; k0, k1 = self._range(nParts, part)
        blk = m.cv[m.off[k0]:m.off[k1]]
        low = blk < VAR_FLOOR
        blk[low] = VAR_FLOOR
        return int(blk.size), int(low.sum())

    def fix_gconsts(self, nParts=1, part=1):
        m = self.m; k0, k1 = self._range(nParts, part)
        for g in range(m.off[k0], m.off[k1]):                                 # cT:228-241
            logDet = 0.0
            for d in range(m.D):
                v = float(m.cv[g, d])
                logDet += math.log(v) if v > 0.0 else (-math.inf if v == 0.0 else math.nan)
            if math.isnan(logDet):
                raise ConsistencyError("Determinant is NaN")
            m.det[g] = f32(logDet)

    def invert_variances(self, nParts=1, part=1):
        m = self.m; k0, k1 = self._range(nParts, part)
        sl = slice(m.off[k0], m.off[k1])
        with np.errstate(divide="ignore"):
            m.cv[sl] = (1.0 / m.cv[sl].astype(np.float64)).astype(f32)       # cT:218-223

    def split(self, k, minCount=0.0, splitFactor=0.2):
        """dT:92-109, cT:122-198 -> the Gaussian that was split; the new one is appended to codebook k"""
        m = self.m; a, R = m.off[k], m.refN[k]; minCount = f32(minCount); splitFactor = f32(splitFactor)
        maxIdx, maxCount = 0, m.count[a]
        for r in range(1, R):
            if m.count[a + r] > maxCount:
                maxCount, maxIdx = m.count[a + r], r
        if minCount > 0.0 and maxCount < minCount:
            raise ParameterError("maxCount < minCount")
        if R >= 256:
            raise DimensionError("256 Gaussians")
        src, at = a + maxIdx, a + R
        perturb = (float(splitFactor) / np.sqrt(m.cv[src].astype(np.float64))).astype(f32)
        new_mean = m.mean[src] - perturb; m.mean[src] = m.mean[src] + perturb
        m.mean = np.insert(m.mean, at, new_mean, axis=0); m.cv = np.insert(m.cv, at, m.cv[src], axis=0)
        m.det = np.insert(m.det, at, m.det[src])
        half = f32(float(m.count[src]) / 2.0); m.count[src] = half; m.count = np.insert(m.count, at, half)
        nval = f32(float(m.val[src]) + math.log(2.0)); m.val[src] = nval; m.val = np.insert(m.val, at, nval)
        m.refN[k] = R + 1; m._off()
        for name in self.NAMES:                                               # fresh accumulators for this codebook / distribution
            arr = getattr(self, name)
            arr = np.insert(arr, at, 0.0, axis=0); arr[a:at + 1] = 0.0
            setattr(self, name, arr)
        if self.track:
            for name in ("absG", "absO", "absOsq", "n"):
                arr = np.insert(getattr(self, name), at, 0, axis=0); arr[a:at + 1] = 0; setattr(self, name, arr)
        return maxIdx

    # ---- accumulator files (big-endian mach_ind_io)
    def save_codebook_accus(self, totalPr=0.0, totalT=0, countsOnly=False):
        """cT:625-647, 299-365, AccMap dT:357-373, 400-411 -> bytes"""
        m = self.m
        live = [bool(np.any(self.count[m.off[k]:m.off[k + 1]] != 0.0) or np.any(self.den[m.off[k]:m.off[k + 1]] != 0.0)) for k in range(m.K)]
        amap, offset = {}, 0
        for k in range(m.K):
            if not live[k]:
                continue
            amap[m.cbNames[k].encode()] = offset
            sz = 2 * m.refN[k] * 4 + (0 if countsOnly else 2 * m.refN[k] * 4 * m.D)
            offset += sz + 2 + len(m.cbNames[k].encode()) + 1 + 5 * 4 + 4       # cT:542-563
        out = [struct.pack(">fi", float(f32(totalPr)), int(totalT)), _write_map(amap)]
        for k in range(m.K):
            if not live[k]:
                continue
            out.append(_wstr(m.cbNames[k].encode()) + struct.pack(">5i", m.refN[k], m.D, 1, 2, 1 if countsOnly else 0))
            for g in range(m.off[k], m.off[k + 1]):
                out.append(struct.pack(">2f", float(f32(self.count[g])), float(f32(self.den[g]))))
                if not countsOnly:
                    out.append(self.sumO[g].astype(">f4").tobytes() + self.sumOsq[g].astype(">f4").tobytes())
            out.append(struct.pack(">i", CB_MARKER))
        return b"".join(out)

    def load_codebook_accus(self, data, factor=1.0, nParts=1, part=1):
        """cT:649-678, 369-433 -> (totalPr, totalT); adds factor x the stored floats"""
        m = self.m; k0, k1 = self._range(nParts, part); factor = f32(factor)
        totalPr, totalT = struct.unpack_from(">fi", data, 0)
        amap, p0 = _read_map(data, 8)
        new = [a.copy() for a in (self.count, self.den, self.sumO, self.sumOsq)]
        for k in range(k0, k1):
            name = m.cbNames[k].encode()
            if name not in amap:
                continue
            p = p0 + amap[name]
            _, p = _rstr(data, p)
            refN, dimN, subN, typ, co = struct.unpack_from(">5i", data, p); p += 20
            if refN != m.refN[k] or dimN != m.D or subN != 1 or typ != 2:
                raise DimensionError("accumulator of another shape")
            for g in range(m.off[k], m.off[k + 1]):
                c, d = np.frombuffer(data, ">f4", 2, p).astype(f32); p += 8
                new[0][g] += float(factor * c); new[1][g] += float(factor * d)
                if co:
                    continue
                new[2][g] += (factor * np.frombuffer(data, ">f4", m.D, p).astype(f32)).astype(np.float64); p += 4 * m.D
                new[3][g] += (factor * np.frombuffer(data, ">f4", m.D, p).astype(f32)).astype(np.float64); p += 4 * m.D
            if struct.unpack_from(">i", data, p)[0] != CB_MARKER:
                raise IOError("marker expected")
        self.count, self.den, self.sumO, self.sumOsq = new
        return totalPr, totalT

    def save_distrib_accus(self):
        """dT:439-461, 239-252, AccMap dT:375-393 -> bytes"""
        m = self.m
        live = [bool(np.any(self.dcount[m.off[k]:m.off[k + 1]] > 0.0) or np.any(self.dden[m.off[k]:m.off[k + 1]] > 0.0)) for k in range(m.K)]
        amap, offset = {}, 0
        for k in range(m.K):
            if live[k]:
                amap[m.dsNames[k].encode()] = offset; offset += 2 * m.refN[k] * 4 + 3 * 4
        out = [_write_map(amap)]
        for k in range(m.K):
            if not live[k]:
                continue
            out.append(struct.pack(">2i", m.refN[k], 1))
            for g in range(m.off[k], m.off[k + 1]):
                out.append(struct.pack(">2f", float(f32(self.dcount[g])), float(f32(self.dden[g]))))
            out.append(struct.pack(">i", DS_MARKER))
        return b"".join(out)

    def load_distrib_accus(self, data, factor=1.0, nParts=1, part=1):
        m = self.m; k0, k1 = self._range(nParts, part); factor = f32(factor)
        amap, p0 = _read_map(data, 0)
        new = [self.dcount.copy(), self.dden.copy()]
        for k in range(k0, k1):
            name = m.dsNames[k].encode()
            if name not in amap:
                continue
            p = p0 + amap[name]
            valN, subN = struct.unpack_from(">2i", data, p); p += 8
            if valN != m.refN[k] or subN != 1:
                raise DimensionError("Number of values do not match")
            for g in range(m.off[k], m.off[k + 1]):
                c, d = np.frombuffer(data, ">f4", 2, p).astype(f32); p += 8
                new[0][g] += float(factor * c); new[1][g] += float(factor * d)
            if struct.unpack_from(">i", data, p)[0] != DS_MARKER:
                raise IOError("marker expected")
        self.dcount, self.dden = new


def _wstr(b):
    return struct.pack(">h", len(b)) + b + b"\0"


def _rstr(data, p):
    n = struct.unpack_from(">h", data, p)[0]
    return bytes(data[p + 2:p + 2 + n]), p + 2 + n + 1


def _write_map(amap):
    return b"".join(_wstr(k) + struct.pack(">i", amap[k]) for k in sorted(amap)) + _wstr(END_OF_ACCS.encode())


def _read_map(data, p):
    amap = {}
    while True:
        name, p = _rstr(data, p)
        if name == END_OF_ACCS.encode():
            return amap, p
        if name in amap:
            raise KeyError(name)
        amap[name] = struct.unpack_from(">i", data, p)[0]; p += 4


# ---- test models ----------------------------------------------------------------------------------------------------------------------
def random_model(refN, D, seed, scale=None, spread=1.0):
    """a well-conditioned random model: means N(0, spread), variances in [0.5, 2], weights from a Dirichlet draw; consistent det"""
    rng = np.random.default_rng(seed); G = int(sum(refN))
    mean = (spread * rng.standard_normal((G, D))).astype(f32)
    var = rng.uniform(0.5, 2.0, (G, D)).astype(f32)
    val = np.concatenate([-np.log(rng.dirichlet(np.full(r, 4.0))) for r in refN]).astype(f32)
    m = Model(refN, mean, var, np.zeros(G, f32), val, scale)
    a = Accu(m); a.fix_gconsts(); a.invert_variances()
    return m


def sample(m, k, n, rng):
    """n frames drawn from distribution k of the model (cv holds inverse variances)"""
    a, b = m.off[k], m.off[k + 1]
    w = np.exp(-m.val[a:b].astype(np.float64)); w /= w.sum()
    comp = rng.choice(b - a, size=n, p=w)
    sd = 1.0 / np.sqrt(m.cv[a:b].astype(np.float64))
    return (m.mean[a:b][comp] + sd[comp] * rng.standard_normal((n, m.D))).astype(f32)
