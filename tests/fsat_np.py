"""numpy restatement of the fast form of asr/sat for diagonal 1:1 models: GaussDensity::normFastAccu (asr/sat/codebookFastSAT.cc:346-418,
"cfs"), the fast-accumulator file (cfs:175-253, 544-566, 597-644 over codebookTrain.cc:299-420), descLength (cfs:523-539, 654-673),
FastSAT::accumulate / addFastAcc / update / _updateVariance (asr/sat/sat.cc:501-587, "sat"), MDLSATMean::update / _solve (sat:395-493) with
numpy.linalg.eigh, SATBase::FastAcc::update (sat:1079-1099) and the return value of SATFast::estimate (sat.h:825-831, sat:1802-1839).

normFastAccu is written in the reference's operation order in fp64, so the device is compared bit for bit; FastSAT::accumulate is the mat part
of tests.sat_np.MeanAccus (sat:518-524 are sat:192-198), which also forms it in np.longdouble."""
import struct

import numpy as np

from tests import sat_np as N

f32, f64, LD = np.float32, np.float64, np.longdouble
SMALL_CK = 1.0e-06                                             # GaussDensity::Small_ck, cfs:344
MAX_RATIO = 1.0e-07                                            # SATMean::MaxSingularValueRatio, sat:255
LEFT, UPDATED, KEPT_OLD, ZEROED, FLAGGED = 0, 1, 2, 3, 4
END_OF_ACCS = "EndOfAccumulators"                              # distribTrain.h:230-233
MARKER = 123456789                                             # codebookTrain.cc:309
COV_DIAGONAL = 2


class DimensionError(Exception):
    """jdimension_error"""


class ConsistencyError(Exception):
    """jconsistency_error"""


class IOError_(Exception):
    """jio_error"""


class FastAccus(object):
    """CodebookFastSAT::FastAccu of every Gaussian, subN == 1: count, den [G], fastMean, fastVar [G][D], scalar [G][nB]"""

    def __init__(self, G, D, nB):
        self.G, self.D, self.nB, self.bl = G, D, nB, D // nB
        self.count, self.den = np.zeros(G), np.zeros(G)
        self.fastMean, self.fastVar, self.scalar = np.zeros((G, D)), np.zeros((G, D)), np.zeros((G, nB))

    def copy(self):
        o = FastAccus(self.G, self.D, self.nB)
        for k in ("count", "den", "fastMean", "fastVar", "scalar"):
            setattr(o, k, getattr(self, k).copy())
        return o

    def norm(self, classes, mean, iv, num, den, sumO, sumOsq, xf):
        """normFastAccu of one speaker for every Gaussian (cfs:346-418): num, den [G] = numProb, denProb; xf {class: Xform}"""
        classes = np.asarray(classes); num, den = np.asarray(num, f64), np.asarray(den, f64); bl = self.bl
        xs = {int(rc): N.transformer(xf, int(rc)) for rc in sorted(set(classes.tolist()))}
        for x in xs.values():
            if x.nB != self.nB:
                raise DimensionError("'nblks' does not match (%d vs. %d)" % (x.nB, self.nB))
        seen = ~((num == 0.0) & (den == 0.0))                                                    # cfs:348
        self.count[seen] = self.count[seen] + num[seen]; self.den[seen] = self.den[seen] + den[seen]    # cfs:365-366
        ck_all = num - den                                                                       # double postProb()
        live = seen & ~(np.abs(ck_all) < SMALL_CK)                                               # cfs:368
        for rc, x in xs.items():
            sel = np.nonzero(live & (classes == rc))[0]
            if not len(sel):
                continue
            ck = ck_all[sel]; trn = N.transform_mean(x, np.asarray(mean, f32)[sel]).astype(f64)   # cfs:374-377
            for nb in range(self.nB):
                sl = slice(nb * bl, (nb + 1) * bl); ivb = np.asarray(iv, f32)[sel, sl].astype(f64)
                T = x.A[nb][None, :, :] * ivb[:, :, None]                                        # cfs:383-388: temp1[m][n] = A[m][n] inv[m]
                so = np.asarray(sumO, f64)[sel, sl]; v = so - ck[:, None] * x.b[sl][None, :]      # cfs:391-393
                y = np.zeros((len(sel), bl))                                                     # dgemv(CblasTrans), beta = 0: row by row, a zero skipped
                for m in range(bl):
                    y = np.where(v[:, m, None] != 0.0, y + v[:, m, None] * T[:, m, :], y)
                self.fastMean[sel, sl] = self.fastMean[sel, sl] + y                              # cfs:397-399
                for m in range(bl):                                                              # cfs:402-405
                    self.scalar[sel, nb] = self.scalar[sel, nb] + ivb[:, m] * v[:, m] * v[:, m] / ck
                t = trn[:, sl]; sqr = t * t                                                      # cfs:410-414
                self.fastVar[sel, sl] = self.fastVar[sel, sl] + np.asarray(sumOsq, f64)[sel, sl] - 2.0 * t * so + ck[:, None] * sqr


# ---- the file ------------------------------------------------------------------------------------------------------------------------------------
def _wstr(s):
    b = s.encode(); return struct.pack(">H", len(b)) + b + b"\0"                                 # write_string: a short length, the bytes, a NUL


def _rstr(data, pos):
    if pos + 2 > len(data):
        raise IOError_("premature end of file")
    n = struct.unpack_from(">h", data, pos)[0]
    if n < 0 or pos + 2 + n + 1 > len(data):
        raise IOError_("premature end of file")
    return data[pos + 2:pos + 2 + n].decode(), pos + 2 + n + 1


def record_size(name, refN, D, nB):
    """FastAccu::size (cfs:241-254) over Accu::_size with rv of orgDimN (codebookTrain.cc:542-563)"""
    return 2 * refN * 4 + 2 * refN * 4 * D + 2 + len(name) + 1 + 5 * 4 + 4 + 2 * 4 + refN * nB * 4


def save_fast(acc, refN, names):
    """saveFastAccus (cfs:597-617) -> the bytes of the file; the codebooks are `refN` Gaussians each, in model order"""
    off = np.concatenate([[0], np.cumsum(refN)]).astype(int); D, nB = acc.D, acc.nB
    live = [bool(((acc.count[off[k]:off[k + 1]] != 0.0) | (acc.den[off[k]:off[k + 1]] != 0.0)).any()) for k in range(len(refN))]
    amap, pos = {}, 0
    for k in range(len(refN)):
        if live[k]:
            amap[names[k]] = pos; pos += record_size(names[k], refN[k], D, nB)
    out = b"".join(_wstr(n) + struct.pack(">i", amap[n]) for n in sorted(amap)) + _wstr(END_OF_ACCS)   # AccMap::write: std::map order
    for k in range(len(refN)):
        if not live[k]:
            continue
        out += _wstr(names[k]) + struct.pack(">7i", refN[k], D, 1, COV_DIAGONAL, 0, D, nB)
        for g in range(off[k], off[k + 1]):
            out += struct.pack(">2f", f32(acc.count[g]), f32(acc.den[g]))
            out += acc.fastMean[g].astype(">f4").tobytes() + acc.fastVar[g].astype(">f4").tobytes()
        out += acc.scalar[off[k]:off[k + 1]].astype(">f4").tobytes()
        out += struct.pack(">i", MARKER)
    return out


def load_fast(data, acc, refN, names, D, ks=None):
    """loadFastAccus (cfs:619-644): ADDS the file to acc (None: accumulators of the file's nblks) for the codebooks ks -> acc"""
    off = np.concatenate([[0], np.cumsum(refN)]).astype(int); G = int(off[-1]); amap, pos = {}, 0
    while True:
        name, pos = _rstr(data, pos)
        if name == END_OF_ACCS:
            break
        if pos + 4 > len(data):
            raise IOError_("premature end of file")
        amap[name] = struct.unpack_from(">i", data, pos)[0]; pos += 4
    start = pos; new = None if acc is None else acc.copy()

    def take(fmt, p):
        n = struct.calcsize(fmt)
        if p + n > len(data):
            raise IOError_("premature end of file")
        return struct.unpack_from(fmt, data, p), p + n
    for k in (range(len(refN)) if ks is None else ks):
        if names[k] not in amap:
            continue
        _, p = _rstr(data, start + amap[names[k]])
        (r, d, subN, typ, countsOnly), p = take(">5i", p)
        if r != refN[k] or d != D or subN != 1 or typ != COV_DIAGONAL:
            raise DimensionError("the record of %s does not match" % names[k])
        if countsOnly:
            raise ConsistencyError("Mean and variance statistics must be included in fast accumulators.")
        (orgDimN, nblks), p = take(">2i", p)
        if orgDimN != D:
            raise DimensionError("'orgDimN' does not match (%d vs. %d)" % (orgDimN, D))
        if new is None:
            if nblks < 1 or D % nblks:
                raise DimensionError("'nblks' = %d" % nblks)
            new = FastAccus(G, D, nblks)
        if nblks != new.nB:
            raise DimensionError("'nblks' does not match (%d vs. %d)" % (nblks, new.nB))
        for g in range(off[k], off[k + 1]):                    # float factor (1) x float value, added in double
            v, p = take(">%df" % (2 + 2 * D), p); v = np.asarray(v, f32).astype(f64)
            new.count[g] += v[0]; new.den[g] += v[1]; new.fastMean[g] += v[2:2 + D]; new.fastVar[g] += v[2 + D:]
        v, p = take(">%df" % (refN[k] * nblks), p)
        new.scalar[off[k]:off[k + 1]] += np.asarray(v, f32).astype(f64).reshape(refN[k], nblks)
        (marker,), p = take(">i", p)
        if marker != MARKER:
            raise IOError_("CheckMarker: Marker expected in accu file (%d vs. %d)." % (marker, MARKER))
    return new


# ---- the SAT sums ----------------------------------------------------------------------------------------------------------------------------------
class SatSums(object):
    """FastSAT of every Gaussian: mat, vec, scalar, occ (sat_np.MeanAccus) and varVec [G][D]"""

    def __init__(self, G, D, dtype=f64):
        self.a = N.MeanAccus(G, D, dtype); self.G, self.D = G, D; self.varVec = np.zeros((G, D))

    def accumulate(self, classes, iv, c, xf, gs=None):
        """FastAcc::accumulate (sat:1067-1077, 501-528): float c = float(count - denCount); mat and occ only"""
        a = self.a; keep = None if not a.nB else (a.vec.copy(), a.scalar.copy())
        a.accumulate(classes, iv, c, np.zeros((self.G, self.D)), xf, gs)
        a.vec[:] = 0 if keep is None else keep[0]; a.scalar[:] = 0 if keep is None else keep[1]     # vec and scalar come from add_fast alone

    def add_fast(self, fast, gs=None):
        """FastSAT::addFastAcc (sat:530-550): every block is allocated afterwards"""
        a = self.a; a._check_blocks(fast.nB); gs = np.arange(self.G) if gs is None else np.asarray(gs); t = a.dtype
        keep = (a.vec.copy(), a.scalar.copy())
        a.vec[gs] = keep[0][gs] + fast.fastMean.reshape(self.G, fast.nB, fast.bl)[gs].astype(t)
        a.scalar[gs] = keep[1][gs] + fast.scalar[gs].astype(t)
        self.varVec[gs] = self.varVec[gs] + fast.fastVar[gs]
        a.has[gs] = True


def mdl_solve(mat, vec, thr):
    """MDLSATMean::_solve (sat:469-493) with numpy.linalg.eigh -> dict(x, kept, keep [bl], lam, t, contrib, ratio)"""
    lam, U = np.linalg.eigh(mat)
    t = U.T @ vec
    largest = max(0.0, float(lam.max()))                                                        # from 0.0, sat:474-477
    with np.errstate(divide="ignore", invalid="ignore"):
        contrib = 0.5 * (t * t / lam); ratio = lam / largest
        keep = (contrib > thr) & (ratio >= MAX_RATIO)
        tt = np.where(keep, t / np.where(keep, lam, 1.0), 0.0)
    return dict(x=U @ tt, kept=int(keep.sum()), keep=keep, lam=lam, t=t, contrib=contrib, ratio=ratio)


def update_variance(varVec, occ, cv, meanOnly):
    """FastSAT::update's variance half (sat:555-560, 570-587) of one Gaussian: cv float32 [D] holds inverse variances -> float32"""
    inv = (1.0 / cv.astype(f64)).astype(f32)
    if meanOnly:
        return inv
    with np.errstate(divide="ignore", invalid="ignore"):
        var = np.asarray(varVec, f64) / occ
    return np.where(np.isnan(var), inv, var.astype(f32)).astype(f32)


def update(mat, vec, scalar, occ, has, varVec, mean, cv, descLen, lhoodThreshold, massThreshold, meanOnly=False, gs=None, skip=()):
    """FastAcc::update over the Gaussians gs in model order (sat:1079-1099, 552-587, 395-462) on given sums.  skip: Gaussians the library flags
    (their mean and description lengths stay, their covariance slot becomes 1 / var, they count in the totals only).
    -> dict(mean, cv float32, descLen, info [4], totals [2], aux, decision, kept, auxOld, auxNew [G][nB], solves {(g, nb): mdl_solve})"""
    mean = np.array(mean, f32); cv0 = np.array(cv, f32); cv = cv0.copy(); descLen = np.array(descLen, np.int64)
    G, nB, bl = mat.shape[0], mat.shape[1], mat.shape[2]; thr = N.threshold_of(massThreshold)
    info = [0, 0, 0, 0]; totals = [0, 0]; aux = 0.0; solves = {}
    dec = np.zeros((G, nB), np.int32); kept = np.zeros((G, nB), np.int32); aO = np.zeros((G, nB)); aN = np.zeros((G, nB))
    for g in (range(G) if gs is None else gs):
        totals[0] += 1
        if occ[g] < thr:
            cv[g] = (1.0 / cv0[g].astype(f64)).astype(f32)                                      # sat:1088-1093
            continue
        totals[1] += 1
        if not has[g]:
            continue
        if g in skip:
            cv[g] = (1.0 / cv0[g].astype(f64)).astype(f32); dec[g] = FLAGGED
            continue
        cv[g] = update_variance(varVec[g], occ[g], cv0[g], meanOnly)
        if occ[g] == 0.0:
            mean[g] = 0.0; dec[g] = ZEROED                                                      # sat:399-407
            continue
        for nb in range(nB):
            sl = slice(nb * bl, (nb + 1) * bl); M, v, sc = np.asarray(mat[g, nb], f64), np.asarray(vec[g, nb], f64), float(scalar[g, nb])
            old = N.aux_func(M, v, sc, mean[g, sl].astype(f64)) + lhoodThreshold * int(descLen[g, nb])      # sat:424-426
            s = mdl_solve(M, v, lhoodThreshold); solves[(g, nb)] = s
            new = N.aux_func(M, v, sc, s["x"]) + lhoodThreshold * s["kept"]                     # sat:430-432
            aO[g, nb], aN[g, nb], kept[g, nb] = old, new, s["kept"]
            if old < new:                                                                       # sat:439-443
                aux += old; info[0] += 1; dec[g, nb] = KEPT_OLD
                continue
            descLen[g, nb] = s["kept"]; mean[g, sl] = s["x"].astype(f32); aux += new; dec[g, nb] = UPDATED
            info[0] += 1; info[1] += 1; info[2] += bl; info[3] += s["kept"]
    return dict(mean=mean, cv=cv, descLen=descLen, info=info, totals=totals, aux=aux, decision=dec, kept=kept, auxOld=aO, auxNew=aN, solves=solves)


def conditions(res, lhoodThreshold):
    """how far the inputs of an update are from every tie the device may resolve the other way -> dict of the smallest margins:
    contrib: min |0.5 t^2 / l - thr| / max(thr, 0.5 t^2 / |l|) over components whose ratio test passes (those it fails are dropped either way);
    ratio: min over components of max(ratio / 1e-7, 1e-7 / ratio) for ratio > 0 (a non-positive ratio is dropped however it is rounded);
    gap: min relative distance of a kept eigenvalue to a dropped one (then V t' is unique);  aux: min |auxOld - auxNew| / max(|auxOld|, |auxNew|)"""
    out = dict(contrib=np.inf, ratio=np.inf, gap=np.inf, aux=np.inf)
    for (g, nb), s in res["solves"].items():
        lam, c, r, keep = s["lam"], s["contrib"], s["ratio"], s["keep"]
        for k in range(len(lam)):
            if r[k] >= MAX_RATIO and np.isfinite(c[k]):
                out["contrib"] = min(out["contrib"], abs(c[k] - lhoodThreshold) / max(lhoodThreshold, abs(c[k])) if max(lhoodThreshold, abs(c[k])) > 0 else np.inf)
            if r[k] > 0:
                out["ratio"] = min(out["ratio"], max(r[k] / MAX_RATIO, MAX_RATIO / r[k]))
        for a in lam[keep]:
            for b in lam[~keep]:
                out["gap"] = min(out["gap"], abs(a - b) / max(abs(a), abs(b)))
        o, n = res["auxOld"][g, nb], res["auxNew"][g, nb]
        out["aux"] = min(out["aux"], abs(o - n) / max(abs(o), abs(n)) if max(abs(o), abs(n)) > 0 else np.inf)
    return out


def desc_length(descLen):
    """CodebookSetFastSAT::descLength (cfs:654-673)"""
    return int(np.asarray(descLen, np.int64).sum())


def estimate_return(lhoodThreshold, descLength, totalPr, totalT):
    """sat:1805-1806, 1825-1826, 1838: LogLhoodThreshhold descLength() + the LogDouble(float)s, in double, over an int sum"""
    pr = lhoodThreshold * descLength
    for p in np.asarray(totalPr, f32):
        pr += float(p)
    return pr / int(np.sum(np.asarray(totalT, np.int64)))
