"""numpy restatement of the ML slice of asr/sat/sat.cc ("sat") for diagonal 1:1 models: SATMean (sat:54-342), SATVariance (sat:686-760),
SATBase::MeanAcc / VarianceAcc (sat:999-1025, 1194-1246), SATBase::estimate's file names and return value (sat:1802-1839, 1890),
TransformerTree::transformer (asr/adapt/transform.cc:2165-2173, "tr") and SpeakerList (tr:1989-1998).

The accumulators are formed in the reference's order (speaker by speaker, block by block) in fp64, and a second time in np.longdouble
(dtype=LD) as the near-exact sums the device is bounded against; `bounds` are the sums of the terms' magnitudes those bounds scale."""
import numpy as np

from tests import adapt_np as A

f32, f64, LD = np.float32, np.float64, np.longdouble
HAVE_LD = np.finfo(LD).nmant >= 63                           # the tests that need the near-exact sums skip otherwise


def require_ld():
    """the near-exact sums need eleven bits more than a double: asserted wherever they are formed"""
    assert np.finfo(LD).nmant >= 63, "np.longdouble holds %d mantissa bits here" % np.finfo(LD).nmant
MLLR, APT = 1, 2
MAX_SV_RATIO = 1.0e-07                                       # SATMean::MaxSingularValueRatio, sat:255
LEFT, UPDATED, KEPT_OLD, ZEROED, FLAGGED = 0, 1, 2, 3, 4


class NumericError(Exception):
    """jnumeric_error"""


class DimensionError(Exception):
    """jdimension_error"""


class ParseError(Exception):
    """the library's answer to a line SpeakerList cannot hold"""


class Xform(object):
    """TransformMatrix of one (speaker, class): A [nBlocks][bl][bl], b [D] (the block offsets), the first bSize of which the transform adds"""

    def __init__(self, kind, A_, b=None):
        A_ = np.asarray(A_, f64); self.kind = kind; self.A = A_[None] if A_.ndim == 2 else A_
        self.nB, self.bl = self.A.shape[0], self.A.shape[1]; D = self.nB * self.bl
        self.bSize = 0 if b is None else len(b); self.b = np.zeros(D); self.b[:self.bSize] = np.asarray(b if b is not None else [], f64)


def mllr_xforms(tree):
    """the transformers of an adapt_np.ParamTree (tr:1746-1768): one block, the bias as the offset"""
    return {rc: Xform(MLLR, np.asarray(p.matrix, f64).reshape(p.size, p.size), p.bias) for rc, p in tree.map.items()}


def apt_xform(matrix, nSub, bias=()):
    """tr:1339-1363: nSub blocks holding the same matrix, the float bias as the offsets of the blocks it covers"""
    return Xform(APT, np.stack([matrix] * nSub), np.asarray(bias, f32).astype(f64) if len(bias) else None)


def transformer(xf, rc):
    """TransformerTree::transformer (tr:2165-2173): the exact node, which must be a leaf (tr:2082-2100)"""
    if rc == 0:
        raise A.IndexError_("Regression class index must be >= 1")
    if rc not in xf:
        raise A.KeyError_("Could not find node %d." % rc)
    if any(k != rc and A.is_ancestor(rc, k) for k in xf):
        raise A.ConsistencyError("Node for regression class %d is not a leaf" % rc)
    return xf[rc]


def transform_mean(x, mu):
    """transformer.transform(origMean) in the reference's types, rows [N][D] -> float32.  MLLR (tr:1777-1784): float comp = offset;
    comp += A[m][n] * from[n], rounded to float after every term.  APT (tr:1300-1336): the double sum stored to float, then the float bias"""
    mu = np.asarray(mu, f32); N = mu.shape[0]; out = np.empty_like(mu)
    for nb in range(x.nB):
        sl = slice(nb * x.bl, (nb + 1) * x.bl); m = mu[:, sl].astype(f64)
        if x.kind == MLLR:
            comp = np.broadcast_to(np.where(np.arange(sl.start, sl.stop) < x.bSize, x.b[sl], 0.0).astype(f32), (N, x.bl)).copy()
            for j in range(x.bl):
                comp = (comp.astype(f64) + x.A[nb][None, :, j] * m[:, j, None]).astype(f32)
        else:
            acc = np.zeros((N, x.bl))
            for j in range(x.bl):
                acc = acc + x.A[nb][None, :, j] * m[:, j, None]
            comp = acc.astype(f32)
            k = np.arange(sl.start, sl.stop) < x.bSize
            comp[:, k] = comp[:, k] + x.b[sl][k].astype(f32)[None, :]
        out[:, sl] = comp
    return out


def post_prob(c):
    """float c_k = postProb() (codebookTrain.h:142-144, sat:1003) of c = count - denCount"""
    return np.asarray(c, f64).astype(f32)


class MeanAccus(object):
    """SATMean of every Gaussian; dtype LD gives the near-exact sums.  occ is always the sequential double sum (sat:217, 1007)"""

    def __init__(self, G, D, dtype=f64):
        if dtype is LD:
            require_ld()
        self.G, self.D, self.dtype, self.nB = G, D, dtype, 0
        self.occ = np.zeros(G); self.has = np.zeros(G, bool); self.n = 0

    def _check_blocks(self, nB):                                   # sat:54-81, one count for the handle
        if self.nB:
            if nB != self.nB:
                raise DimensionError("Block sizes (%d vs %d) are not equivalent." % (nB, self.nB))
            return
        if self.D % nB:
            raise DimensionError("Transformed feature length %d is not compatible with %d blocks." % (self.D, nB))
        self.nB, self.bl = nB, self.D // nB; G, bl, t = self.G, self.D // nB, self.dtype
        self.mat, self.vec, self.scalar = np.zeros((G, nB, bl, bl), t), np.zeros((G, nB, bl), t), np.zeros((G, nB), t)
        self.bmat, self.bvec, self.bscalar = np.zeros((G, nB, bl, bl)), np.zeros((G, nB, bl)), np.zeros((G, nB))

    def accumulate(self, classes, iv, c, sumO, xf, gs=None):
        """one speaker (sat:999-1008, 171-218): c [G] = count - denCount, sumO [G][D], xf {class: Xform}; gs: the Gaussians of the part"""
        t = self.dtype; classes = np.asarray(classes); gs = np.arange(self.G) if gs is None else np.asarray(gs)
        xs = {int(rc): transformer(xf, int(rc)) for rc in sorted(set(classes[gs].tolist()))}
        self._check_blocks(next(iter(xs.values())).nB)
        for x in xs.values():
            self._check_blocks(x.nB)
        cf = post_prob(c); live = np.zeros(self.G, bool); live[gs] = True; live &= (cf != 0)
        bl = self.bl
        for rc, x in xs.items():
            sel = np.nonzero(live & (classes == rc))[0]
            if not len(sel):
                continue
            ck = cf[sel].astype(t)
            for nb in range(self.nB):
                sl = slice(nb * bl, (nb + 1) * bl); Ab = x.A[nb].astype(t); ivb = np.asarray(iv, f32)[sel, sl].astype(t)
                T = Ab[None, :, :] * ivb[:, :, None]                                             # sat:192-197
                self.mat[sel, nb] += ck[:, None, None] * np.einsum("gmp,mq->gpq", T, Ab)         # sat:198
                v1 = np.asarray(sumO, f64)[sel, sl].astype(t) - ck[:, None] * x.b[sl].astype(t)[None, :]      # sat:204-206
                self.vec[sel, nb] += np.einsum("gmp,gm->gp", T, v1)                              # sat:207
                for m in range(bl):                                                              # sat:210-213
                    self.scalar[sel, nb] += ivb[:, m] * v1[:, m] * v1[:, m] / ck
                aT = np.abs(T.astype(f64)); aA = np.abs(x.A[nb]); ac = np.abs(ck.astype(f64))
                mag = np.abs(np.asarray(sumO, f64)[sel, sl]) + ac[:, None] * np.abs(x.b[sl])[None, :]
                self.bmat[sel, nb] += ac[:, None, None] * np.einsum("gmp,mq->gpq", aT, aA)
                self.bvec[sel, nb] += np.einsum("gmp,gm->gp", aT, mag)
                self.bscalar[sel, nb] += (ivb.astype(f64) * mag * mag / ac[:, None]).sum(1)
        self.occ[live] = self.occ[live] + cf[live].astype(f64)
        self.has |= live
        self.n += 1


class VarAccus(object):
    """SATVariance of every Gaussian (sat:704-729): the reference's expression, evaluated left to right in double"""

    def __init__(self, G, D):
        self.G, self.D = G, D; self.vec = np.zeros((G, D)); self.occ = np.zeros(G); self.bound = np.zeros((G, D)); self.model = np.zeros((G, D)); self.n = 0

    def accumulate(self, classes, mean, c, sumO, sumOsq, xf, gs=None, exact=None):
        """-> the transformed means float32 [G][D] (zero where the count is zero).  exact [G][D] (or None): the speaker's true means, for
        `model`, the sum of c (trn - exact)^2 that the float transform leaves in the variance"""
        classes = np.asarray(classes); gs = np.arange(self.G) if gs is None else np.asarray(gs)
        xs = {int(rc): transformer(xf, int(rc)) for rc in sorted(set(classes[gs].tolist()))}
        cf = post_prob(c); live = np.zeros(self.G, bool); live[gs] = True; live &= (cf != 0)
        out = np.zeros((self.G, self.D), f32)
        for rc, x in xs.items():
            sel = np.nonzero(live & (classes == rc))[0]
            if not len(sel):
                continue
            trn32 = transform_mean(x, np.asarray(mean, f32)[sel]); out[sel] = trn32
            trn = trn32.astype(f64); sqr = trn * trn; ck = cf[sel].astype(f64)[:, None]
            so, sq = np.asarray(sumO, f64)[sel], np.asarray(sumOsq, f64)[sel]
            self.vec[sel] = self.vec[sel] + sq - 2.0 * trn * so + ck * sqr                        # sat:723-724
            self.bound[sel] += np.abs(sq) + 2.0 * np.abs(trn * so) + np.abs(ck) * sqr
            if exact is not None:
                self.model[sel] += ck * (trn - np.asarray(exact, f64)[sel]) ** 2
        self.occ[live] = self.occ[live] + cf[live].astype(f64)
        self.n += 1
        return out


def aux_func(mat, vec, scalar, mean):
    """SATMean::_auxFunc (sat:276-286)"""
    return 0.5 * (float(mean @ (mat @ mean)) + scalar) - float(mean @ vec)


def solve(mat, vec):
    """SATMean::_solve (sat:257-274) -> (new mean, kept components, singular values)"""
    U, s, Vt = np.linalg.svd(mat)
    t = U.T @ vec
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = (s / s[0]) >= MAX_SV_RATIO
    t = np.where(keep, t / np.where(keep, s, 1.0), 0.0)
    return Vt.T @ t, int(keep.sum()), s


def threshold_of(massThreshold):
    return 10.0 if massThreshold == 0.0 else massThreshold       # sat:1768


def update_means(mat, vec, scalar, occ, has, mean, massThreshold, gs=None):
    """MeanAcc::update over the Gaussians gs in model order (sat:1010-1023, 288-342) on given accumulators
    -> dict(mean float32, info [4], totals [2], aux, decision [G][nB], kept [G][nB], auxOld, auxNew [G][nB])"""
    mean = np.array(mean, f32); G, nB, bl = mat.shape[0], mat.shape[1], mat.shape[2]; thr = threshold_of(massThreshold)
    gs = range(G) if gs is None else gs
    info = [0, 0, 0, 0]; totals = [0, 0]; aux = 0.0
    dec = np.zeros((G, nB), np.int32); kept = np.zeros((G, nB), np.int32); aO = np.zeros((G, nB)); aN = np.zeros((G, nB))
    for g in gs:
        totals[0] += 1
        if occ[g] < thr:
            continue
        totals[1] += 1
        if not has[g]:
            continue
        if occ[g] == 0.0:
            mean[g] = 0.0; dec[g] = ZEROED
            continue
        for nb in range(nB):
            sl = slice(nb * bl, (nb + 1) * bl); M, v, sc = np.asarray(mat[g, nb], f64), np.asarray(vec[g, nb], f64), float(scalar[g, nb])
            old = aux_func(M, v, sc, mean[g, sl].astype(f64))
            q, k, _ = solve(M, v)
            new = aux_func(M, v, sc, q)
            aO[g, nb], aN[g, nb], kept[g, nb] = old, new, k
            if old < new:                                                                       # sat:322-326
                aux += old; info[0] += 1; dec[g, nb] = KEPT_OLD
                continue
            if np.isnan(q).any():
                raise NumericError("Degenerate value in mean component")
            mean[g, sl] = q.astype(f32); aux += new; dec[g, nb] = UPDATED
            info[0] += 1; info[1] += 1; info[2] += bl; info[3] += k                             # uinfo(1, 1); ttlDimensions is set, then added
    return dict(mean=mean, info=info, totals=totals, aux=aux, decision=dec, kept=kept, auxOld=aO, auxNew=aN)


def update_variances(vec, occ, cv, massThreshold, gs=None):
    """VarianceAcc::update (sat:1233-1244, 731-756) -> (the covariance slot float32, holding VARIANCES where updated, totals [2])"""
    cv = np.array(cv, f32); thr = threshold_of(massThreshold); totals = [0, 0]
    for g in (range(len(occ)) if gs is None else gs):
        totals[0] += 1
        if occ[g] < thr:
            cv[g] = (1.0 / cv[g].astype(f64)).astype(f32)                                       # fixup
            continue
        totals[1] += 1
        if occ[g] == 0.0:
            cv[g] = 0.0
            continue
        with np.errstate(invalid="ignore", divide="ignore"):
            new = vec[g] / occ[g]
        if np.isnan(new).any():
            raise NumericError("updateSATVar: degenerate variance value")
        cv[g] = new.astype(f32)
    return cv, totals


def speaker_list(data):
    """SpeakerList (tr:1989-1998) over the bytes of the file: fgets into 128 bytes, strtok(buffer, "\\n")"""
    out, pos = [], 0
    while pos < len(data):
        end = data.find(b"\n", pos, pos + 127)
        chunk = data[pos:pos + 127] if end < 0 else data[pos:end + 1]
        pos += len(chunk)
        tok = chunk.rstrip(b"\n")                                # a chunk holds a newline only at its end
        if not tok:
            raise ParseError("empty line %d" % (len(out) + 1))   # strtok returns NULL there
        out.append(tok.decode())
    return out


def accu_file(meanVarsStats, spkr):
    return meanVarsStats + spkr + ".cbs.accu"                   # sat:1821


def param_file(spkrAdaptParms, spkr):
    return spkrAdaptParms + spkr                                # sat:1890: no separator


def estimate_return(totalPr, totalT):
    """sat:1825-1826, 1838: LogDouble(float) summed in double over an int sum"""
    return float(np.sum(np.asarray(totalPr, f32).astype(f64))) / int(np.sum(np.asarray(totalT, np.int64)))
