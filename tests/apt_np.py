"""numpy restatement of the one-parameter all-pass transforms of asr/adapt/transform.cc ("tr") and asr/train/estimateAdapt.cc ("eA"): the
yardstick of the APT tests.  Restated from the cited lines: LaurentSeries, CauchyProduct, multAdd, shift (tr:39-101), _calcMappedPoint and
_calcTransMatrix (tr:1199-1242), transform (tr:1295-1337), bilinear (tr:1404-1414), SLAPTTransformer::_calcSequence (tr:1640-1650, 1716-1741),
the parameter text format (tr:283-441, 490-501, 542-551), findAPT (tr:862-896), bracket / brentsMethod (eA:81-240), _calcBias / _calcMixLhood
(eA:1574-1620), both calcLogLhoods and estimates (eA:821-830, 1638-1690, 1851-1929), LeafIterator::estimate (eA:3105-3133).

Float / double placement is the reference's: np.float32 where it holds a float (the transformed mean, the bias and its denominator, c_k, the
inverse variances), fp64 elsewhere.  Sums over j (Cauchy products), m (transform) and k (_calcMixLhood) are sequential; only the output
index and the Gaussians of one step are vectorised.  Nothing here is taken from the reference's text."""
import math

import numpy as np

from tests.adapt_np import (ConsistencyError, IndexError_, KeyError_, ParameterError, TypeError_, is_ancestor, node_gaussians, tree_nodes)

f32, f64 = np.float32, np.float64
LEN = 150                            # DefaultSeriesLength (transform.h:83)
LAST = LEN - 1
COLUMNS = 50                         # SLAPTTransformer::NoColumns (tr:1638)
UNSPECIFIED, RAPT, SLAPT = 0, 1, 2   # AdaptationType + 1
NONE, CEPSTRA_ONLY, ALL_COMPONENTS = 0, 1, 2

# EstimatorBase (eA:81-91)
MAX_ITNS, TOLERANCE, CONST_GOLD, GOLD, GOLD_LIMIT, TINY, Z_EPSILON = 100, 1.0e-02, 0.3819660, 1.618034, 10.0, 1.0e-20, 1.0e-10
RHO_EPSILON, MAXIMUM_RHO = 1.0e-03, 0.90


class DimensionError(Exception):
    """jdimension_error"""


# ---- Laurent series: arrays of 2 LEN - 1 doubles, coefficient i at [i + LAST] -----------------------------------------------------------------
def series():
    return np.zeros(2 * LEN - 1)


def cauchy(s1, s2):
    """CauchyProduct (tr:85-101): out[i] = sum_j s1[j] s2[i - j] for j = max(-last, i - last) .. min(last, i + last), j ascending.  Walking j
    outside and updating every i whose range holds j adds each i's products in the same order.  A step whose s1[j] is zero adds +-0 to a
    sum that starts at +0 -- the same bits -- and is left out while s2 is finite (the SLAPT series has two non-zero coefficients)."""
    out = series(); finite = bool(np.isfinite(s2).all())
    for j in range(-LAST, LAST + 1):
        a = s1[j + LAST]
        if a == 0.0 and finite:
            continue
        lo, hi = max(-LAST, j - LAST), min(LAST, j + LAST)                   # the i with lower <= j <= upper
        out[lo + LAST:hi + LAST + 1] += a * s2[lo - j + LAST:hi - j + LAST + 1]
    return out


def bilinear(mu):
    """BLTTransformer::bilinear (tr:1404-1414)"""
    if abs(mu) >= 1.0:
        raise ParameterError("Mu value (%g) is not < 1.0" % mu)
    s = series(); s[LAST] = -mu; s[LAST + 1] = 1.0 - mu * mu
    for i in range(2, LEN):
        s[LAST + i] = mu * s[LAST + i - 1]
    return s


def e_coefficients():
    """tr:1640-1650"""
    e = np.ones(COLUMNS)
    for i in range(2, COLUMNS):
        e[i] = e[i - 1] / i
    return e


def slapt_sequence(params):
    """SLAPTTransformer::_calcSequence (tr:1716-1741)"""
    params = np.atleast_1d(np.asarray(params, f64)); e = e_coefficients()
    f0 = series(); f0[LAST] = 1.0
    f1 = series()
    for i in range(1, len(params) + 1):
        f1[LAST + i] = (math.pi / 2) * params[i - 1]; f1[LAST - i] = -(math.pi / 2) * params[i - 1]
    seq = series()
    seq += e[0] * f0                                                         # multAdd (tr:69-76)
    seq += e[1] * f1
    prev = f1
    for i in range(2, COLUMNS):
        prev = cauchy(f1, prev)
        seq += e[i] * prev
    seq[1:] = seq[:-1].copy()                                                # shift (tr:78-83): element -last stays as it was
    return seq


def calc_sequence(kind, params):
    return bilinear(float(np.atleast_1d(params)[0])) if kind == RAPT else slapt_sequence(params)


def mapped_point(z, seq):
    """_calcMappedPoint (tr:1199-1210)"""
    s = 0j; si = 0j; zi = 1.0 / z
    for i in range(LEN - 1, 0, -1):
        si = seq[LAST - i] + zi * si
        s = seq[LAST + i] + z * s
    return si * zi + s * z + seq[LAST]


def trans_matrix(seq, L):
    """_calcTransMatrix (tr:1212-1242) without an LDA matrix -> [L][L]"""
    A = np.zeros((L, L)); A[0, 0] = 1.0
    q = seq
    for m in range(1, L):
        if m >= 2:
            q = cauchy(seq, q)
        el = q[LAST:LAST + L] + q[LAST - np.arange(L)]
        el[0] /= 2.0
        A[:, m] = el
    return A


def matrix(kind, params, L):
    return trans_matrix(calc_sequence(kind, params), L)


def transform(A, mean, nSub, bias=None):
    """APTTransformerBase::transform (tr:1295-1337), normal case, for rows of means [N][nSub L]: a double sum for m ascending stored to
    float, then the float bias added to the first len(bias) components"""
    L = A.shape[0]; mean = np.asarray(mean, f32); N = mean.shape[0]; x = mean.reshape(N, nSub, L).astype(f64)
    acc = np.zeros((N, nSub, L))
    for m in range(L):
        acc = acc + A[None, None, :, m] * x[:, :, m, None]
    to = acc.astype(f32).reshape(N, nSub * L)
    if bias is not None and len(bias):
        to[:, :len(bias)] = to[:, :len(bias)] + np.asarray(bias, f32)[None, :]
    return to


# ---- the likelihood --------------------------------------------------------------------------------------------------------------------------
def bias_size(biasType, L, nSub):
    """eA:1553-1563"""
    return 0 if biasType == NONE else L if biasType == CEPSTRA_ONLY else L * nSub


class Stats(object):
    """what an estimator of one node reads: the Gaussians `gs` of the node in model order"""

    def __init__(self, mean, ivar, c, sumO, gs, L, nSub, biasType):
        gs = list(gs)
        self.mean = np.asarray(mean, f32)[gs]; self.iv = np.asarray(ivar, f32)[gs]; self.c = np.asarray(c, f64)[gs]
        self.sumO = np.asarray(sumO, f64)[gs]; self.L, self.nSub, self.bSize = L, nSub, bias_size(biasType, L, nSub)
        self.ck = self.c.astype(f32)                                         # float c_k = pdf.postProb()
        self.used = np.nonzero(self.ck != 0.0)[0]


def calc_bias(A, st, track=False):
    """_calcBias (eA:1574-1601): float accumulators, Gaussian after Gaussian"""
    b = st.bSize
    if b == 0:
        return (np.zeros(0, f32), None) if track else np.zeros(0, f32)
    T = transform(A, st.mean, st.nSub)
    bias = np.zeros(b, f32); den = np.zeros(b, f32); aN = np.zeros(b); aD = np.zeros(b)
    for j in st.used:
        ck = st.ck[j]; iv = st.iv[j, :b]
        prod = ck * T[j, :b]; assert prod.dtype == f32                       # c_k * _transFeat(n): a float product
        term = (st.sumO[j, :b] - prod.astype(f64)) * iv.astype(f64)
        bias = (bias.astype(f64) + term).astype(f32)
        dt = ck * iv; assert dt.dtype == f32
        den = den + dt
        aN += np.abs(term); aD += np.abs(dt.astype(f64))
    with np.errstate(divide="ignore", invalid="ignore"):
        out = bias / den
    assert out.dtype == f32
    if track:
        return out, dict(num=bias.astype(f64), den=den.astype(f64), absNum=aN, absDen=aD, n=len(st.used))
    return out


def mix_lhood(A, bias, st, track=False):
    """the sum of _calcMixLhood (eA:1603-1620) over the node's Gaussians and the counts -> (sum, nCounts)"""
    u = st.used; D = st.mean.shape[1]
    trn = transform(A, st.mean[u], st.nSub, bias).astype(f64)
    ck = st.ck[u].astype(f64); iv = st.iv[u].astype(f64); so = st.sumO[u]
    mix = np.zeros(len(u)); absT = np.zeros((len(u), D))
    for k in range(D):
        term = (so[:, k] - 0.5 * ck * trn[:, k]) * trn[:, k] * iv[:, k]
        mix = mix + term; absT[:, k] = np.abs(term)
    total = 0.0; nCounts = 0.0
    for j in range(len(u)):
        total += float(mix[j]); nCounts += float(ck[j])
    if track:
        return total, nCounts, dict(trn=trn, absT=absT, sens=(np.abs(so) + np.abs(ck[:, None] * trn)) * iv, ck=ck, iv=iv)
    return total, nCounts


def calc_log_lhood(kind, x, st, want_bias=False):
    """BLTEstimatorAdapt::calcLogLhood (eA:1638-1657) / SLAPTEstimatorAdapt::calcLogLhood (eA:2026-2045) with one parameter"""
    A = matrix(kind, [x], st.L)
    bias = calc_bias(A, st)
    total, n = mix_lhood(A, bias, st)
    with np.errstate(divide="ignore", invalid="ignore"):
        L = float(np.float64(total) / np.float64(n))
    return (L, bias) if want_bias else L


U32, U64 = 2.0 ** -24, 2.0 ** -53


def bias_bound(info, bias):
    """|bias_dev - bias_np| per component.  The device adds the numerator and the denominator of _calcBias in fp64 and rounds each to float
    once; the reference rounds each accumulator to float after every Gaussian (eA:1594: `_bias(n) +=`, eA:1595: `_denom(n) +=`): 2 float
    roundings a used Gaussian and component that the reordered sums skip.  Each is at most 2^-24 of the partial sum, itself at most the sum
    of the terms' magnitudes; the device's own rounding to float adds one more; the quotient is rounded once on either side."""
    n = info["n"]; b = np.abs(np.asarray(bias, f64))
    dnum = ((n + 1) * U32 + 2 * n * U64) * info["absNum"]; dden = ((n + 1) * U32 + 2 * n * U64) * info["absDen"]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (dnum + b * dden) / np.abs(info["den"]) + 2 * U32 * b


def lhood_bound(kind, x, st):
    """|L_dev - L_np| at one point, to first order in the roundings.  eA:1613-1616 holds no float rounding that the device skips (its sum
    is a double, and each Gaussian's value is computed as there), so without a bias only the order of the two fp64 sums over the n used
    Gaussians differs: 2 n 2^-53 of the sum of the terms' magnitudes, for either sum.  With a bias the 2 n skipped float roundings a
    component of eA:1592-1596 move the bias by at most bias_bound; a component of a transformed mean, float(t + b), then moves by at most
    that plus one float rounding either side (2 2^-24 |trn|), and a term (sumO - c trn / 2) trn iv by (|sumO| + |c trn|) iv per unit.
    All of it is divided by the counts."""
    A = matrix(kind, [x], st.L)
    bias, info = calc_bias(A, st, track=True)
    total, nC, t = mix_lhood(A, bias, st, track=True)
    n = len(st.used); dS = 2 * n * U64 * t["absT"].sum()
    if st.bSize:
        db = bias_bound(info, bias)
        dtrn = db[None, :] + 2 * U32 * np.abs(t["trn"][:, :st.bSize])
        dS += (t["sens"][:, :st.bSize] * dtrn).sum() + (0.5 * np.abs(t["ck"])[:, None] * t["iv"][:, :st.bSize] * dtrn ** 2).sum()
    dN = 2 * n * U64 * np.abs(t["ck"]).sum()
    L = total / nC
    return (dS + abs(L) * dN) / abs(nC) + 4 * U64 * abs(L)


# ---- the line search ---------------------------------------------------------------------------------------------------------------------------
def _sign(a, b):
    return abs(a) if b > 0.0 else -abs(a)


def _bound(mn, mx, q):
    """eA:94-106"""
    if q > mx:
        q = mx
    if q < mn:
        q = mn
    return q


def find_range(kind, rho):
    """eA:252-255, 1544-1548"""
    return (-rho, rho) if kind == RAPT else (-100.0, 100.0)


class NotANumber(Exception):
    """bracket returned false (eA:122-130)"""


def bracket(kind, f, ax, bx):
    """eA:109-180 -> (ax, bx, cx); f is calcLogLhood"""
    minim, maxim = find_range(kind, MAXIMUM_RHO - RHO_EPSILON)
    ax = _bound(minim, maxim, ax)
    fa = -f(ax)
    if math.isnan(fa):
        raise NotANumber()
    fb = -f(bx)
    if math.isnan(fb):
        raise NotANumber()
    if fb > fa:
        ax, bx = bx, ax; fb, fa = fa, fb
    cx = _bound(minim, maxim, bx + GOLD * (bx - ax))
    fc = -f(cx)
    if math.isnan(fc):
        raise NotANumber()
    while fb > fc:
        r = (bx - ax) * (fb - fc)
        q = (bx - cx) * (fb - fa)
        u = bx - ((bx - cx) * q - (bx - ax) * r) / (2.0 * _sign(max(abs(q - r), TINY), q - r))
        u = _bound(minim, maxim, u)
        ulim = _bound(minim, maxim, bx + GOLD_LIMIT * (cx - bx))
        if (bx - u) * (u - cx) > 0.0:
            fu = -f(u)
            if fu < fc:
                return bx, u, cx
            elif fu > fb:
                return ax, bx, u
            u = _bound(minim, maxim, cx + GOLD * (cx - bx))
            fu = -f(u)
        elif (cx - u) * (u - ulim) > 0.0:
            fu = -f(u)
            if fu < fc:
                bx, cx, u = cx, u, _bound(minim, maxim, cx + GOLD * (cx - bx))
                fb, fc, fu = fc, fu, -f(u)
        elif (u - ulim) * (ulim - cx) >= 0.0:
            u = ulim
            fu = -f(u)
        else:
            u = _bound(minim, maxim, cx + GOLD * (cx - bx))
            fu = -f(u)
        ax, bx, cx = bx, cx, u
        fa, fb, fc = fb, fc, fu
    return ax, bx, cx


def brents_method(f, ax, bx, cx):
    """eA:183-240 -> (xmin, logLhood)"""
    d = 0.0; e = 0.0
    a = min(ax, cx); b = max(ax, cx)
    x = w = v = bx
    fw = fv = fx = -f(x)
    for _ in range(MAX_ITNS):
        xm = 0.5 * (a + b)
        tol1 = TOLERANCE * abs(x) + Z_EPSILON; tol2 = 2.0 * tol1
        if abs(x - xm) <= (tol2 - 0.5 * (b - a)):
            return x, -fx
        if abs(e) > tol1:
            r = (x - w) * (fx - fv)
            q = (x - v) * (fx - fw)
            p = (x - v) * q - (x - w) * r
            q = 2.0 * (q - r)
            if q > 0.0:
                p = -p
            q = abs(q)
            etemp = e
            e = d
            if abs(p) >= abs(0.5 * q * etemp) or p <= q * (a - x) or p >= q * (b - x):
                e = a - x if x >= xm else b - x
                d = CONST_GOLD * e
            else:
                d = p / q
                u = x + d
                if u - a < tol2 or b - u < tol2:
                    d = _sign(tol1, xm - x)
        else:
            e = a - x if x >= xm else b - x
            d = CONST_GOLD * e
        u = x + d if abs(d) >= tol1 else x + _sign(tol1, d)
        fu = -f(u)
        if fu <= fx:
            if u >= x:
                a = x
            else:
                b = x
            v, w, x = w, x, u
            fv, fw, fx = fw, fx, fu
        else:
            if u < x:
                a = u
            else:
                b = u
            if fu <= fw or w == x:
                v = w; w = u; fv = fw; fw = fu
            elif fu <= fv or v == x or v == w:
                v = u; fv = fu
    raise ConsistencyError("Too many iterations of Brent's method")


def line_search(kind, f):
    """BLTEstimatorAdapt::estimate (eA:1659-1665: b = 0, a = b + 0.1) / the one-parameter branch of APTEstimatorBase::optimize (eA:821-830:
    a = -0.05, b = 0) -> (alpha or xmin, the points evaluated in order, their values); raises NotANumber or ConsistencyError"""
    pts, vals = [], []

    def g(x):
        v = float(f(float(x))); pts.append(float(x)); vals.append(v)
        return v
    a, b = (0.0 + 0.10, 0.0) if kind == RAPT else (-0.05, 0.0)
    ax, bx, cx = bracket(kind, g, a, b)
    x, _ = brents_method(g, ax, bx, cx)
    return x, pts, vals


class Replay(object):
    """calcLogLhood answered from a recorded trace: the point asked for must be the recorded one, as doubles bit for bit"""

    def __init__(self, points, values):
        self.points, self.values, self.i = list(points), list(values), 0

    def __call__(self, x):
        assert self.i < len(self.points), "the search asks for more points than the trace holds"
        assert np.float64(x).tobytes() == np.float64(self.points[self.i]).tobytes(), (self.i, x, self.points[self.i])
        self.i += 1
        return self.values[self.i - 1]


def estimate_node(kind, st):
    """estimate (eA:1659-1674, 1898-1929) of one node -> (conf, bias, points, values).  The bias: _calcBias under the matrix at alpha (BLT,
    eA:1667-1668) or under the matrix of the last trial point (SLAPT, eA:1926: _laurentCoeffs still holds its series)"""
    x, pts, vals = line_search(kind, lambda p: calc_log_lhood(kind, p, st))
    at = x if kind == RAPT else pts[-1]
    return x, calc_bias(matrix(kind, [at], st.L), st), pts, vals


# ---- parameters and their files --------------------------------------------------------------------------------------------------------------
TYPE_NAME = {RAPT: "RAPT", SLAPT: "SLAPT"}


class Param(object):
    """APTParamBase (tr:410-441): _conf doubles, the bias floats"""

    def __init__(self, regClass=0, conf=(), bias=()):
        self.regClass = regClass; self.conf = np.array(conf, f64).reshape(-1); self.bias = np.array(bias, f32).reshape(-1)

    def copy(self):
        return Param(self.regClass, self.conf.copy(), self.bias.copy())

    def text(self, typ):
        """ParamBase::write (tr:365-372) with RAPTParam / SLAPTParam::_putParams (tr:490-501, 542-551)"""
        s = "<AdaptType> %s\n<RegClass> %d\n<%sParam> %d\n" % (TYPE_NAME[typ], 1 if self.regClass == 0 else self.regClass, TYPE_NAME[typ], len(self.conf))
        s += "".join(" %g" % (abs(v) if typ == RAPT and i >= 2 and i % 2 == 0 else v) for i, v in enumerate(self.conf)) + "\n"
        if len(self.bias):
            s += "<BiasOffset> %d\n" % len(self.bias) + "".join(" %g" % float(v) for v in self.bias) + "\n"
        return s + "<EndClass>\n"


class Params(object):
    """the ParamTree (tr:789-950) of one speaker, of RAPT or of SLAPT parameters"""

    def __init__(self, text=None):
        self.map, self.type = {}, UNSPECIFIED
        if text:
            self.read(text)

    def hasIndex(self, rc):
        return rc in self.map

    def findAPT(self, rc, typ, useAncestor=True):
        """tr:862-896"""
        if self.type == UNSPECIFIED:
            self.type = typ
        elif self.type != typ:
            raise ConsistencyError("Tree not instantiated with %s parameters." % TYPE_NAME[typ])
        if rc == 0:
            raise IndexError_("Regression class index is zero")
        if rc in self.map:
            return self.map[rc]
        if not useAncestor:
            raise IndexError_("Could not find parameters for regression class %d." % rc)
        reg = rc // 2
        while reg > 0 and reg not in self.map:
            reg //= 2
        par = Param() if reg == 0 else self.map[reg].copy()
        par.regClass = rc; self.map[rc] = par
        return par

    def text(self):
        return "".join(self.map[k].text(self.type) for k in sorted(self.map))

    def read(self, text):
        """tr:927-950 with ParamBase::param / _readParams (tr:339-407): tokens are <Symbol> and numbers separated by white space"""
        self.map, self.type = {}, UNSPECIFIED
        tok = text.replace("<", " <").replace(">", "> ").split(); p = 0; new = {}; typ = UNSPECIFIED
        if text and not tok:
            raise TypeError_("Unable to determine adaptation type.")
        names = {"RAPT": RAPT, "SLAPT": SLAPT, "MLLR": 3}
        while p < len(tok):
            if tok[p] != "<AdaptType>":
                raise TypeError_("Unable to determine adaptation type.")
            t = names[tok[p + 1]]
            if t == 3:
                raise ParameterError("Attempted to read parameters of wrong type.")
            p += 2; par = Param()
            while tok[p] != "<EndClass>":
                sym = tok[p]; p += 1
                if sym == "<AdaptType>":
                    if names[tok[p]] != t:
                        raise ParameterError("Attempted to read parameters of wrong type.")
                    p += 1
                elif sym == "<RegClass>":
                    par.regClass = int(tok[p]); p += 1
                elif sym in ("<RAPTParam>", "<SLAPTParam>", "<MLLRParam>"):
                    if sym == "<RAPTParam>" and t == SLAPT:
                        raise ParameterError("Attempted to read SLAPT parameters.")
                    if sym != "<RAPTParam>" and t == RAPT:
                        raise ParameterError("Attempted to read RAPT parameters.")
                    n = int(tok[p]); p += 1
                    par.conf = np.array([float(x) for x in tok[p:p + n]], f64); p += n
                elif sym == "<BiasOffset>":
                    n = int(tok[p]); p += 1
                    par.bias = np.array([float(x) for x in tok[p:p + n]], f64).astype(f32); p += n
                else:
                    raise ParameterError("Unexpected symbol %s in conformal parameter file." % sym)
            p += 1
            new.setdefault(par.regClass, par)
            if typ == UNSPECIFIED:
                typ = t
            elif typ != t:
                raise ConsistencyError("Incorrect adaptation type for regression class %d." % par.regClass)
        if typ == UNSPECIFIED:
            raise ConsistencyError("Unable to determine adaptation type.")
        self.map, self.type = new, typ


# ---- estimation over the tree and the transformed means -----------------------------------------------------------------------------------------
def ttl_frames(c, gs):
    """EstimatorAdapt::ttlFrames (eA:1565-1572)"""
    t = 0.0
    for g in gs:
        t += float(c[g])
    return t


def plan_tree(classes, c, threshold, speaker=0):
    """LeafIterator::estimate's back-off (eA:3105-3121) for every leaf -> rows (speaker, node, leaf)"""
    leaves, nodes = tree_nodes(classes); thr = float(f32(threshold)); plan = []
    ttl = dict((k, ttl_frames(c, node_gaussians(classes, k))) for k in nodes)
    for leaf in leaves:
        rc = leaf
        while rc > 0:
            if ttl[rc] > thr:
                break
            rc //= 2
        if rc == 0:
            rc = 1
        plan.append((speaker, rc, leaf))
    return plan, ttl


def estimate_tree(kind, classes, mean, ivar, c, sumO, L, nSub, biasType, threshold, params=None, speaker=0, node_estimate=None):
    """estimateAdaptationParameters (eA:3064-3078) for a tree that is not MLLR: nothing is cleared or copied; the back-off node is estimated
    and stored under the leaf's class.  node_estimate(node, Stats) -> (conf, bias) replaces the search (it is the same for a node reached
    twice: the start point does not depend on what is stored).  -> (Params, plan, ok); a search that fails leaves `params` as it was"""
    params = Params() if params is None else params
    plan, _ = plan_tree(classes, c, threshold, speaker); done = {}
    new = Params(); new.type = params.type; new.map = dict((k, v.copy()) for k, v in params.map.items())
    for _, rc, leaf in plan:
        if rc not in done:
            st = Stats(mean, ivar, c, sumO, node_gaussians(classes, rc), L, nSub, biasType)
            try:
                done[rc] = node_estimate(rc, st) if node_estimate else estimate_node(kind, st)[:2]
            except (NotANumber, ConsistencyError):
                return params, plan, False
        par = new.findAPT(leaf, kind)
        par.conf = np.array([done[rc][0]], f64); par.bias = np.array(done[rc][1], f32)
    return new, plan, True


def tree_node(params, rc):
    """BaseTree::node(idx, useAncestor = true) (tr:2030-2049) over the classes of the parameters"""
    if rc == 0:
        raise IndexError_("Regression class index must be >= 1")
    idx = rc
    if params.hasIndex(idx):
        return idx
    while idx > 1:
        idx //= 2
        if params.hasIndex(idx):
            return idx
    raise KeyError_("Could not find node %d." % idx)


def transform_tree(params, classes, mean, L, nSub):
    """TransformerTree::transform (tr:2149-2163) with BLTTransformer / SLAPTTransformer -> the new means"""
    mean = np.asarray(mean, f32); out = np.empty_like(mean)
    where = np.array([tree_node(params, int(c)) for c in classes])
    for node in sorted(set(where)):
        sel = where == node; p = params.map[node]
        out[sel] = transform(matrix(params.type, p.conf, L), mean[sel], nSub, p.bias)
    return out
