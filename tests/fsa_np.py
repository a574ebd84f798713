"""numpy restatement of FeatureSpaceAdaptationFeature (asr/train/fsa.{h,cc}, "fsa"; the nearest Gaussian of asr/gaussian/codebookBasic.cc
"cB"): the yardstick of the feature-space adaptation tests.

Float / double placement is spelled out: np.float32 where the reference holds or multiplies floats (gamma, beta, mean x invCov, the pattern),
fp64 for its gsl matrices, sums sequential in item order.  estimate() follows the reference through singular value decompositions (of every
G_i once, of A for every row); variant="inv" takes the cofactors from numpy.linalg.inv / det instead, the legitimate other order of the
same arithmetic that the device tests are measured against.  Nothing here is taken from the reference's text.
Layout as in the library: Gaussians of all codebooks in one run, codebook k owning rows off[k]..off[k+1]."""
import math
import struct

import numpy as np

f32 = np.float32
MAX_SV_RATIO = 1.0e-07               # fsa:330


class IndexError_(Exception):
    pass


class ConsistencyError(Exception):
    pass


class DimensionError(Exception):
    pass


class IOError_(Exception):
    pass


def nearest(refN, mean, ivar, det, x, k):
    """the index (inside codebook k) of the one-hot addCount of _scoreOpt (cB:431-554): fp32, d ascending, strict '<'"""
    off = np.concatenate([[0], np.cumsum(refN)]); a, b = int(off[k]), int(off[k + 1]); D = mean.shape[1]
    pi = f32(math.log(2.0 * math.pi) * D)
    dist = (pi + det[a:b]).astype(f32)
    x = np.asarray(x, f32)
    for d in range(D):
        diff = (mean[a:b, d] - x[d]).astype(f32)
        dist = (dist + ((diff * diff).astype(f32) * ivar[a:b, d]).astype(f32)).astype(f32)
    best, idx = f32(1e20), 0
    for r in range(b - a):
        if dist[r] < best:
            best, idx = dist[r], r
    return idx


class Fsa(object):
    """the state of a FeatureSpaceAdaptationFeature for a diagonal model; track=True also keeps the sums of the magnitudes of the terms"""

    def __init__(self, refN, mean, ivar, det, nAccu=1, nTran=1, track=False):
        self.refN = [int(r) for r in refN]; self.K = len(self.refN); self.off = np.concatenate([[0], np.cumsum(self.refN)]).astype(int)
        self.mean = np.array(mean, f32).reshape(int(self.off[-1]), -1); self.ivar = np.array(ivar, f32).reshape(self.mean.shape)
        self.det = np.array(det, f32).reshape(-1); self.D = D = self.mean.shape[1]; self.nAccu, self.nTran, self.track = nAccu, nTran, track
        self.on = np.zeros(self.K, bool); self.topN = 1; self.shift = f32(1.0)
        self.count = np.zeros(nAccu); self.beta = np.zeros(nAccu, f32)
        self.z = np.zeros((nAccu, D, D + 1)); self.G = np.zeros((nAccu, D, D + 1, D + 1))
        self.zabs = np.zeros_like(self.z); self.Gabs = np.zeros_like(self.G); self.items = np.zeros(nAccu, int)
        self.W = np.zeros((nTran, D, D + 1))
        for t in range(nTran):
            self.clear(t)
        self._tril = np.tril(np.ones((D + 1, D + 1), bool))

    # ---- estimation set-up
    def add(self, dsX):
        if not 0 <= dsX < self.K:
            raise IndexError_(dsX)
        self.on[dsX] = True

    def addAll(self):
        self.on[:] = True

    def _accu(self, a):
        if not 0 <= a < self.nAccu:
            raise IndexError_("Bad accu index: %d should be less then %d." % (a, self.nAccu))

    def _tran(self, t):
        if not 0 <= t < self.nTran:
            raise IndexError_("Bad transformation index: %d should be less then %d." % (t, self.nTran))

    # ---- accumulation
    def accu_one(self, dsX, xScore, xSrc, accuX, gamma):
        """_accuOne (fsa:187-245); returns the Gaussian (model row) or None for a masked distribution"""
        if not self.on[dsX]:
            return None
        self.count[accuX] += 1.0
        g = int(self.off[dsX]) + nearest(self.refN, self.mean, self.ivar, self.det, xScore, dsX)
        gamma = f32(gamma)
        self.beta[accuX] = f32(self.beta[accuX] + gamma)
        xi = np.concatenate([[1.0], np.asarray(xSrc, f32).astype(np.float64)])
        c = float(gamma)                                                     # gamma * addCount (= 1.0f), a float, into a double
        cz = c * (self.mean[g] * self.ivar[g]).astype(f32).astype(np.float64)     # fsa:223: the product of two floats is a float
        cg = c * self.ivar[g].astype(np.float64)                             # fsa:233
        tz = cz[:, None] * xi[None, :]
        tg = (cg[:, None] * xi[None, :])[:, :, None] * xi[None, None, :]      # (c x_j) x_k, rounded after each product
        tg = np.where(self._tril[None], tg, 0.0)
        self.z[accuX] += tz; self.G[accuX] += tg
        if self.track:
            self.zabs[accuX] += np.abs(tz); self.Gabs[accuX] += np.abs(tg); self.items[accuX] += 1
        return g

    def accumulate_items(self, xScore, xSrc, frame, dist, gamma, accu):
        return [self.accu_one(int(d), xScore[f], xSrc[f], int(a), g) for f, d, g, a in zip(frame, dist, gamma, accu)]

    def accumulate(self, xScore, xSrc, path, accuX=0, factor=1.0):
        """accumulate(path) (fsa:282-297); an entry None is a name the distribution set does not know: the frame index does not advance"""
        frameX = 0
        for ds in path:
            if ds is None:
                continue
            self.accu_one(int(ds), xScore[frameX], xSrc[frameX], accuX, factor); frameX += 1
        return frameX

    def accumulate_lattice(self, xScore, xSrc, links, accuX=0, factor=1.0):
        """accumulateLattice (fsa:299-321); links: (input, gamma, start, end).  frameX is incremented in the loop header AND in the call."""
        cnt = 0
        for inp, gamma, start, end in links:
            if inp == 0 or gamma > 10.0:
                continue
            post = f32(float(f32(factor)) * math.exp(-gamma)); cnt += 1
            frameX = start
            while frameX <= end:
                self.accu_one(inp - 1, xScore[frameX], xSrc[frameX], accuX, post); frameX += 1
                frameX += 1
        return cnt

    def accumulate_fast(self, x, dist, accuX=0, gamma=1.0):
        """the statistics of frames x with distributions dist in one einsum each: the same sums in another order and without the reference's
        intermediate roundings -- for tests of estimate() that do not compare bits"""
        x = np.asarray(x, f32); T = len(x)
        g = np.array([int(self.off[d]) + nearest(self.refN, self.mean, self.ivar, self.det, x[t], d) for t, d in enumerate(dist)])
        xi = np.concatenate([np.ones((T, 1)), x.astype(np.float64)], 1); c = float(f32(gamma))
        cz = c * (self.mean[g] * self.ivar[g]).astype(f32).astype(np.float64); cg = c * self.ivar[g].astype(np.float64)
        self.z[accuX] += np.einsum("ti,tn->in", cz, xi)
        self.G[accuX] += np.where(self._tril[None], np.einsum("ti,tj,tk->ijk", cg, xi, xi, optimize=True), 0.0)
        self.count[accuX] += T
        for t in range(T):
            self.beta[accuX] = f32(self.beta[accuX] + f32(gamma))

    def zeroAccu(self, a=0):
        self._accu(a); self.count[a] = 0.0; self.beta[a] = 0.0; self.z[a] = 0.0; self.G[a] = 0.0; self.zabs[a] = 0.0; self.Gabs[a] = 0.0; self.items[a] = 0

    def scaleAccu(self, scale, a=0):
        self._accu(a); s = float(f32(scale))
        self.count[a] *= s; self.beta[a] = f32(self.beta[a] * f32(scale)); self.z[a] = self.z[a] * s; self.G[a] = self.G[a] * s

    def addAccu(self, a, b, factor=1.0):
        fa = float(f32(factor))
        self.count[a] += fa * self.count[b]; self.beta[a] = f32(self.beta[a] + f32(f32(factor) * self.beta[b]))
        self.z[a] = self.z[a] + fa * self.z[b]; self.G[a] = self.G[a] + fa * self.G[b]

    # ---- estimation
    def sym(self, a):
        """_makeSymmetric (fsa:323-328): the lower triangle copied up"""
        L = np.tril(self.G[a]); return L + np.transpose(np.tril(self.G[a], -1), (0, 2, 1))

    def aux(self, W, a):
        """Q(W) = beta log|det A| - 1/2 sum_i w_i G_i w_i^T + sum_i w_i . z_i"""
        Gs = self.sym(a); s, ld = np.linalg.slogdet(W[:, 1:])
        return float(self.beta[a]) * ld - 0.5 * sum(W[i] @ Gs[i] @ W[i] for i in range(self.D)) + float((W * self.z[a]).sum())

    def cofactor(self, W, i0, variant="svd", flip=False):
        D = self.D; A = W[:, 1:]
        if not np.isfinite(A).all():                                         # LAPACK refuses what gsl carries on: NaN in, NaN out
            return np.full(D + 1, np.nan)
        if variant == "svd":                                                 # _calcCofactor, fsa:332-361
            U, s, Vt = np.linalg.svd(A)
            keep = (s / s[0]) >= MAX_SV_RATIO
            inv = (Vt.T * np.where(keep, 1.0 / np.where(keep, s, 1.0), 0.0)[None, :]) @ U.T
            det = float(np.prod(s[keep]))
        else:
            inv = np.linalg.inv(A); det = float(np.linalg.det(A))
        p = np.zeros(D + 1); p[1:] = det * inv[:, i0]
        return -p if flip else p

    def estimate(self, iterN=1, accuX=0, tranX=0, variant="svd", flip=False, after_row=None, W0=None):
        """estimate (fsa:363-433) -> W (also stored, whatever it holds: the reference stores NaN as well)"""
        self._accu(accuX); self._tran(tranX)
        D = self.D; beta = float(self.beta[accuX]); z = self.z[accuX]; Gs = self.sym(accuX)
        W = np.array(self.W[tranX] if W0 is None else W0, np.float64)
        dec = []
        for i in range(D):
            U, s, Vt = np.linalg.svd(Gs[i])
            inv = np.where((s / s[0]) >= MAX_SV_RATIO, 1.0 / s, 0.0) if s[0] > 0 else np.zeros_like(s)
            dec.append((U, inv, Vt))
        pinv = lambda i, v: dec[i][0] @ ((dec[i][2] @ v) * dec[i][1])        # U diag(1/s) V^T v, fsa:380-387
        with np.errstate(all="ignore"):
            for it in range(iterN):
                for i in range(D):
                    p = self.cofactor(W, i, variant, flip)
                    d = pinv(i, p)
                    term1 = float(d @ p); term2 = float(d @ z[i])
                    term3 = term2 / (2 * term1); term4 = math.sqrt(term3 * term3 + beta / term1) if term3 * term3 + beta / term1 >= 0 else float("nan")
                    alpha1 = -1.0 * term3 + term4; alpha2 = -1.0 * term3 - term4
                    k1 = beta * np.log(np.abs(alpha1 * term1 + term2)) - 0.5 * alpha1 * alpha1 * term1
                    k2 = beta * np.log(np.abs(alpha2 * term1 + term2)) - 0.5 * alpha2 * alpha2 * term1
                    alpha = alpha2 if k2 > k1 else alpha1
                    W[i] = pinv(i, alpha * p + z[i])
                    if after_row is not None:
                        after_row(it, i, W)
        self.W[tranX] = W
        return W

    def clear(self, t=0):
        self._tran(t); self.W[t] = 0.0
        for i in range(self.D):
            self.W[t, i, i + 1] = 1.0

    def compareTransform(self, x, y):
        """fsa:483-503: columns 0 .. dimN - 1 -- the bias and all of A but its last column"""
        self._tran(x); self._tran(y); D = self.D
        tmp = self.W[x][:, :D] - self.W[y][:, :D]
        s = 0.0
        for i in range(D):
            for j in range(D):
                s += tmp[i, j] * tmp[i, j]
        return f32(s)

    # ---- the transform
    def apply(self, x, tranX=0, shift=1.0):
        """next (fsa:247-280) for rows x [N][D]; tranX an int or one index per row"""
        x = np.asarray(x, f32); N, D = x.shape; out = np.zeros((N, D), f32)
        tr = np.full(N, tranX, int) if np.isscalar(tranX) else np.asarray(tranX, int)
        sh = f32(shift)
        for n in range(N):
            w = self.W[tr[n]]
            if sh == -1:
                out[n] = (w[:, 0] + x[n].astype(np.float64)).astype(f32)
            else:
                s = float(sh) * w[:, 0]
                for i in range(D):
                    s = s + w[:, i + 1] * float(x[n, i])
                out[n] = s.astype(f32)
        return out

    # ---- files: big-endian floats (btk/common/mach_ind_io.cc)
    def accu_bytes(self, a=0):
        """saveAccu (fsa:505-533)"""
        self._accu(a); D = self.D
        vals = np.concatenate([[f32(self.count[a]), self.beta[a]], self.z[a].astype(f32).ravel(), self.G[a].astype(f32).ravel()]).astype(">f4")
        return b"SAS" + struct.pack(">i", D) + vals.tobytes()

    def load_accu_bytes(self, data, a=0, factor=1.0):
        """loadAccu (fsa:535-583): ADDS factor x the file"""
        self._accu(a); D = self.D
        if data[:3] != b"SAS":
            raise ConsistencyError("Couldn't find magic SAS")
        if struct.unpack(">i", data[3:7])[0] != D:
            raise DimensionError("Dimension mismatch")
        v = np.frombuffer(data[7:], ">f4").astype(f32); fa = float(f32(factor))
        self.count[a] += float(f32(f32(factor) * v[0]))
        self.beta[a] = f32(float(self.beta[a]) + fa * float(v[1]))
        nz = D * (D + 1)
        self.z[a] = self.z[a] + fa * v[2:2 + nz].astype(np.float64).reshape(D, D + 1)
        self.G[a] = self.G[a] + fa * v[2 + nz:2 + nz + nz * (D + 1)].astype(np.float64).reshape(D, D + 1, D + 1)

    def tran_bytes(self, t=0):
        """save (fsa:585-603)"""
        self._tran(t)
        return b"SAW" + struct.pack(">i", self.D) + self.W[t].astype(f32).astype(">f4").tobytes()

    def load_tran_bytes(self, data, t=0):
        """load (fsa:605-635)"""
        self._tran(t); D = self.D
        if data[:3] != b"SAW":
            raise IOError_("Couldn't find magic SAW")
        if struct.unpack(">i", data[3:7])[0] != D:
            raise DimensionError("Dimension mismatch")
        self.W[t] = np.frombuffer(data[7:7 + 4 * D * (D + 1)], ">f4").astype(np.float64).reshape(D, D + 1)


def synth_model(K, refN, D, seed):
    """a random diagonal model: refN Gaussians (an int or one per codebook) per codebook"""
    rng = np.random.default_rng(seed)
    refN = np.full(K, refN, np.int32) if np.isscalar(refN) else np.asarray(refN, np.int32); G = int(refN.sum())
    mean = rng.standard_normal((G, D)).astype(f32) * f32(2.0)
    ivar = (1.0 / rng.uniform(0.5, 2.0, (G, D))).astype(f32)
    det = (-np.log(ivar.astype(np.float64)).sum(1)).astype(f32)
    val = np.full(G, 0.0, f32)
    for k in range(K):
        a = int(refN[:k].sum()); w = rng.uniform(0.5, 1.5, int(refN[k])); val[a:a + int(refN[k])] = (-np.log(w / w.sum())).astype(f32)
    return dict(refN=refN, mean=mean, ivar=ivar, det=det, val=val)


def synth_speaker(model, T, seed, a_scale=0.15, b_scale=0.3):
    """T frames drawn from the model (one distribution per frame) and passed through the INVERSE of a known affine map (A0 = I + a_scale N/sqrt(D),
    b0 = b_scale N), so that W0 = (b0 | A0) maps them back -> (x [T][D] float32, dist [T], W0 [D][D + 1])"""
    rng = np.random.default_rng(seed); refN = np.asarray(model["refN"]); K = len(refN); D = model["mean"].shape[1]
    off = np.concatenate([[0], np.cumsum(refN)])
    A0 = np.eye(D) + a_scale * rng.standard_normal((D, D)) / math.sqrt(D); b0 = b_scale * rng.standard_normal(D)
    dist = rng.integers(0, K, T); g = off[dist] + rng.integers(0, refN[dist])
    y = model["mean"][g].astype(np.float64) + rng.standard_normal((T, D)) / np.sqrt(model["ivar"][g].astype(np.float64))
    x = np.linalg.solve(A0, (y - b0).T).T
    return np.ascontiguousarray(x, f32), dist.astype(np.int32), np.concatenate([b0[:, None], A0], 1)
