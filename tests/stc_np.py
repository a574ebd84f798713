"""numpy restatement of STCTransformer / LDATransformer (asr/adapt/transform.cc:1788-1984, "tr") and STCEstimator / LDAEstimator
(asr/train/estimateAdapt.cc:2203-3036, "eA") for one sub-feature: the yardstick of the STC / LDA tests.

Float / double placement is spelled out: np.float32 where the reference holds or multiplies floats (count = addCount x factor, wgt = invCov x
count, count / invCov, the differences pattern - mean), fp64 for its gsl matrices, sums sequential in item order.  Only the lower triangle is
written by accumulation; sym() is copyUpperTriangle, which the reference runs on every read through sumOsq() / regSq() / within() / ...
Stc.update() follows the reference through an LU decomposition of A per row (variant="lu", with the determinant itself); variant="inv" takes
A^-1 and the determinant's sign from numpy.linalg, the legitimate other order of the same arithmetic that the device is measured against.
Nothing here is taken from the reference's text.  Layout as in the library: Gaussians of all codebooks in one run."""
import os
import struct
import subprocess

import numpy as np

from tests.fsa_np import nearest, synth_model                              # noqa: F401  the same model layout and nearest Gaussian

f32 = np.float32
MAX_ITNS = 10                        # eA:2389


class DimensionError(Exception):
    pass


class NumericError(Exception):
    pass


def sym(M):
    """copyUpperTriangle (eA:2658-2663) of one matrix or a stack of them: a symmetric copy of the lower triangle"""
    L = np.tril(M); return L + np.swapaxes(np.tril(M, -1), -1, -2)


# ---------------------------------------------------------------------------------------------------------------- LU as gsl_linalg_LU_*
def lu_decomp(A):
    """-> (LU, perm, signum): Doolittle with partial pivoting, row by row elimination"""
    a = np.array(A, np.float64); n = len(a); perm = np.arange(n); sign = 1
    for k in range(n):
        p = k + int(np.argmax(np.abs(a[k:, k])))
        if p != k:
            a[[k, p]] = a[[p, k]]; perm[[k, p]] = perm[[p, k]]; sign = -sign
        if a[k, k] != 0.0:
            a[k + 1:, k] = a[k + 1:, k] / a[k, k]
            a[k + 1:, k + 1:] -= a[k + 1:, k, None] * a[None, k, k + 1:]
    return a, perm, sign


def lu_invert(lu, perm):
    n = len(lu); x = np.eye(n)[perm]
    for k in range(n):                                                     # L y = P b, unit diagonal
        x[k + 1:] -= lu[k + 1:, k, None] * x[None, k]
    for k in range(n - 1, -1, -1):                                         # U x = y
        x[k] = x[k] / lu[k, k]
        x[:k] -= lu[:k, k, None] * x[None, k]
    return x


def lu_inv_det(A):
    lu, perm, sign = lu_decomp(A)
    return lu_invert(lu, perm), sign * float(np.prod(np.diag(lu)))


class Stc(object):
    """one STCEstimator over a diagonal model; track=True also keeps the sums of the magnitudes of the terms"""

    def __init__(self, refN, mean, ivar, det, cascade=False, mmi=False, track=False):
        self.refN = [int(r) for r in refN]; self.K = len(self.refN); self.off = np.concatenate([[0], np.cumsum(self.refN)]).astype(int)
        self.mean = np.array(mean, f32).reshape(int(self.off[-1]), -1); self.ivar = np.array(ivar, f32).reshape(self.mean.shape)
        self.det = np.array(det, f32).reshape(-1); self.D = D = self.mean.shape[1]
        self.cascade, self.mmi, self.track = cascade, mmi, track
        self.A = np.eye(D); self.Ainv = np.eye(D); self.E = 0.0
        self._tril = np.tril(np.ones((D, D), bool))
        self.zero()

    def zero(self):
        D = self.D
        self.count = self.denCount = self.totalPr = 0.0; self.totalT = 0
        self.sumOsq = np.zeros((D, D, D)); self.regSq = np.zeros((D, D, D))
        self.Sabs = np.zeros((D, D, D)); self.Rabs = np.zeros((D, D, D)); self.items = 0; self.denItems = 0

    def transform(self, x):
        """_transform (tr:1866-1879): a double sum, j ascending"""
        x = np.atleast_2d(np.asarray(x, f32)).astype(np.float64); out = np.zeros((x.shape[0], self.D))
        for j in range(self.D):
            out = out + x[:, j, None] * self.A[None, :, j]
        return out.astype(f32)

    def accu_one(self, dsX, xScore, xSrc, factor):
        """one frame of accumulate (eA:2269-2283) -> the Gaussian (model row)"""
        g = int(self.off[dsX]) + nearest(self.refN, self.mean, self.ivar, self.det, xScore, dsX)
        block = np.asarray(xSrc, f32)
        if self.cascade:
            block = self.transform(block)[0]
        factor = f32(factor); iv = self.ivar[g]
        # accumulateW1, eA:2569-2606
        count = f32(f32(1.0) * factor)
        if count > 0.0:
            self.count += float(count)
        elif count < 0.0:
            self.denCount -= float(count)
        o = (block - self.mean[g]).astype(f32).astype(np.float64)
        wgt = (iv * count).astype(f32).astype(np.float64)
        t = (wgt[:, None] * o[None, :])[:, :, None] * o[None, None, :]       # (wgt o_i) o_j
        t = np.where(self._tril[None], t, 0.0)
        self.sumOsq += t; self.items += 1
        if self.track:
            self.Sabs += np.abs(t)
        # accumulateW2, eA:2609-2651
        if not factor > 0.0:
            c2 = f32(f32(1.0) * f32(-factor)); P = np.zeros((self.D, self.D)); Pabs = np.zeros((self.D, self.D))
            for col in range(self.D):
                a = self.Ainv[:, col]; w = float(f32(c2 / iv[col]))
                t2 = np.where(self._tril, (w * a)[:, None] * a[None, :], 0.0)
                P += t2; Pabs += np.abs(t2)
            self.regSq += iv.astype(np.float64)[:, None, None] * P[None]; self.denItems += 1
            if self.track:
                self.Rabs += iv.astype(np.float64)[:, None, None] * Pabs[None]
        return g

    def accumulate(self, xScore, xSrc, path, factor=1.0, scores=None):
        """accumulate(path, factor) (eA:2265-2294); scores: the distributions' scores of the frames (totalPr), zeros when not given"""
        total = 0.0
        for t, ds in enumerate(path):
            self.accu_one(int(ds), xScore[t], xSrc[t], factor)
            total += float(scores[t]) if scores is not None else 0.0
        if f32(factor) > 0.0:
            self.totalPr += total; self.totalT += len(path)
        else:
            self.totalPr += -total
        return len(path)

    # ---- estimation
    def G(self, E):
        return sym(self.sumOsq) + E * sym(self.regSq)

    def make_pos_def(self, minE=1.0, multE=1.0, cap=200):
        """eA:2689-2711 (the reference has no cap: it would not return)"""
        E = minE
        for _ in range(cap):
            if all(np.linalg.eigvalsh(g).min() > 0.0 for g in self.G(E)):
                self.E = E * multE; return self.E
            E *= 2.0
        raise NumericError("statistics cannot be made positive definite")

    def gamma(self, E):
        return self.denCount * E if self.mmi else self.count

    def aux(self, A, E=None):
        """2 gamma log |det A| - sum_d a_d G_d a_d^T: what a row update maximises (NOT the value calcAuxFunc prints, eA:2665-2686)"""
        E = self.E if E is None else E; G = self.G(E)
        return 2.0 * self.gamma(E) * np.linalg.slogdet(A)[1] - float(np.einsum("di,dij,dj->", A, G, A))

    def update(self, A, minE=1.0, multE=1.0, variant="lu", after_row=None, itns=MAX_ITNS):
        """_update (eA:2387-2464) from the matrix A -> the new matrix"""
        A = np.array(A, np.float64); D = self.D
        E = self.make_pos_def(minE, multE); G = self.G(E); gamma = self.gamma(E)
        Gi = np.stack([lu_inv_det(g)[0] if variant == "lu" else np.linalg.inv(g) for g in G])
        for it in range(itns):
            for d in range(D):
                if variant == "lu":
                    inv, det = lu_inv_det(A); c = det * inv[:, d]
                else:
                    c = np.linalg.slogdet(A)[0] * np.linalg.inv(A)[:, d]
                v = Gi[d].T @ c; f = float(v @ c)
                if not f > 0.0:
                    raise NumericError("Inner product %f <= 0.0 for dimension %d." % (f, d))
                A[d] = np.sqrt(gamma / f) * v
                if after_row is not None:
                    after_row(it, d, A)
        return A

    def estimate(self, minE=1.0, multE=1.0, variant="lu", **kw):
        """estimate (eA:2296-2316)"""
        B = self.update(self.A, minE, multE, variant, **kw)
        self.A = B @ self.A if self.cascade else B
        self.Ainv = lu_inv_det(self.A)[0] if variant == "lu" else np.linalg.inv(self.A)
        return self.A

    # ---- files
    def accu_bytes(self):
        self.sumOsq = sym(self.sumOsq); self.regSq = sym(self.regSq)         # save reads through sumOsq() / regSq()
        return (struct.pack(">ii", self.D, 1) + struct.pack(">fff", f32(self.count), f32(self.denCount), f32(self.totalPr)) + struct.pack(">i", self.totalT)
                + self.sumOsq.astype("=f8").tobytes() + self.regSq.astype("=f8").tobytes())

    def load_accu_bytes(self, data):
        D = self.D; sub, ns = struct.unpack(">ii", data[:8])
        if sub != D:
            raise DimensionError("Sub-feature lengths (%d vs. %d) do not match." % (D, sub))
        if ns != 1:
            raise DimensionError("Number of sub-features (%d vs. %d) do not match." % (1, ns))
        c, dc, pr = struct.unpack(">fff", data[8:20]); T, = struct.unpack(">i", data[20:24])
        m = np.frombuffer(data[24:24 + 16 * D ** 3], "=f8").reshape(2, D, D, D)
        self.count += c; self.denCount += dc; self.totalPr += pr; self.totalT += T
        self.sumOsq = self.sumOsq + m[0]; self.regSq = self.regSq + m[1]

    def tran_bytes(self):
        return self.A.astype("=f8").tobytes()

    def load_tran_bytes(self, data):
        self.A = np.frombuffer(data, "=f8").reshape(self.D, self.D).copy(); self.Ainv = lu_inv_det(self.A)[0]

    def trans_matrix(self):
        return self.A.astype(f32)

    def save_float_bytes(self, trans=None):
        """STCEstimator::save(fileName, trans) (eA:2327-2346): a float product, k ascending"""
        T = self.trans_matrix()
        if trans is not None:
            tr = np.asarray(trans, f32); out = np.zeros((self.D, self.D), f32)
            for k in range(self.D):
                out = (out + (T[:, k, None] * tr[None, k, :]).astype(f32)).astype(f32)
            T = out
        return T.astype("=f4").tobytes()


def yardstick(s, Alu, Ainv):
    """the larger of the restatement's own LU / inv difference and 10 D 2^-53 max_d cond(G_d) max |A|"""
    kappa = max(np.linalg.cond(g) for g in s.G(s.E))
    return max(float(np.abs(Alu - Ainv).max()), 10 * s.D * 2.0 ** -53 * kappa * float(np.abs(Alu).max()))


class Lda(object):
    """one LDAEstimator; mu0 = Gaussian 0 of the global codebook, globalRefN its size"""

    def __init__(self, refN, mean, ivar, det, mu0, globalRefN, track=False):
        self.refN = [int(r) for r in refN]; self.K = len(self.refN); self.off = np.concatenate([[0], np.cumsum(self.refN)]).astype(int)
        self.mean = np.array(mean, f32).reshape(int(self.off[-1]), -1); self.ivar = np.array(ivar, f32).reshape(self.mean.shape)
        self.det = np.array(det, f32).reshape(-1); self.D = D = self.mean.shape[1]; self.mu0 = np.asarray(mu0, f32); self.globalRefN = int(globalRefN)
        self.track = track; self.L = np.eye(D); self._tril = np.tril(np.ones((D, D), bool)); self.zero()

    def zero(self):
        D = self.D; self.count = 0.0; self.items = 0
        self.within = np.zeros((D, D)); self.between = np.zeros((D, D)); self.mixture = np.zeros((D, D))     # the reference starts from unset memory
        self.abs = np.zeros((3, D, D))

    def accu_one(self, dsX, xScore, xSrc, factor):
        """Accu::accumulate (eA:2989-3036)"""
        if self.refN[dsX] != self.globalRefN:
            raise DimensionError("Codebook sizes (%d and %d) do not match." % (self.refN[dsX], self.globalRefN))
        g = int(self.off[dsX]) + nearest(self.refN, self.mean, self.ivar, self.det, xScore, dsX)
        x = np.asarray(xSrc, f32); count = f32(f32(1.0) * f32(factor)); self.count += float(count); c = float(count)
        obs = [(x - self.mean[g]).astype(f32), (self.mean[g] - self.mu0).astype(f32), (x - self.mu0).astype(f32)]
        for k, (o, name) in enumerate(zip(obs, ("within", "between", "mixture"))):
            o = o.astype(np.float64); t = np.where(self._tril, (c * o)[:, None] * o[None, :], 0.0)
            setattr(self, name, getattr(self, name) + t)
            if self.track:
                self.abs[k] += np.abs(t)
        self.items += 1
        return g

    def scale(self):
        """scaleScatterMatrices (eA:2921-2932): in place"""
        self.within = self.within / self.count; self.between = self.between / self.count; self.mixture = self.mixture / self.count

    def solve(self, W, B):
        """_update (eA:2793-2836) through numpy.linalg.eigh -> (L, eigenvalues of W, eigenvalues of the whitened B descending)"""
        l, V = np.linalg.eigh(W)
        s = np.where(l <= 0.0, 0.0, 1.0 / np.sqrt(np.where(l <= 0.0, 1.0, l))); Wh = V * s[None, :]
        S = Wh.T @ B @ Wh; m, U = np.linalg.eigh(sym(S)); order = np.argsort(-m, kind="stable")
        return (Wh @ U[:, order]).T, l, m[order]

    def estimate(self):
        self.scale(); self.L, lw, lb = self.solve(sym(self.within), sym(self.between))
        return self.L

    def apply(self, x, outDim):
        """LDATransformer::next (tr:1948-1955)"""
        x = np.atleast_2d(np.asarray(x, f32)).astype(np.float64); out = np.zeros((x.shape[0], outDim))
        for j in range(self.D):
            out = out + x[:, j, None] * self.L[None, :outDim, j]
        return out.astype(f32)

    def accu_bytes(self):
        self.within, self.between, self.mixture = sym(self.within), sym(self.between), sym(self.mixture)
        return (struct.pack(">ii", self.D, 1) + self.within.astype("=f8").tobytes() + self.between.astype("=f8").tobytes() + self.mixture.astype("=f8").tobytes()
                + struct.pack(">f", f32(self.count)))

    def load_accu_bytes(self, data):
        D = self.D; sub, ns = struct.unpack(">ii", data[:8])
        if sub != D:
            raise DimensionError("Sub-feature lengths (%d vs. %d) do not match." % (D, sub))
        if ns != 1:
            raise DimensionError("Number of sub-features (%d vs. %d) do not match." % (1, ns))
        m = np.frombuffer(data[8:8 + 24 * D * D], "=f8").reshape(3, D, D); c, = struct.unpack(">f", data[8 + 24 * D * D:12 + 24 * D * D])
        self.within = self.within + m[0]; self.between = self.between + m[1]; self.mixture = self.mixture + m[2]; self.count += c

    def tran_bytes(self):
        """save writes float32 (tr:1967-1973)"""
        return self.L.astype("=f4").tobytes()

    def load_tran_bytes(self, data):
        """load reads float64 (tr:1979-1984)"""
        self.L = np.frombuffer(data, "=f8").reshape(self.D, self.D).copy()


# ---------------------------------------------------------------------------------------------------------------- synthetic data
def synth_stc(K, R, D, T, seed, spread=8.0):
    """a model whose Gaussians share the diagonal covariance Lambda in a rotated space, and T frames drawn from Gaussians of covariance
    Rot^T Lambda Rot around its means -> (model, x [T][D] float32, dist [T], Rot, Lambda)"""
    rng = np.random.default_rng(seed); m = synth_model(K, R, D, seed)
    lam = np.exp(rng.uniform(-0.5 * np.log(spread), 0.5 * np.log(spread), D)); Rot = np.linalg.qr(rng.standard_normal((D, D)))[0]
    G = len(m["mean"]); m["ivar"] = np.tile((1.0 / lam).astype(f32), (G, 1)); m["det"] = np.full(G, np.log(lam).sum(), f32)
    refN = np.asarray(m["refN"]); off = np.concatenate([[0], np.cumsum(refN)])
    dist = rng.integers(0, K, T); g = off[dist] + rng.integers(0, refN[dist])
    x = m["mean"][g].astype(np.float64) + (rng.standard_normal((T, D)) * np.sqrt(lam)) @ Rot
    return m, np.ascontiguousarray(x, f32), dist.astype(np.int32), Rot, lam


def offdiag_ratio(M):
    """off-diagonal energy over the whole energy"""
    return float((M ** 2).sum() - (np.diag(M) ** 2).sum()) / float((M ** 2).sum())


def synth_scatter(D, seed, step=1.25):
    """within = C C^T and between with a known spectrum: the generalised eigenvalues are step^-k (neighbours differ by >= 10 %)"""
    rng = np.random.default_rng(seed); C = np.eye(D) + 0.3 * rng.standard_normal((D, D)) / np.sqrt(D); W = C @ C.T
    Q = np.linalg.qr(rng.standard_normal((D, D)))[0]; lam = 3.0 * step ** -np.arange(D, dtype=np.float64)
    B = (C @ Q) @ np.diag(lam) @ (C @ Q).T                                                    # C^-1 B C^-T = Q diag(lam) Q^T
    return sym(W), sym(B), lam


# ---------------------------------------------------------------------------------------------------------------- the device's phases on the host
HOST_SRC = r"""
#include <cstdio>
#include <vector>
#include "stc_rows.h"
using namespace dsr;
int main(int argc, char** argv) {
  FILE* f = fopen(argv[1], "rb"); double hd[3]; if (!f || fread(hd, 8, 3, f) != 3) return 9;
  const int mode = (int) hd[0], D = (int) hd[1], n = D, m = (n + 1) & ~1; const double gamma = hd[2];
  auto sync = [] {};
  int rc = 0; std::vector<double> out;
  if (mode == 0) {
    std::vector<double> G((size_t) D * n * n), A((size_t) n * n), Ginv(G.size());
    if (fread(G.data(), 8, G.size(), f) != G.size() || fread(A.data(), 8, A.size(), f) != A.size()) return 9;
    for (int d = 0; d < D && !rc; d++) {
      std::vector<double> a(G.begin() + (size_t) d * n * n, G.begin() + (size_t) (d + 1) * n * n), v(n * n), t(n), cs(m), sq(2); double ev[2];
      if (!stc_eig_run(a.data(), v.data(), t.data(), cs.data(), sq.data(), n, Ginv.data() + (size_t) d * n * n, ev, 0, 1, sync)) rc = 1;
      else if (!stc_posdef(ev[0], ev[1], n)) rc = 3;
    }
    std::vector<double> mem(StcWork::doubles(D, 1) + D); StcWork w; w.carve(mem.data(), D, 1);
    for (int e = 0; e < n * n; e++) w.A[e] = A[e];
    if (!rc && !stc_rows_run(w, D, kStcMaxItns, Ginv.data(), gamma, 0, 1, sync)) rc = 2;
    if (!rc) for (int e = 0; e < n * n; e++) A[e] = w.A[e];
    out = A;
  } else {
    std::vector<double> W((size_t) n * n), B((size_t) n * n), a(n * n), v(n * n), u(n * n), lam(2 * n), cs(m), sq(2), L(n * n), ev(2 * n); std::vector<int> ord(n);
    if (fread(W.data(), 8, W.size(), f) != W.size() || fread(B.data(), 8, B.size(), f) != B.size()) return 9;
    if (!lda_run(W.data(), B.data(), a.data(), v.data(), u.data(), lam.data(), cs.data(), sq.data(), ord.data(), n, L.data(), ev.data(), 0, 1, sync)) rc = 1;
    out = L; out.insert(out.end(), ev.begin(), ev.end());
  }
  fclose(f);
  f = fopen(argv[2], "wb"); double r = rc; fwrite(&r, 8, 1, f); fwrite(out.data(), 8, out.size(), f); fclose(f);
  return 0;
}
"""


def build_host(tmp, csrc):
    """the phases of csrc/stc_rows.h as a host program of one thread, plain g++ -> path of the executable"""
    src = os.path.join(str(tmp), "stc_host.cpp"); exe = os.path.join(str(tmp), "stc_host")
    with open(src, "w") as fh:
        fh.write(HOST_SRC)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", "-I", csrc, src, "-o", exe])
    return exe


def _run(exe, tmp, head, arrays):
    inp, outp = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    np.concatenate([np.asarray(head, np.float64)] + [np.asarray(a, np.float64).ravel() for a in arrays]).tofile(inp)
    subprocess.check_call([exe, inp, outp])
    return np.fromfile(outp)


def host_stc(exe, tmp, G, A0, gamma):
    """-> (rc, A): k_stc_eig's and k_stc_rows' code with one thread; rc 1 not finite, 2 refused by the rows, 3 not positive definite"""
    D = len(A0); r = _run(exe, tmp, [0, D, gamma], [G, A0])
    return int(r[0]), r[1:].reshape(D, D)


def host_lda(exe, tmp, W, B):
    """-> (rc, L, eigenvalues of W as found, eigenvalues of the whitened B descending): k_lda_solve's code with one thread"""
    D = len(W); r = _run(exe, tmp, [1, D, 0.0], [W, B])
    return int(r[0]), r[1:1 + D * D].reshape(D, D), r[1 + D * D:1 + D * D + D], r[1 + D * D + D:]
