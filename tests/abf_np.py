"""A literal fp64 restatement of the classes of btk/lib/subbandBeamforming.py that dsr_abf_* replaces (include/dsr.h section 2a''): the set-up
helpers, SubbandBeamformerDS / GSC, SubbandBeamformerGriffithsJim, SubbandBeamformerMVDR (sample matrix inversion) and SubbandBeamformerMPDR, as
shipped, NC = 1 (the static GSC: also 2), no halfBandShift.  It keeps numpy.linalg.inv where the reference calls inverse().

Every sum is an explicit left-to-right loop over the summation index (_lr), so an order of operations exists to be matched; the bins of a frame
and the entries that are not summed over are carried as numpy axes (the reference loops over them, the results are the same numbers).

Each adaptive class has a second evaluation that differs only in rounding (alt=True): numpy's own summation order for the inverse-free
Griffiths-Jim, a numpy.longdouble Cholesky solve in place of inv for the two sample-matrix classes.  form="rl" evaluates MPDR the way the device
does -- R = B^H Sx B and conj(L) = conj(wq^H Sx B) averaged directly, fp64 Cholesky -- which is the same mathematics.

A run works on one utterance X [C][T][F] (bins 0..fftLen/2) and returns a dict: Y [T][F], w (the final weights [F][C-1] or [F][C]), and for
Griffiths-Jim the counts of every decision (gate, norm constraint, floor: taken, idle) with the smallest relative distance of a compared value
from its threshold; for the sample-matrix classes the smallest eigenvalue and the Hermitian defect of every matrix that was inverted."""
import numpy as np

SSPEED = 343740.0


def _lr(n, term):
    """term(0) + term(1) + ... + term(n - 1), added left to right"""
    acc = term(0)
    for k in range(1, n):
        acc = acc + term(k)
    return acc


# ---- the set-up helpers ------------------------------------------------------------------------------------------------------------------
def calcDelays(x, y, z, mpos):
    """:227-246"""
    chanN = len(mpos)
    delays = np.array([np.sqrt((x - mpos[i, 0]) ** 2 + (y - mpos[i, 1]) ** 2 + (z - mpos[i, 2]) ** 2) / SSPEED for i in range(chanN)], np.float64)
    mid = delays[chanN // 2]
    return delays - mid


def calcBlockingMatrix(vs, NC=1):
    """:249-277"""
    vs = np.asarray(vs, np.complex128); vsize = len(vs); bsize = vsize - NC
    blockMat = np.zeros((vsize, bsize), np.complex128)
    norm_vs = _lr(vsize, lambda i: vs[i] * np.conj(vs[i]))
    if norm_vs.real > 0.0:
        PcPerp = np.eye(vsize) - np.outer(np.conj(vs), vs) / norm_vs
        for idim in range(bsize):
            vec = PcPerp[:, idim].copy()
            for jdim in range(idim):
                rvec = blockMat[:, jdim]
                ip = _lr(vsize, lambda i: np.conj(rvec[i]) * vec[i])
                vec = vec - rvec * ip
            norm_vec = np.sqrt(abs(_lr(vsize, lambda i: np.conj(vec[i]) * vec[i])))
            blockMat[:, idim] = vec / norm_vec
    return blockMat


def calcArrayManifold_f(fbinX, fftLen, chanN, sampleRate, delays, halfBandShift=False, norm=True):
    """:438-463 (norm) and calcArrayManifoldWoNorm_f :465-493 (norm=False)"""
    assert not halfBandShift
    Delta_f = sampleRate / float(fftLen); J = 1j
    vs = np.zeros(chanN, np.complex128)
    for chanX in range(chanN):
        if fbinX <= fftLen // 2:
            vs[chanX] = np.exp(-J * 2.0 * np.pi * fbinX * Delta_f * delays[chanX])
        else:
            vs[chanX] = np.exp(J * 2.0 * np.pi * (fftLen - fbinX) * Delta_f * delays[chanX])
        if norm:
            vs[chanX] = vs[chanX] / chanN
    return vs


def getInverseMat22(mat):
    """:495-514"""
    det = mat[0][0] * mat[1][1] - mat[0][1] * mat[1][0]
    if abs(det) < 1.0e-07:
        mat = mat + 0.01 * np.eye(2)
        det = mat[0][0] * mat[1][1] - mat[0][1] * mat[1][0]
    inv = np.zeros((2, 2), np.complex128)
    inv[0][0] = mat[1][1] / det; inv[0][1] = -mat[0][1] / det; inv[1][0] = -mat[1][0] / det; inv[1][1] = mat[0][0] / det
    return inv


def calcNullBeamformer(w_t, w_j, NC=2):
    """:517-546"""
    assert NC == 2
    nChan = len(w_t)
    Cm = np.zeros((nChan, 2), np.complex128); Cm[:, 0] = w_t; Cm[:, 1] = w_j
    CH = Cm.conj().T
    CHC = np.array([[_lr(nChan, lambda k: CH[a, k] * Cm[k, b]) for b in range(2)] for a in range(2)])
    inv = getInverseMat22(CHC)
    V = np.array([inv[0][0] * 1.0 + inv[0][1] * 0.0, inv[1][0] * 1.0 + inv[1][1] * 0.0])
    return Cm[:, 0] * V[0] + Cm[:, 1] * V[1]


def design(fftLen, chanN, sampleRate, delays, NC=1):
    """calcArrayManifoldVectors of SubbandBeamformerGSC (:603-618) for bins 0..fftLen/2 -> (wq [F][C], B [F][C][C-NC])"""
    F = fftLen // 2 + 1
    wq = np.array([calcArrayManifold_f(f, fftLen, chanN, sampleRate, delays) for f in range(F)])
    B = np.array([calcBlockingMatrix(wq[f], NC) for f in range(F)])
    return wq, B


# ---- the fixed-weight classes ------------------------------------------------------------------------------------------------------------
def _wp(wp, isamp, val):
    return wp[isamp] * val if wp is not None and isamp < len(wp) else val


def static_ds(X, wq, wp=None):
    """SubbandBeamformerDS.__iter__ (:371-384): conj(v) . x"""
    Cn, T, F = X.shape
    return np.array([_wp(wp, t, _lr(Cn, lambda c: np.conj(wq[:, c]) * X[c, t].astype(np.complex128))) for t in range(T)]).reshape(T, F)


def static_gsc(X, wq, B, wa, wp=None):
    """SubbandBeamformerGSC.__iter__ (:573-601): conj(x^H wq - (x^H B) wa)"""
    Cn, T, F = X.shape; nb = B.shape[2]
    Y = np.zeros((T, F), np.complex128)
    for t in range(T):
        XKH = np.conj(X[:, t].astype(np.complex128))
        ZK = _lr(Cn, lambda c: XKH[c][:, None] * B[:, c, :])
        YcK = _lr(Cn, lambda c: XKH[c] * wq[:, c])
        Y[t] = _wp(wp, t, np.conj(YcK - _lr(nb, lambda j: ZK[:, j] * wa[:, j])))
    return Y


# ---- Griffiths-Jim -----------------------------------------------------------------------------------------------------------------------
def _margin(best, value, thr):
    m = np.min(np.abs(np.asarray(value, np.float64) - thr) / np.abs(thr)) if np.size(value) else np.inf
    return min(best, float(m))


def griffiths_jim(X, wq, B, fftLen, beta=0.999, gamma=0.0005, initDiagLoad=1.0e10, floorSubBandSigmaK=2.0e7, silThresh=1.0e10, alpha2=0.001,
                  staticAfter=1000, wp=None, alt=False):
    """nextSpkr() (:1092-1104) and __iter__ (:1013-1090) over the T frames of X [C][T][F]"""
    Cn, T, F = X.shape; n = Cn - 1
    g = gamma; avg = initDiagLoad; wa = np.zeros((F, n), np.complex128); sbs = np.full(F, initDiagLoad, np.float64)
    Y = np.zeros((T, F), np.complex128)
    cnt = dict(gate=[0, 0], norm=[0, 0], floor=[0, 0]); mar = dict(gate=np.inf, norm=np.inf, floor=np.inf)
    for isamp in range(T):
        x = X[:, isamp].astype(np.complex128)                                   # [C][F]
        x0 = np.concatenate([x[0], np.conj(x[0][1:F - 1][::-1])])                # the full spectrum of channel 0
        dot0 = np.dot(np.conj(x0), x0) if alt else _lr(fftLen, lambda i: np.conj(x0[i]) * x0[i])
        sigmaK = abs(dot0) / fftLen
        if isamp == staticAfter:
            g /= 10.0
        gate = sigmaK > (avg / silThresh)
        cnt["gate"][0 if gate else 1] += 1; mar["gate"] = _margin(mar["gate"], sigmaK, avg / silThresh)
        if alt:
            ZK = np.einsum("fcj,cf->fj", np.conj(B), x); YcK = np.einsum("fc,cf->f", np.conj(wq), x)
        else:
            ZK = _lr(Cn, lambda c: np.conj(B[:, c, :]) * x[c][:, None]); YcK = _lr(Cn, lambda c: np.conj(wq[:, c]) * x[c])
        if gate:
            if alt:
                epa = YcK - (wa * ZK).sum(1); pw = np.abs((np.conj(x) * x).sum(0))
            else:
                epa = YcK - _lr(n, lambda j: wa[:, j] * ZK[:, j]); pw = np.abs(_lr(Cn, lambda c: np.conj(x[c]) * x[c]))
            sb = sbs * beta + (1.0 - beta) * pw if isamp > 0 else pw
            low = sb < floorSubBandSigmaK
            cnt["floor"][0] += int(low.sum()); cnt["floor"][1] += int((~low).sum()); mar["floor"] = _margin(mar["floor"], sb, floorSubBandSigmaK)
            sb = np.where(low, floorSubBandSigmaK, sb)
            alphaK = g / sb
            wat = wa + epa[:, None] * np.conj(ZK) * alphaK[:, None]
            nrm = np.abs((wat * np.conj(wat)).sum(1)) if alt else np.abs(_lr(n, lambda j: wat[:, j] * np.conj(wat[:, j])))
            over = nrm > alpha2
            cnt["norm"][0] += int(over.sum()); cnt["norm"][1] += int((~over).sum()); mar["norm"] = _margin(mar["norm"], nrm, alpha2)
            cK = np.sqrt(alpha2 / np.where(over, nrm, 1.0))
            wa = np.where(over[:, None], cK[:, None] * wat, wat); sbs = sb
        val = YcK - ((wa * ZK).sum(1) if alt else _lr(n, lambda j: wa[:, j] * ZK[:, j]))
        Y[isamp] = _wp(wp, isamp, val)
        avg = avg * beta + (1.0 - beta) * sigmaK
    return dict(Y=Y, w=wa, counts=cnt, margins=mar)


# ---- sample matrix inversion -------------------------------------------------------------------------------------------------------------
def _chol_solve(A, r, dtype):
    """A [F][m][m] Hermitian positive definite, r [F][m]: A^-1 r by a Cholesky factorisation and two triangular solves in `dtype`"""
    ct = np.clongdouble if dtype is np.longdouble else np.complex128
    A = A.astype(ct); r = r.astype(ct); Fn, m, _ = A.shape
    L = np.zeros_like(A)
    for j in range(m):                                                          # column by column; the sums over q < j as one numpy reduction
        d = np.sqrt(A[:, j, j].real - (L[:, j, :j] * np.conj(L[:, j, :j])).real.sum(-1)); L[:, j, j] = d
        L[:, j + 1:, j] = (A[:, j + 1:, j] - (L[:, j + 1:, :j] * np.conj(L[:, j, None, :j])).sum(-1)) / d[:, None]
    s = np.zeros_like(r)
    for i in range(m):
        s[:, i] = (r[:, i] - (L[:, i, :i] * s[:, :i]).sum(-1)) / L[:, i, i]
    for i in range(m - 1, -1, -1):
        s[:, i] = (s[:, i] - (np.conj(L[:, i + 1:, i]) * s[:, i + 1:]).sum(-1)) / L[:, i, i]
    return s


def _pd(stat, A):
    ev = np.linalg.eigvalsh(A)
    stat["min_eig"] = min(stat["min_eig"], float(ev.min())); stat["cond"] = max(stat["cond"], float((ev.max(-1) / ev.min(-1)).max()))
    stat["herm"] = max(stat["herm"], float(np.abs(A - np.conj(np.swapaxes(A, 1, 2))).max() / np.abs(A).max()))


def smi_mvdr(X, v, diagLoad=0.001, forgetFactor=0.99, end=20, wp1L=None, alt=False):
    """SubbandBeamformerMVDR.__iter__ with updateSx (:1131-1175), bins 0..fftLen/2; v [F][C] the array manifold.  w: conj(_wH) [F][C]"""
    Cn, T, F = X.shape
    Sx = np.zeros((F, Cn, Cn), np.complex128); wH = np.zeros((F, Cn), np.complex128); eye = diagLoad * np.identity(Cn)
    Y = np.zeros((T, F), np.complex128); stat = dict(min_eig=np.inf, herm=0.0, cond=0.0)
    for frame in range(T):
        x = X[:, frame].astype(np.complex128).T                                 # [F][C]
        if frame <= end:
            newSx = x[:, :, None] * np.conj(x[:, None, :])
            Sx = newSx if frame == 0 else forgetFactor * Sx + (1.0 - forgetFactor) * newSx
            A = Sx + eye; _pd(stat, A)
            if alt:
                temp = _chol_solve(A, v, np.longdouble).astype(np.complex128)
            else:
                Ainv = np.linalg.inv(A); temp = _lr(Cn, lambda k: Ainv[:, :, k] * v[:, k][:, None])
            wo = temp / _lr(Cn, lambda k: np.conj(v[:, k]) * temp[:, k])[:, None]
            wH = np.conj(wo)
        val = _lr(Cn, lambda c: wH[:, c] * x[:, c])
        if wp1L is not None and len(wp1L) > 0:
            val = wp1L[frame] * val
        Y[frame] = val
    return dict(Y=Y, w=np.conj(wH), stat=stat)


def smi_mpdr(X, wq, B, diagLoad=0.001, forgetFactor=0.99, end=20, alt=False, form="sx"):
    """SubbandBeamformerMPDR.__iter__ with updateActiveWeight and updateSx (:1206-1265), bins 0..fftLen/2.  w: _waK [F][C-1]"""
    Cn, T, F = X.shape; n = Cn - 1
    Sx = np.zeros((F, Cn, Cn), np.complex128); waK = np.zeros((F, n), np.complex128); eye = diagLoad * np.identity(n)
    R = np.zeros((F, n, n), np.complex128); h = np.zeros((F, n), np.complex128)
    Y = np.zeros((T, F), np.complex128); stat = dict(min_eig=np.inf, herm=0.0, cond=0.0)
    BH = np.conj(np.swapaxes(B, 1, 2))                                          # [F][n][C]
    for frame in range(T):
        x = X[:, frame].astype(np.complex128).T
        XHK = np.conj(x)
        ZHK = _lr(Cn, lambda c: XHK[:, c][:, None] * B[:, c, :])
        YcK = _lr(Cn, lambda c: XHK[:, c] * wq[:, c])
        if form == "rl":                                                         # the device's formulation: R and conj(L) averaged directly
            if frame <= end:
                z = np.conj(ZHK); yc = np.conj(YcK)
                nR = z[:, :, None] * np.conj(z[:, None, :]); nh = z * np.conj(yc)[:, None]
                R = nR if frame == 0 else forgetFactor * R + (1.0 - forgetFactor) * nR
                h = nh if frame == 0 else forgetFactor * h + (1.0 - forgetFactor) * nh
                waK = _chol_solve(R + eye, h, np.float64)
        else:
            if frame == 0:
                Sx = x[:, :, None] * np.conj(x[:, None, :])
            elif frame <= end:
                Sx = forgetFactor * Sx + (1.0 - forgetFactor) * (x[:, :, None] * np.conj(x[:, None, :]))
            if alt:                                                              # numpy's own order for the three products
                temp = Sx @ B; L = (np.conj(wq)[:, None, :] @ temp)[:, 0, :]; Rm = BH @ temp
            else:
                temp = _lr(Cn, lambda k: Sx[:, :, k][:, :, None] * B[:, k, :][:, None, :])      # Sx B
                L = _lr(Cn, lambda k: np.conj(wq[:, k])[:, None] * temp[:, k, :])
                Rm = _lr(Cn, lambda k: BH[:, :, k][:, :, None] * temp[:, k, :][:, None, :])
            A = Rm + eye
            if frame <= end:
                _pd(stat, A)
            if alt:
                waK = _chol_solve(A, np.conj(L), np.longdouble).astype(np.complex128)
            else:
                Rinv = np.linalg.inv(A); waK = np.conj(_lr(n, lambda k: L[:, k][:, None] * Rinv[:, k, :]))
        Y[frame] = np.conj(YcK - _lr(n, lambda j: ZHK[:, j] * waK[:, j]))
    return dict(Y=Y, w=waK, stat=stat)


def mvdr_device_order(X, v, diagLoad=0.001, forgetFactor=0.99, end=20):
    """MVDR the way the device evaluates it: fp64 Cholesky in place of inv"""
    Cn, T, F = X.shape
    Sx = np.zeros((F, Cn, Cn), np.complex128); w = np.zeros((F, Cn), np.complex128); eye = diagLoad * np.identity(Cn)
    Y = np.zeros((T, F), np.complex128)
    for frame in range(T):
        x = X[:, frame].astype(np.complex128).T
        if frame <= end:
            newSx = x[:, :, None] * np.conj(x[:, None, :])
            Sx = newSx if frame == 0 else forgetFactor * Sx + (1.0 - forgetFactor) * newSx
            s = _chol_solve(Sx + eye, v, np.float64)
            w = s / (np.conj(v) * s).sum(1)[:, None]
        Y[frame] = (np.conj(w) * x).sum(1)
    return dict(Y=Y, w=w)
