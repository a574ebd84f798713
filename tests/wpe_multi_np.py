"""Numpy restatement of MultiChannelWPEDereverberation (btk/dereverberation/dereverberation.cc:397-620) for one (subband, channel):
stacked lags [channel][lag] (_getLags), theta_n from the channel's own filter (_calculateThetan), the weighted correlation matrix and
vector (_calculateRr), diagonal loading (_loadR), Cholesky solve (_estimateGn), iterated; optionally seeded with the filters a previous
block left (reset() keeps _Gn).  The checks of the device's tiled path at sizes and in modes the CPU oracle cannot reach use it."""
import numpy as np


def lags(Yb, lowerN, P):
    """Yb [C][N] complex (one subband, all channels) -> X [N][C P]: X[n][c P + l] = Yb[c][n - lowerN - l], zero before frame 0."""
    Cn, N = Yb.shape
    X = np.zeros((N, Cn * P), np.complex128)
    for c in range(Cn):
        for l in range(P):
            s = lowerN + l
            if s < N:
                X[s:, c * P + l] = Yb[c, :N - s]
    return X


def selected(b, fftLen, bandWidth, sampleRate=16000.0):
    lowerBW = fftLen // 2 if bandWidth == 0.0 else int((bandWidth / (sampleRate / 2.0)) * (fftLen // 2))
    return b <= lowerBW or b >= fftLen - lowerBW


def predict(Yb, c, g, lowerN, P, X=None):
    """y_c[n] - g^H x_n for n >= lowerN, y_c[n] before."""
    X = lags(Yb, lowerN, P) if X is None else X
    d = X @ np.conj(g)
    out = Yb[c].astype(np.complex128).copy()
    out[lowerN:] -= d[lowerN:]
    return out


def filters(Yb, c, lowerN, upperN, iterationsN=2, loadDb=-20.0, g0=None):
    """The prediction filter [C P] of channel c for one subband after iterationsN iterations from g0 (zero by default); NaN where the
    loaded matrix is not positive definite."""
    Yb = np.asarray(Yb, np.complex128)
    Cn, N = Yb.shape
    P = upperN - lowerN + 1
    X = lags(Yb, lowerN, P)
    g = np.zeros(Cn * P, np.complex128) if g0 is None else np.asarray(g0, np.complex128).copy()
    for _ in range(iterationsN):
        e = predict(Yb, c, g, lowerN, P, X)
        th = np.maximum(np.abs(e), 1e-3) ** 2
        w = 1.0 / th
        R = X.T @ (w[:, None] * np.conj(X))                                  # sum_n x_n x_n^H / theta_n
        r = X.T @ (w * np.conj(Yb[c]))                                       # sum_n conj(y_c[n]) x_n / theta_n
        d = np.abs(np.diag(R))
        R[np.diag_indices(Cn * P)] = d + d.max() * 10 ** (loadDb / 10)
        try:
            L = np.linalg.cholesky(R)
        except np.linalg.LinAlgError:
            return np.full(Cn * P, np.nan + 1j * np.nan)
        g = np.linalg.solve(np.conj(L.T), np.linalg.solve(L, r))
    return g


def wpe_multi(Y, fftLen, lowerN, upperN, iterationsN=2, loadDb=-20.0, bandWidth=0.0, sampleRate=16000.0, filterChan=-1, gn0=None, pairs=None):
    """Y [C][N][F] (F = fftLen / 2 + 1) -> (out [C][N][F], gn [C][F][C P]) like the device call for one utterance; gn0: seed filters.
    pairs: only these (subband, channel) filters are computed (the others stay zero, and only their outputs are meaningful)."""
    Y = np.asarray(Y, np.complex128)
    Cn, N, F = Y.shape
    P = upperN - lowerN + 1
    gn = np.zeros((Cn, F, Cn * P), np.complex128)
    out = Y.copy()
    todo = pairs if pairs is not None else [(b, c) for b in range(F) for c in range(Cn)]
    for b, c in todo:
        if selected(b, fftLen, bandWidth, sampleRate):
            gn[c, b] = filters(Y[:, :, b], c, lowerN, upperN, iterationsN, loadDb, None if gn0 is None else gn0[c, b])
    for b, c in todo:
        if selected(b, fftLen, bandWidth, sampleRate):
            fc = filterChan if filterChan >= 0 else c
            out[c, :, b] = predict(Y[:, :, b], c, gn[fc, b], lowerN, P)
    return out, gn
