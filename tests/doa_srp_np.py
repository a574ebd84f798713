"""Numpy fp64 restatement of DOAEstimatorSRPDSBLA (btk/beamformer/beamformer.h:462-560, beamformer.cc:2920-3283) over whole utterances:
the theta grid and the steering table (_calcSteeringUnitTable :3105-3152, setLookDirection :3257-3271, calcMainlobe :531-594), the
frame energy with its float accumulator emulated step by step (calcEnergy :3043-3074), the response powers (_calcResponsePower
:3154-3186), the energy gate, the per-frame N-best and the accumulators (next :3188-3245), and the final N-best
(_getNBestHypothesesFromACCRP :2986-3025).  The GPU tests check the device against it."""
import numpy as np


def theta_grid(minTheta, maxTheta, widthTheta):
    """:3113 _nTheta = (unsigned)((max - min) / width + 0.5); the loops accumulate theta += width from min (:3133, :3223)"""
    n = int((maxTheta - minTheta) / widthTheta + 0.5)
    th, out = float(minTheta), []
    for _ in range(n):
        out.append(th); th += widthTheta
    return np.array(out, np.float64)


def look_delays(positions, C, theta):
    """setLookDirection (:3257-3271): d_0 = 0, d_c = |x_c - x_0| cos(theta); only x, no speed of sound"""
    x = np.asarray(positions, np.float64)
    d = np.zeros(C)
    for c in range(1, C):
        d[c] = abs(x[c] - x[0]) * np.cos(theta)
    return d


def wq(delays, fs, M, f):
    """calcMainlobe (:557-581), halfBandShift == false: the delay-and-sum weights of bin f, / C"""
    C = len(delays)
    if f == 0:
        return np.full(C, 1.0 / C, np.complex128)
    val = (-2.0 * np.pi * f * delays * fs / M) if f < M // 2 else (-np.pi * fs * delays)
    return (np.cos(val) + 1j * np.sin(val)) / C


def steering_table(positions, C, fs, M, thetas, fbinMin, fbinMax):
    """[fbinMax+1][nTheta][C]: bin 0 = (1, 0) (:3136-3137), then wq_f for fbinMin..fbinMax (:3138-3141; overwrites bin 0 when fbinMin = 0)"""
    W = np.zeros((fbinMax + 1, len(thetas), C), np.complex128)
    for k, th in enumerate(thetas):
        d = look_delays(positions, C, th)
        W[0, k] = 1.0
        for f in range(fbinMin, fbinMax + 1):
            W[f, k] = wq(d, float(fs), M, f)
    return W


def energy(X, fbinMin, fbinMax, M):
    """calcEnergy (:3043-3074) for X [C][T][>= fbinMax+1] complex64: a float accumulator rp += g_f |zdotc(X_f, X_f)|^2 (the double term added to
    the float promoted to double, the sum rounded back to float), divided by 2 (M/2) C in float.  Vectorised over frames only."""
    C, T = X.shape[0], X.shape[1]
    Xr = X.real.astype(np.float64); Xi = X.imag.astype(np.float64)
    rp = np.zeros(T, np.float32)
    for f in range(fbinMin, fbinMax + 1):
        s = np.zeros(T)
        for c in range(C):                                  # gslcblas zdotc: r_real += x_re y_re - (-1) x_im y_im, channel by channel
            s = s + (Xr[c, :, f] * Xr[c, :, f] + Xi[c, :, f] * Xi[c, :, f])
        g = 2.0 if f < M // 2 else 1.0
        rp = (rp.astype(np.float64) + g * (s * s)).astype(np.float32)
    return rp / np.float32(2 * (M // 2) * C)


def response_power(X, W, fbinMin, fbinMax, M):
    """_calcResponsePower (:3154-3186) -> (rp [T][nTheta], val [T][nTheta][fbinMax+1]: w^H X per bin, the unit's beamformed values)"""
    T, nT = X.shape[1], W.shape[1]
    rp = np.zeros((T, nT))
    val = np.zeros((T, nT, fbinMax + 1), np.complex128)
    Xd = X.astype(np.complex128)
    for f in range(fbinMin, fbinMax + 1):
        v = np.einsum("kc,ct->tk", np.conj(W[f]), Xd[:, :, f])
        val[:, :, f] = v
        rp += (2.0 if f < M // 2 else 1.0) * (v.real ** 2 + v.imag ** 2)
    return rp / (fbinMax - fbinMin + 1), val


def nbest(rps, nBest):
    """the insertion of :3226-3244 / :3004-3021: strict > (on a tie the earlier direction stays ahead); index -1 = empty rank (-10e10)"""
    R = np.full(nBest, -10e10); I = np.full(nBest, -1, np.int64)
    for k, v in enumerate(rps):
        if v > R[nBest - 1]:
            for n1 in range(nBest):
                if v > R[n1]:
                    R[n1 + 1:] = R[n1:-1].copy(); I[n1 + 1:] = I[n1:-1].copy()
                    R[n1] = v; I[n1] = k
                    break
    return R, I


def run(X, nframes, positions, fs, M, nBest, thetas, fbinMin, fbinMax, threshold, acc=None):
    """X [U][C][T][M/2+1] complex64 -> dict(energy [U][T] f32, rp [U][T][nT], gated [U][T], nbest_rp / nbest_idx [U][T][nBest], acc [U][nT],
    y [U][T][M/2+1]: the last unit's beamformed bins fbinMin..fbinMax).  Frames from nframes[u] on stay zero."""
    U, C, T, F = X.shape
    nT = len(thetas)
    W = steering_table(positions, C, fs, M, thetas, fbinMin, fbinMax)
    out = dict(energy=np.zeros((U, T), np.float32), rp=np.zeros((U, T, nT)), gated=np.zeros((U, T), np.int32),
               nbest_rp=np.zeros((U, T, nBest)), nbest_idx=np.zeros((U, T, nBest), np.int64),
               acc=np.zeros((U, nT)) if acc is None else np.array(acc, np.float64), y=np.zeros((U, T, F), np.complex128))
    for u in range(U):
        N = min(int(nframes[u]), T)
        if N == 0:
            continue
        Xu = X[u, :, :N]
        e = energy(Xu, fbinMin, fbinMax, M)
        rp, val = response_power(Xu, W, fbinMin, fbinMax, M)
        out["energy"][u, :N] = e; out["rp"][u, :N] = rp
        out["y"][u, :N, fbinMin:fbinMax + 1] = val[:, nT - 1, fbinMin:fbinMax + 1]
        for t in range(N):
            R, I = np.full(nBest, -10e10), np.full(nBest, -1)
            if e[t] < np.float32(threshold):
                out["gated"][u, t] = 1
            else:
                R, I = nbest(rp[t], nBest)
                out["acc"][u] += rp[t]                    # :3201, frame by frame
            out["nbest_rp"][u, t] = R; out["nbest_idx"][u, t] = I
    return out
