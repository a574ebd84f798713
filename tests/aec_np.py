"""Numpy restatement of the subband echo cancellers of btk/cancelVP/cancelVP.{h,cc}: NLMSAcousticEchoCancellationFeature (cancelVP.cc:57-104),
KalmanFilterEchoCancellationFeature (:141-209), BlockKalmanFilterEchoCancellationFeature (:287-383) and
DTDBlockKalmanFilterEchoCancellationFeature (:1077-1198), in the reference's operation order, fp64, inputs rounded to complex64 first.

One object = one reference object: it keeps the filter coefficients, the covariances, the played history (_ComplexBuffer, cancelVP.h:145-212)
and, for DTD, the three smoothed scalars, from run() to run() exactly as the reference keeps them from utterance to utterance; reset() is the
reference's reset() (cancelVP.h:60, :98, :134-142).  Only bins 0..M/2 are computed (:68, :152, :299, :1134); full() adds the conjugate mirror
(:74-77).  Not restated: the printf dumps at bin 20 and the DTD constructor's debug file (:1065, :1102-1107)."""
import numpy as np

NLMS, KALMAN, BLOCK, DTD = 0, 1, 2, 3


def gsl_div(a, b):
    """gsl_complex_div (gsl complex/math.c): s = 1/|b|, (a s)(conj(b) s)"""
    s = 1.0 / np.hypot(b.real, b.imag)
    sbr, sbi = s * b.real, s * b.imag
    return complex((a.real * sbr + a.imag * sbi) * s, (a.imag * sbr - a.real * sbi) * s)


def abs2(z):
    return z.real * z.real + z.imag * z.imag


class Aec:
    def __init__(self, kind, fftLen, sampleN=1, delta=100.0, epsilon=1.0e-4, threshold=100.0, beta=0.95, sigma2=5.0, sigmau2=10e-4, sigmak2=5.0,
                 amp4play=1.0, snrTh=2.0, engTh=100.0, smooth=0.9):
        self.kind, self.M, self.F = kind, fftLen, fftLen // 2 + 1
        self.L = sampleN if kind in (BLOCK, DTD) else 1
        self.delta, self.epsilon, self.threshold, self.beta, self.amp = delta, epsilon, threshold, beta, amp4play
        self.snrTh, self.engTh, self.smooth = snrTh, engTh, smooth
        F, L = self.F, self.L
        self.R = np.zeros((F, L), np.complex128)                                    # NLMS: defined zero (the reference relies on __iter__'s reset())
        self.hist = np.zeros((F, L), np.complex128)                                 # hist[f][k] = the played sample k frames back, scaled
        if kind == KALMAN:                                                          # :117-121; sigma2_u = sigma2 (:115)
            self.sv = np.full(F, sigma2); self.K = np.full((F, 1, 1), sigma2, np.complex128); self.su = sigma2
        else:                                                                       # :233-246
            self.sv = np.full(F, sigmau2); self.K = np.tile(sigmak2 * np.eye(L, dtype=np.complex128), (F, 1, 1)); self.su = sigmau2
        self.dtd = np.zeros(3)                                                      # _EkEnergy, _SkEnergy, _snr (:1062)
        self.margin = np.inf; self.decisions = [0, 0]                               # DTD gate statistics outside the first-100-frames branch

    def reset(self):
        if self.kind in (NLMS, KALMAN):                                             # cancelVP.h:60, :98; the block variants reset nothing (:134-142)
            self.R[:] = 0

    def _update_band(self, Ak, Ek, frameX):                                         # :1077-1109
        if frameX < 100:
            smE = 1.0 - float(frameX) * (1.0 - self.smooth) / 100.0; smS = smE
        else:
            smE = smS = self.smooth
        Sk = Ak - Ek
        ce, cs = abs2(Ek), abs2(Sk)
        self.dtd[0] = ce * smE + self.dtd[0] * (1.0 - smE)
        self.dtd[1] = cs * smS + self.dtd[1] * (1.0 - smS)
        csnr = cs / (ce + 1.0e-15)
        self.dtd[2] = csnr * smE + self.dtd[2] * (1.0 - smE)
        snr, sk = self.dtd[2], self.dtd[1]
        if frameX >= 100:
            ok = snr > self.snrTh and sk > self.engTh
            m = abs(snr - self.snrTh) / self.snrTh                                  # the decision flips when the failing (or the nearer) test flips
            m2 = abs(sk - self.engTh) / self.engTh
            self.margin = min(self.margin, min(m, m2))
            self.decisions[1 if ok else 0] += 1
        if frameX < 100 or (snr > self.snrTh and sk > self.engTh):
            with np.errstate(over="ignore"):                                      # exp(-snr) = inf gives sf = -1, as in C
                return 2.0 / (1.0 + np.exp(-snr)) - 1.0
        return -1.0

    def _block_update(self, f, v, Ek, sf):                                          # :318-355, :1162-1193
        L = self.L
        self.sv[f] = self.beta * self.sv[f] + (1.0 - self.beta) * abs2(Ek)
        Km = (self.su * sf) * np.eye(L, dtype=np.complex128) + self.K[f]
        s = Km @ np.conj(v)
        sig = float(np.dot(v, s).real) + self.sv[f]
        G = (1.0 / sig) * s
        self.R[f] = self.R[f] + Ek * G
        self.K[f] = (np.eye(L, dtype=np.complex128) - np.outer(G, v)) @ Km

    def run(self, played, recorded, frame0=0, frame_mode=0):
        """played, recorded [T][F] -> E [T][F] complex128 (the device rounds it to complex64)"""
        V = np.asarray(played).astype(np.complex64).astype(np.complex128); A = np.asarray(recorded).astype(np.complex64).astype(np.complex128)
        T, F = V.shape[0], self.F
        out = np.zeros((T, F), np.complex128)
        for t in range(T):
            frameX = frame0 + t if frame_mode == 0 else -5
            if self.kind in (BLOCK, DTD):                                           # _buffer.nextSample(playBlock, _amp4play) (:297)
                self.hist[:, 1:] = self.hist[:, :-1].copy(); self.hist[:, 0] = V[t] * self.amp if self.amp != 1.0 else V[t]
            if self.kind == NLMS:
                for f in range(F):
                    Vk, Ak, Rk = complex(V[t, f]), complex(A[t, f]), complex(self.R[f, 0])
                    out[t, f] = Ak - Rk * Vk
                    if abs2(Vk) > self.threshold:
                        dC = Rk - gsl_div(Ak, Vk)
                        self.R[f, 0] = Rk - dC * (self.epsilon * abs2(Vk) / (self.delta + abs2(Ak)))
            elif self.kind == KALMAN:
                for f in range(F):
                    Vk, Ak, Rk = complex(V[t, f]), complex(A[t, f]), complex(self.R[f, 0])
                    Ek = Ak - Rk * Vk; out[t, f] = Ek
                    if abs2(Vk) > self.threshold:
                        sv = self.beta * self.sv[f] + (1.0 - self.beta) * abs2(Ek); self.sv[f] = sv
                        Vk2 = abs2(Vk); Kp = self.K[f, 0, 0].real + self.su
                        sig = Vk2 * Kp + sv
                        Gk = np.conj(Vk) * (Kp / sig)
                        self.R[f, 0] = Rk + Gk * Ek
                        self.K[f, 0, 0] = (1.0 - Kp * Vk2 / sig) * Kp
            elif self.kind == BLOCK:
                for f in range(F):
                    v = self.hist[f]; Ek = complex(A[t, f]) - np.dot(self.R[f], v); out[t, f] = Ek
                    if abs2(v[0]) > self.threshold:
                        self._block_update(f, v, Ek, 1.0)
            else:
                for f in range(F):                                                  # first loop (:1134-1146)
                    out[t, f] = complex(A[t, f]) - np.dot(self.R[f], self.hist[f])
                for f in range(F):                                                  # second loop (:1148-1194)
                    sf = self._update_band(complex(A[t, f]), complex(out[t, f]), frameX)
                    if sf < 0.0:
                        continue
                    self._block_update(f, self.hist[f], complex(out[t, f]), sf)
        return out

    def full(self, E):
        """[T][F] -> [T][M]: bin M-k = conj(bin k), 0 < k < M/2"""
        M = self.M
        return np.concatenate([E, np.conj(E[:, 1:M // 2][:, ::-1])], axis=1)


def erle_db(recorded, E, last=200):
    """echo-return-loss enhancement over the last frames: recorded power over residual power"""
    return 10.0 * np.log10(np.sum(np.abs(recorded[-last:]) ** 2) / np.sum(np.abs(E[-last:]) ** 2))


def echo_case(T, F, L, seed, near=1.0, amp=30.0, switch=None, quiet=()):
    """played [T][F] with `amp` per component, recorded = FIR(played, g) + near-end noise; g [F][L] random decaying taps (|g_k| ~ 0.3 e^{-k/4}).
    switch = (lo, hi, period): the near-end amplitude alternates every `period` frames.  quiet: (a, b) frame ranges where played is ~0."""
    rng = np.random.default_rng(seed)
    V = amp * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F)))
    for a, b in quiet:
        V[a:b] *= 1e-3
    V = V.astype(np.complex64).astype(np.complex128)
    g = 0.3 * np.exp(-np.arange(L) / 4.0) * (rng.standard_normal((F, L)) + 1j * rng.standard_normal((F, L))) / np.sqrt(2.0)
    echo = np.zeros((T, F), np.complex128)
    for k in range(min(L, T)):
        echo[k:] += g[:, k] * V[:T - k]
    n = np.full(T, near)
    if switch is not None:
        lo, hi, per = switch
        n = np.where((np.arange(T) // per) % 2 == 0, lo, hi).astype(float)
    N = n[:, None] * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F)))
    A = (echo + N).astype(np.complex64)
    return V.astype(np.complex64), A, g


def run_batch(make, V, A, nframes, frame0=0, frame_mode=0):
    """one fresh object per utterance (the batch entry's rule): V, A [U][T][F] -> E [U][T][F] (zero from nframes[u] on) and the objects"""
    U, T, F = V.shape
    E = np.zeros((U, T, F), np.complex128); objs = []
    for u in range(U):
        o = make(); n = int(nframes[u])
        E[u, :n] = o.run(V[u, :n], A[u, :n], frame0, frame_mode); objs.append(o)
    return E, objs


# The DTD cases of the GPU comparison: (fftLen, sampleN, frame mode, seed), U = 3 ragged, 260 frames, near-end noise switched between 0.5 and 12
# every 40 frames, SWIG defaults.  The seeds are chosen on the CPU (tests/test_aec_np_cpu.py) so that no gate decision lies within 1e-6 of its
# threshold and each side takes at least 10 % of the decisions: the device comparison then leaves no frame or bin out.
DTD_T = 260
DTD_CASES = [(64, 1, 0, 11), (64, 2, 0, 12), (64, 3, 0, 13), (64, 4, 0, 14), (64, 8, 0, 15), (64, 16, 0, 16), (64, 32, 0, 17), (64, 4, 1, 18),
             (256, 8, 0, 19), (512, 2, 0, 20)]


def dtd_inputs(M, L, seed, T=DTD_T, U=3):
    F = M // 2 + 1
    VA = [echo_case(T, F, L, seed * 100 + u, switch=(0.5, 12.0, 40))[:2] for u in range(U)]
    return np.stack([v for v, _ in VA]), np.stack([a for _, a in VA]), np.array([T, (2 * T) // 3, 1], np.int32)
