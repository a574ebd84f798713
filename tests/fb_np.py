"""Oversampled DFT filter bank in plain numpy: the closed forms of SURVEY.md Appendix A.1 / A.2 written from the reference's loops
(modulated.cc:412-452 analysis, :586-664 synthesis), the design sweep the GPU tests run, and the launchers' LDS arithmetic redone on the host.

Nothing here looks at a kernel: the closed forms pin the oracle (tests/test_oracle_cpu.py) at designs where it had never been compared with
anything, and their float32 evaluation is the yardstick for what rounding alone costs at a design (tests/test_gpu_filterbank_designs.py)."""
import numpy as np

# (M, m, r) by the analysis kernel the dispatch (fb_analysis, csrc/k_filterbank.hip) selects for it.  A change of the dispatch is answered
# by a change of these lists; no test asserts a kernel name.
Q256 = [(256, 2, 1)]
WAVE = [(128, 2, 0), (128, 4, 2), (128, 2, 7), (256, 2, 3), (256, 4, 2), (512, 4, 1), (1024, 2, 2), (1024, 4, 3), (1024, 2, 0), (1024, 4, 0)]
GENERIC = [(16, 2, 1), (16, 2, 4), (32, 4, 0), (64, 3, 2), (128, 1, 1), (256, 3, 1), (512, 1, 0), (1024, 3, 1), (2048, 2, 2), (2048, 1, 4),
           (2048, 4, 0)]
SHIPPED = {(256, 4, 1): "M256-m4-r1", (512, 2, 2): "M512-m2-r2", (512, 2, 3): "M512-m2-r3"}      # prototypes under tests/golden/
DESIGNS = Q256 + WAVE + GENERIC
# synthesis designs whose R*m - 1 frames of history do not fit the LDS of k_synthesis at their M (refused with DSR_E_DIMENSION)
SYNTHESIS_REFUSED = {(128, 2, 7), (1024, 4, 3), (2048, 1, 4)}
LDS_MAX = 160 * 1024


def delays(m, r, dct, synthesis):
    """(processingDelay, look-ahead) of modulated.cc:279-296"""
    R = 1 << r
    if dct == 1:
        return m * R - 1, 0
    if dct == 2:
        return (m * R // 2, 0) if synthesis else (m * R - 1, m * R // 2 - 1)
    return 2 * m - 1, 0


def dct_defined(m, r, dct):
    """delayCompensationType 2 with m * R < 2 makes the reference's look-ahead m*R/2 - 1 negative (an unsigned wrap there): no defined result"""
    return not (dct == 2 and m * (1 << r) < 2)


def analysis_closed_form(x, h, M, m, r, dct=0, gain=1, dtype=np.float64):
    """X_t[f] = gain * sum_k u_t[k] e^{+2 pi j f k / M},  u_t[k] = sum_q h[k + qM] x[n_t - k - qM],  n_t = (t + laN + 1) D - 1; samples before the
    start and after the end are zero; T = ceil(n / D) - laN + processingDelay frames (none when the input is shorter than the look-ahead).
    dtype float32: polyphase sums in float32 and the DFT on complex64 data -- what fp32 arithmetic alone costs.  -> [T][M]"""
    D = M >> r
    pd, la = delays(m, r, dct, False)
    nblk = (len(x) + D - 1) // D
    T = 0 if nblk < la else nblk - la + pd
    ctype = np.complex128 if dtype == np.float64 else np.complex64
    if T == 0:
        return np.zeros((0, M), ctype)
    xp = np.concatenate([np.zeros(m * M), np.asarray(x, np.float64), np.zeros((T + la + 1) * D)]).astype(dtype)
    hh = np.asarray(h, np.float64).astype(dtype)
    nt = (np.arange(T) + la + 1) * D - 1 + m * M
    u = np.zeros((T, M), dtype)
    k = np.arange(M)
    for q in range(m):
        u += hh[k + q * M][None, :] * xp[nt[:, None] - k[None, :] - q * M]
    X = np.fft.ifft(u, axis=1) * M if dtype == np.float64 else _fft_pow2(u.astype(ctype), +1)
    return X * dtype(gain) if gain > 0 else X


def synthesis_closed_form(Y, g, M, m, r, dct=0, gain=1):
    """v_tau[k] = Re sum_f Y_tau[f] e^{-2 pi j f k / M};  s_t[k] = sum_{q<m} g[(M-1-k) + qM] v_{t+pd-Rq}[k];
    y_t[D-1-d] = gain * sum_{i<R} s_{t-R+1+i}[d + iD]; terms with a negative frame index dropped; t = 0 .. T - pd - 1.   Y [T][M] -> float64 [(T-pd) D]"""
    Y = np.asarray(Y, np.complex128); g = np.asarray(g, np.float64)
    T = Y.shape[0]; R = 1 << r; D = M >> r
    pd, _ = delays(m, r, dct, True)
    nout = max(T - pd, 0)
    if nout == 0:
        return np.zeros(0)
    v = np.fft.fft(Y, axis=1).real
    k = np.arange(M)
    s = np.zeros((nout, M))
    for q in range(m):
        tau = np.arange(nout) + pd - R * q
        ok = tau >= 0
        s[ok] += g[(M - 1 - k) + q * M][None, :] * v[tau[ok]]
    y = np.zeros((nout, D))
    d = np.arange(D)
    for i in range(R):
        ts = np.arange(nout) - R + 1 + i
        ok = ts >= 0
        y[np.ix_(ok, D - 1 - d)] += s[ts[ok]][:, d + i * D]
    if gain > 0:
        y *= gain
    return y.reshape(-1)


def _fft_pow2(a, sign):
    """radix-2 decimation-in-time DFT along the last axis in the dtype of `a` (numpy's own FFT would do complex64 data in double)"""
    n = a.shape[-1]
    bits = n.bit_length() - 1
    rev = np.array([int(format(i, "0%db" % bits)[::-1], 2) for i in range(n)])
    a = a[..., rev].copy()
    half = 1
    while half < n:
        w = np.exp(sign * 2j * np.pi * np.arange(half) / (2 * half)).astype(a.dtype)
        a = a.reshape(a.shape[:-1] + (n // (2 * half), 2, half))
        lo, hi = a[..., 0, :], a[..., 1, :] * w
        a = np.stack([lo + hi, lo - hi], axis=-2).reshape(a.shape[:-3] + (n,))
        half *= 2
    return a


# ------------------------------------------------------------------------------------- launchers' LDS requests, redone on the host
def analysis_generic_lds(M, m, r):
    """launch_analysis<M>: [tw M float2][proto m*M][window (TF-1) D + m*M, rounded up to 4][two FFT buffers of FB frames]"""
    D = M >> r
    FB = max(4096 // M, 1)
    TF = max(min(2 * FB, 64), FB)
    win = (TF - 1) * D + m * M
    return 8 * M + 4 * (m * M + ((win + 3) & ~3) + 2 * FB * M)


def analysis_wave_lds(M, m, r, TF=32, waves=4):
    """launch_analysis_w<M, m>: [tw][window (TF-1) D + m*M][one skewed strip of M/2 + M/16 float2 per wave]"""
    D = M >> r
    win = (TF - 1) * D + m * M
    return 8 * M + 4 * ((win + 3) & ~3) + 8 * waves * (M // 2 + M // 16)


def synthesis_lds(M, m, r):
    """launch_synthesis<M>: TO output blocks per workgroup, halved while TO + R*m - 1 time-domain frames exceed 48 KB; -> (bytes, TO)"""
    R = 1 << r
    FB = max(4096 // M, 1)
    TO = 32
    while TO > 1 and (TO + R * m - 1) * M * 4 > 48 * 1024:
        TO >>= 1
    NV = TO + R * m - 1
    return 8 * M + 4 * (m * M + NV * M + 2 * FB * M), TO
