"""Restatement of WarpedTwiceMVDRFeature (btk/feature/lpc.cc:212-468) and SpectralSmoothing (lpc.cc:473-529) in numpy scalars.

Every operation is written out in np.float32 / np.float64 scalars in the reference's order, with the implicit double promotions of its C++
expressions made explicit.  Two departures from the reference's text, both stated in include/dsr.h: R holds the order+2 values that
autoCorrelation writes (the reference allocates order+1 and overruns by one float, which is why no compiled reference binary pins this
operator), and the weights of PC are signed as in MVDRFeature (lpc.h:156).  The autocorrelation and the all-pass chain exist in two loop
orders: the reference's, and the interchanged one that the device kernels use."""
import numpy as np

f32, f64 = np.float32, np.float64
_1 = f32(1.0)


def rewarp_of(X, correlate, warp, fixed, sens):
    """lpc.cc:352-355 (fixed) / :392-407,425-428 (from the frame); all float but the marked expression"""
    warp, sens = f32(warp), f32(sens)
    if fixed:
        wv = sens + warp
    else:
        R = []
        for i in (0, 1):
            t = f32(0.0)
            for j in range(correlate - i):
                t = t + X[j] * X[j + i]
            R.append(t)
        r = f32(np.abs(R[1] / R[0]))
        wv = f32(f64(sens) * (f64(r) - f64(0.5)) + f64(warp))       # the literal 0.5 promotes the expression
    return (wv - warp) / (_1 - wv * warp)


def autocorr_ref(X, order, warp):
    """lpc.cc:251-273: R[0..order+1], stage after stage over the whole frame"""
    warp = f32(warp); dim = len(X)
    R = [f32(0.0)] * (order + 2)
    t = f32(0.0)
    for j in range(dim):
        t = t + X[j] * X[j]
    R[0] = t
    WX = [f32(v) for v in X]
    for i in range(1, order + 2):
        WT = list(WX)
        WX[0] = -warp * WT[0]
        for j in range(1, dim):
            WX[j] = warp * (WX[j - 1] - WT[j]) + WT[j - 1]
        t = f32(0.0)
        for j in range(dim):
            t = t + X[j] * WX[j]
        R[i] = t
    return R


def autocorr_streamed(X, order, warp):
    """the same sums with the nest interchanged: every stage advances by one sample at a time"""
    warp = f32(warp); dim = len(X); n = order + 2
    R = [f32(0.0)] * n; PO = [f32(0.0)] * n; PN = [f32(0.0)] * n
    r0 = f32(0.0)
    for j in range(dim):
        x = X[j]
        r0 = r0 + x * x
        old = x
        for i in range(1, n):
            nw = -warp * old if j == 0 else warp * (PN[i] - old) + PO[i]
            R[i] = R[i] + x * nw
            PO[i] = old; PN[i] = nw; old = nw
    R[0] = r0
    return R


def compensate_levinson(R, order, warp, rewarp):
    """lpc.cc:275-323 -> (LP[0..order], E[0])"""
    warp = f32(warp); R = list(R)
    a0 = (warp + rewarp) / (_1 + warp * rewarp)
    gj = f32(f64(1.0) - f64(a0 * a0))
    a1 = a0 / gj
    a0 = f32((f64(1.0) + f64(a0 * a0)) / f64(gj))
    g1 = R[0]
    R[0] = f32(f64(a0 * R[0]) + f64(2.0) * f64(a1) * f64(R[1]))
    for i in range(1, order + 1):
        s = a0 * R[i] + a1 * (g1 + R[i + 1])
        g1 = R[i]; R[i] = s
    E = R[0]; E0 = E
    prev = [f32(0.0)] * (order + 1); cur = [f32(0.0)] * (order + 1)
    for i in range(1, order + 1):
        k = R[i]
        for j in range(1, i):
            k = k - prev[j] * R[i - j]
        k = k / E if E != 0 else f32(1000000000)
        cur[i] = k
        for j in range(1, i):
            cur[j] = prev[j] - k * prev[i - j]
        E = (_1 - k * k) * E
        prev, cur = cur, prev
    LP = [_1] + [-prev[i] for i in range(1, order + 1)]
    return LP, E0


def pc_of(A, E0, order):
    """lpc.cc:432-445: float accumulator, mirrored"""
    PC = [f32(0.0)] * (2 * order + 1)
    for i in range(order + 1):
        t = f32(0.0)
        for ii in range(order - i + 1):
            t = t + f32(order + 1 - i - 2 * ii) * A[ii] * A[ii + i]
        PC[order + i] = -t if E0 > 0 else f32(10000000)
    for i in range(1, order + 1):
        PC[order - i] = PC[order + i]
    return PC


def chain_ref(PC, dim, lam):
    """trans_longchain (lpc.cc:374-389) on xm[0..dim] = 0: sample after sample through all the stages"""
    xm = [f32(0.0)] * (dim + 1)
    for w in range(len(PC)):
        x = PC[w]
        for e in range(dim):
            t = (xm[e] + lam * xm[e + 1]) - lam * x
            xm[e] = x
            x = t
    return xm


def chain_staged(PC, dim, lam):
    """the same chain stage after stage: PA[e] is the last input of stage e"""
    x = list(PC); tim = len(x); PA = [f32(0.0)] * (dim + 1)
    for e in range(dim):
        PA[e] = x[tim - 1]
        if e == dim - 1:
            break
        xm1 = f32(0.0); ym1 = f32(0.0)
        for w in range(tim):
            xw = x[w]
            y = (xm1 + lam * ym1) - lam * xw
            x[w] = y; xm1 = xw; ym1 = y
    return PA


def npoints(dim):
    return 1 << int(np.ceil(np.log(f64(dim)) / np.log(2.0)))    # lpc.cc:32-33


def _envelope(re, im, N, E0, outN):
    p = (re * re + im * im).astype(f32)
    p[0] = f32(re[0] * re[0])
    if outN > N // 2:
        p[N // 2] = f32(re[N // 2] * re[N // 2])
    s = np.sqrt(p.astype(f64))
    out = np.full(outN, 10000000.0, f64)
    ok = s > 0
    out[ok] = f64(E0) / s[ok]
    return out


def envelope(PA, E0, dim):
    """fftPower (lpc.cc:44-60) + lpc.cc:457-465: fp64 real transform, power rounded to float"""
    N = npoints(dim); outN = dim // 2 + 1
    temp = np.zeros(N, f64); temp[:dim] = np.array(PA[:dim], f32).astype(f64)
    sp = np.fft.rfft(temp)
    return _envelope(sp.real[:outN].copy(), sp.imag[:outN].copy(), N, E0, outN)


def envelope_longdouble(PA, E0, dim):
    """the same with a direct DFT in long double, rounded to double: what the conditioning of the cases is judged by"""
    ld = np.longdouble
    N = npoints(dim); outN = dim // 2 + 1
    ang = (ld(8.0) * np.arctan(ld(1.0))) * np.arange(N).astype(ld) / ld(N)
    c, s = np.cos(ang), np.sin(ang)
    v = np.array(PA[:dim], f32).astype(ld)
    idx = (np.arange(outN)[:, None] * np.arange(dim)[None, :]) % N
    re = (c[idx] * v[None, :]).sum(axis=1).astype(f64)
    im = (-(s[idx] * v[None, :]).sum(axis=1)).astype(f64)
    return _envelope(re, im, N, E0, outN)


def wtmvdr_frame(X, order, correlate, warp, fixed, sens, streamed=True):
    """one frame -> dict(rewarp, R (before the compensation), E0, PA [dim+1], out [dim/2+1])"""
    X = [f32(v) for v in X]; dim = len(X)
    if correlate < 10:
        correlate = dim                                               # lpc.cc:348
    with np.errstate(all="ignore"):
        rw = rewarp_of(X, correlate, warp, fixed, sens)
        R = (autocorr_streamed if streamed else autocorr_ref)(X, order, warp)
        LP, E0 = compensate_levinson(R, order, warp, rw)
        PC = pc_of(LP, E0, order)
        PA = (chain_staged if streamed else chain_ref)(PC, dim, -rw)
        out = envelope(PA, E0, dim)
    return dict(rewarp=f32(rw), R=np.array(R, f32), E0=f32(E0), PA=np.array(PA, f32), out=out)


def spectral_smoothing(to, frm):
    """SpectralSmoothing::next (lpc.cc:485-529) on one frame: to, frm float64 [size]"""
    size = len(to)
    R = [f32(0.0)] * size
    for i in range(2, size - 2):
        R[i] = f32(f64(frm[i - 2]) / f64(9.0) + f64(2.0) * f64(frm[i - 1]) / f64(9.0) + f64(frm[i]) / f64(3.0)
                   + f64(2.0) * f64(frm[i + 1]) / f64(9.0) + f64(frm[i + 2]) / f64(9.0))
    maxFFT = f32(0.0); maxSPEC = f32(0.0)
    for i in range(size):
        if maxFFT < R[i]:
            maxFFT = R[i]
    for i in range(size):
        v = f32(to[i])
        if maxSPEC < v:
            maxSPEC = v
    with np.errstate(all="ignore"):
        mult = f32(100) * maxFFT if f64(maxSPEC) < f64(0.01) else maxFFT / maxSPEC
    return np.array([f64(mult) * f64(to[i]) for i in range(size)], f64)
