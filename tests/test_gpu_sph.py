"""Spherical-array beamforming and 2-D SRP DOA on the device (dsr_sph_apply, dsr_sph_srp on both paths, the four stream classes) against
the numpy restatement tests/sph_np.py.  The restatement takes the handle's own host tables (getters), so device parity is not confounded with
table rounding.  y and F are complex64 outputs, so they are held to float32 rounding of the frame's largest value; rp and acc (fp64) to 1e-12."""
import os

import numpy as np
import pytest

from tests import sph_np as S
from tests.test_gpu_doa import _check_nbest, _snapshots

pytestmark = pytest.mark.gpu
FS = 16000


def _geometry(Cn, seed=4):
    if Cn == 32:
        return S.eigenmike()
    rng = np.random.default_rng(seed)
    return 42.0, np.arccos(rng.uniform(-1, 1, Cn)), rng.uniform(0, 2 * np.pi, Cn)


def _handle(dsr, kind, nBest, M, Cn, maxOrder, **kw):
    s = dsr.SphDoaSRP(kind, nBest, FS, M, Cn, maxOrder, normalizeWeight=kw.pop("normalizeWeight", False))
    a, th, ph = _geometry(Cn)
    if Cn == 32:
        s.setEigenMikeGeometry()
    else:
        s.setArrayGeometry(a, th, ph)
    return s


@pytest.mark.parametrize("kind,Cn,maxOrder", [("EB", 4, 1), ("DS", 4, 2), ("EB", 32, 4), ("DS", 32, 8), ("EB", 64, 8), ("DS", 64, 3)])
def test_apply_matches_restatement(dsr, cuda, kind, Cn, maxOrder):
    import torch
    M, U, T = 64, 2, 40
    s = _handle(dsr, kind, 1, M, Cn, maxOrder)
    s.setLookDirection(1.0, 0.3)
    X = _snapshots(U, Cn, T, M, seed=Cn + maxOrder)
    nf = [T, 23]
    y, Fo = s.apply(torch.from_numpy(X).to(cuda), torch.tensor(nf, dtype=torch.int32, device=cuda), want_F=True)
    y, Fo = y.cpu().numpy(), Fo.cpu().numpy()
    yr, Fr = S.apply(X, nf, s.harmonics(), s.lookWeights())
    for u, N in enumerate(nf):
        assert np.all(y[u, N:] == 0) and np.all(Fo[u, N:] == 0)
        sy = np.abs(yr[u, :N]).max(axis=1, keepdims=True); sf = np.abs(Fr[u, :N]).max(axis=(1, 2), keepdims=True)
        assert np.all(np.abs(y[u, :N] - yr[u, :N]) <= 2e-7 * sy)
        assert np.all(np.abs(Fo[u, :N] - Fr[u, :N]) <= 2e-7 * sf)


CASES = [  # kind, C, maxOrder, search or None (constructor 25 x 25) / "default" (setSearchParam() 31 x 63), range, nBest, extra
    ("EB", 4, 1, (0.5, 0.6, 1.0, 1.1, 0.1, 0.1), None, 1, {}),                  # 1 x 1
    ("DS", 4, 2, None, None, 3, {}),
    ("EB", 32, 4, "default", None, 2, {}),
    ("DS", 32, 4, (0.0, np.pi, -np.pi, np.pi, 0.3, 0.3), (0, 20), 4, {}),
    ("EB", 32, 8, (0.0, np.pi, -np.pi, np.pi, 0.25, 0.25), (9, 9), 2, dict(sigma2=0.05, normalizeWeight=True, wgain=1.5)),
    ("DS", 64, 8, None, (0, 32), 2, dict(normalizeWeight=True)),
    ("EB", 64, 2, "default", (5, 30), 5, {}),
]


def _run_case(dsr, cuda, kind, Cn, maxOrder, search, rng, nBest, extra, path, monkeypatch):
    import torch
    M, U, T = 64, 2, 70
    extra = dict(extra)
    s = _handle(dsr, kind, nBest, M, Cn, maxOrder, normalizeWeight=extra.pop("normalizeWeight", False))
    if "sigma2" in extra:
        s.setSigma2(extra["sigma2"])
    if "wgain" in extra:
        s.setWeightGain(extra["wgain"])
    if search == "default":
        s.setSearchParam()
    elif search is not None:
        s.setSearchParam(*search)
    if rng is not None:
        s.setFrequencyRange(*rng)
    fmin, fmax = s.frequencyRange()
    nU = s.units()
    X = _snapshots(U, Cn, T, M, seed=Cn * 3 + maxOrder, silent=[(0, 10, 20)])
    nframes = [T, 41]
    W = np.stack([s.steering(k)[:fmax + 1] for k in range(nU)], axis=1)       # [f][unit][dim], the handle's own table
    Sh = s.harmonics()
    ref0 = S.run(X, nframes, Sh, W, M, nBest, fmin, fmax, 0.0)
    thr = float(np.float32(np.sqrt(ref0["energy"][0, 10:20].max() * ref0["energy"][0, 25:].min())))
    s.setEnergyThreshold(thr)
    ref = S.run(X, nframes, Sh, W, M, nBest, fmin, fmax, thr)
    assert ref["gated"][0, 10:20].all() and ref["gated"].sum() == 10
    monkeypatch.setenv("DSR_SPH_SRP_PATH", path)
    assert s.path() == path
    Xd = torch.from_numpy(X).to(cuda)
    nf = torch.tensor(nframes, dtype=torch.int32, device=cuda)
    import ctypes as C
    sent = dict(energy=torch.full((U, T), -7.0, dtype=torch.float32, device=cuda), rp=torch.full((U, T, nU), -7.0, dtype=torch.float64, device=cuda),
                nbr=torch.full((U, T, nBest), -7.0, dtype=torch.float64, device=cuda), nbi=torch.full((U, T, nBest), -7, dtype=torch.int32, device=cuda),
                y=torch.full((U, T, M // 2 + 1, 2), -7.0, dtype=torch.float32, device=cuda), g=torch.full((U, T), -7, dtype=torch.int32, device=cuda))
    acc = torch.zeros((U, nU), dtype=torch.float64, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    dsr.check(dsr._lib.dsr_sph_srp(s.h, p(torch.view_as_real(Xd)), p(nf), U, T, p(sent["energy"]), p(sent["rp"]), p(sent["nbr"]), p(sent["nbi"]),
                                   p(acc), p(sent["y"]), p(sent["g"]), dsr.cur_stream()))
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in sent.items()}
    accd = acc.cpu().numpy()
    for u, N in enumerate(nframes):
        for k, v in h.items():
            assert np.all(v[u, N:] == -7), (k, u)                            # frames past nframes untouched
        assert np.array_equal(h["energy"][u, :N], ref["energy"][u, :N])     # bit for bit
        assert np.array_equal(h["g"][u, :N], ref["gated"][u, :N])
        rr = ref["rp"][u, :N]
        assert np.all(np.abs(h["rp"][u, :N] - rr) <= 1e-12 * rr.max(axis=1, keepdims=True))
        _check_nbest(h["nbr"][u, :N], h["nbi"][u, :N], ref["nbest_rp"][u, :N], ref["nbest_idx"][u, :N])
        yd = h["y"][u, :N, :, 0] + 1j * h["y"][u, :N, :, 1]
        yr = ref["y"][u, :N, fmin:fmax + 1]
        assert np.all(np.abs(yd[:, fmin:fmax + 1] - yr) <= 2e-7 * np.maximum(np.abs(yr).max(axis=1, keepdims=True), 1e-300))
    assert np.all(np.abs(accd - ref["acc"]) <= 1e-12 * np.abs(ref["acc"]).max(axis=1, keepdims=True))
    Rf, If = s.finalNBest(accd)
    for u in range(U):
        Rr, Ir = S.D.nbest(ref["acc"][u], nBest)
        _check_nbest(Rf[u][None], If[u][None], Rr[None], Ir[None])
    return h


@pytest.mark.parametrize("case", range(len(CASES)))
def test_srp_both_paths(dsr, cuda, case, monkeypatch):
    h1 = _run_case(dsr, cuda, *CASES[case], "fused", monkeypatch)
    h2 = _run_case(dsr, cuda, *CASES[case], "folded", monkeypatch)
    assert np.array_equal(h1["energy"], h2["energy"]) and np.array_equal(h1["g"], h2["g"])


@pytest.mark.parametrize("path", ["fused", "folded"])
def test_acc_carried_over_two_blocks(dsr, cuda, path, monkeypatch):
    import torch
    monkeypatch.setenv("DSR_SPH_SRP_PATH", path)
    U, Cn, T, M = 2, 32, 120, 64
    X = _snapshots(U, Cn, T, M, seed=9, silent=[(0, 30, 60)])
    s = _handle(dsr, "EB", 2, M, Cn, 4); s.setEnergyThreshold(1e-3)
    Xd = torch.from_numpy(X).to(cuda)
    one = s.srp(Xd)["acc"]
    acc = torch.zeros_like(one)
    s.srp(Xd[:, :, :53].contiguous(), acc=acc)
    s.srp(Xd[:, :, 53:].contiguous(), acc=acc)
    a1, a2 = one.cpu().numpy(), acc.cpu().numpy()
    assert np.all(np.abs(a1 - a2) <= 1e-13 * np.abs(a1).max())


def test_plane_wave_on_eigenmike(dsr, cuda):
    """a synthetic rigid-sphere plane wave from (theta0, phi0), built with the handle's own b_n: both DOA kinds find the nearest grid point"""
    import torch
    M, T = 256, 40
    theta0, phi0 = 1.13, -0.71
    for kind, mo in (("EB", 4), ("DS", 3)):
        s = dsr.SphDoaSRP(kind, 2, FS, M, 32, mo); s.setEigenMikeGeometry(); s.setSearchParam()
        s.setFrequencyRange(20, 100)
        a, th_s, ph_s = S.eigenmike()
        X = S.plane_wave(s.modeAmplitudes(), None, th_s, ph_s, theta0, phi0, mo, T)[None]
        r = s.srp(torch.from_numpy(X).to(cuda))
        R, I = s.finalNBest(r["acc"])
        th, ph = s.grid()
        nearest = np.argmin((th - theta0) ** 2 + (ph - phi0) ** 2)
        assert I[0, 0] == nearest, (kind, th[I[0, 0]], ph[I[0, 0]], th[nearest], ph[nearest])


def _banks(protos, xt):
    from dsr.btk.feature import SampleFeaturePtr
    from dsr.btk.modulated import OverSampledDFTAnalysisBankPtr
    M, m, r, h, g = protos["M256-m4-r1"]
    D_ = M >> r
    out = []
    for c in range(xt.shape[0]):
        s = SampleFeaturePtr(blockLen=D_, shiftLen=D_, padZeros=True); s.setSamples(xt[c], FS)
        out.append(OverSampledDFTAnalysisBankPtr(s, prototype=h, M=M, m=m, r=r))
    return out, M


def _snap(protos, xt):
    banks, M = _banks(protos, xt)
    return np.stack([np.array([np.array(b) for b in bank]) for bank in banks])[:, :, : M // 2 + 1].astype(np.complex64), M


@pytest.mark.parametrize("cls", ["EigenBeamformerPtr", "SphericalDSBeamformerPtr"])
def test_beamformer_streams(dsr, cuda, protos, cls):
    import dsr.btk.beamformer as BF
    Cn = 4
    rng = np.random.default_rng(1)
    xt = (rng.standard_normal((Cn, 128 * 300)) * 100).astype(np.float32)
    a, th, ph = _geometry(Cn)
    bf = getattr(BF, cls)(FS, 256, maxOrder=3)
    banks, M = _banks(protos, xt)
    for b in banks:
        bf.setChannel(b)
    bf.setArrayGeometry(a, th, ph); bf.setLookDirection(0.9, 2.0)
    X, _ = _snap(protos, xt)
    h = bf._handle()
    yr, Fr = S.apply(X[None], [X.shape[1]], h.harmonics(), h.lookWeights())
    n = 0
    for t, v in enumerate(bf):
        scale = np.abs(yr[0, t]).max()
        assert np.abs(v[: M // 2 + 1] - yr[0, t]).max() <= 2e-7 * scale
        assert np.abs(v[M // 2 + 1:] - np.conj(yr[0, t, 1:M // 2][::-1])).max() <= 2e-7 * scale
        if t in (0, 150):
            F = bf.getSnapShotArray()
            assert np.abs(F - Fr[0, t]).max() <= 2e-7 * np.abs(Fr[0, t]).max()
        n += 1
    assert n == X.shape[1] and n >= 250
    if cls == "SphericalDSBeamformerPtr":
        assert bf.calcWNG().shape == (M // 2 + 1,)


@pytest.mark.parametrize("cls,kind", [("DOAEstimatorSRPEBPtr", "EB"), ("DOAEstimatorSRPSphDSBPtr", "DS")])
def test_doa_streams_state(dsr, cuda, protos, cls, kind):
    import dsr.btk.beamformer as BF
    Cn, mo = 4, 2
    rng = np.random.default_rng(3)
    xt = (rng.standard_normal((Cn, 128 * 260)) * 100).astype(np.float32)
    xt[:, 128 * 100:128 * 140] = 0.0                                         # a silent stretch: gated frames
    a, th_s, ph_s = _geometry(Cn)
    est = getattr(BF, cls)(3, FS, 256, maxOrder=mo)
    banks, M = _banks(protos, xt)
    for b in banks:
        est.setChannel(b)
    est.setArrayGeometry(a, th_s, ph_s)
    est.setSearchParam(0.0, np.pi, -np.pi, np.pi, 0.5, 0.5)
    est.setEnergyThreshold(1e-6)
    X, _ = _snap(protos, xt)
    h = est._handle()
    T = X.shape[1]
    th, ph = h.grid(); nT, nP = h.gridN()
    W = np.stack([h.steering(k) for k in range(len(th))], axis=1)
    ref = S.run(X[None], [T], h.harmonics(), W, M, 3, 1, M // 2, 1e-6)
    assert 0 < ref["gated"].sum() < T
    last = np.zeros(M, np.complex128)
    for t, v in enumerate(est):
        assert np.float32(est.getEnergy()) == ref["energy"][0, t]
        R, Dm = est.getNBestRPs(), est.getNBestDOAs()
        if ref["gated"][0, t]:
            assert np.all(R == -10e10) and np.all(Dm == -np.pi)
            np.testing.assert_array_equal(v, last)
        else:
            idx = np.array([int(np.flatnonzero((th == d[0]) & (ph == d[1]))[0]) for d in Dm])
            _check_nbest(R[None], idx[None], ref["nbest_rp"][0, t][None], ref["nbest_idx"][0, t][None])
            rpm = est.getResponsePowerMatrix()
            assert rpm.shape == (nT, nP)
            assert np.all(np.abs(rpm.ravel() - ref["rp"][0, t]) <= 1e-12 * ref["rp"][0, t].max())
            y = ref["y"][0, t]
            sc = np.abs(y[1:M // 2 + 1]).max()
            assert np.abs(v[1:M // 2 + 1] - y[1:M // 2 + 1]).max() <= 2e-7 * sc
            assert np.abs(v[M // 2 + 1:] - np.conj(y[1:M // 2][::-1])).max() <= 2e-7 * sc
        if t == T // 2:
            acc_ref = S.run(X[None, :, :t + 1], [t + 1], h.harmonics(), W, M, 3, 1, M // 2, 1e-6)["acc"][0]
            assert np.all(np.abs(est.getAccumulators() - acc_ref) <= 1e-12 * np.abs(acc_ref).max())
        last = np.array(v)
    assert np.all(est.getNBestRPs() == -10e10)                               # the pull that ended the stream reset the N-best first
    est.getFinalNBestHypotheses()
    Rr, Ir = S.D.nbest(ref["acc"][0], 3)
    got = est.getNBestDOAs()
    idx = np.array([int(np.flatnonzero((th == d[0]) & (ph == d[1]))[0]) for d in got])
    _check_nbest(est.getNBestRPs()[None], idx[None], Rr[None], Ir[None])
    assert np.array_equal(est.getResponsePowerMatrix().ravel(), est.getAccumulators())
    for _ in est:                                                            # reset() keeps the accumulators: a second pass doubles them
        pass
    assert np.all(np.abs(est.getAccumulators() - 2 * ref["acc"][0]) <= 1e-12 * np.abs(ref["acc"][0]).max())
    est.initAccs()
    assert np.all(est.getAccumulators() == 0)
    est.setSearchParam()                                                     # clears them; the Python default grid (31 x 63)
    for _ in est:
        pass
    assert est.getAccumulators().shape == (31 * 63,) and est.getResponsePowerMatrix().shape == (31, 63)


def test_estimate_steers_beamformer(dsr, cuda, protos):
    """getNBestDOAs()[0] fed to SphericalDSBeamformerPtr.setLookDirection: the beamformer's weights are those of the winning unit"""
    import dsr.btk.beamformer as BF
    Cn = 4
    rng = np.random.default_rng(8)
    xt = (rng.standard_normal((Cn, 128 * 60)) * 100).astype(np.float32)
    a, th_s, ph_s = _geometry(Cn)
    est = BF.DOAEstimatorSRPSphDSBPtr(1, FS, 256, maxOrder=3)
    banks, M = _banks(protos, xt)
    for b in banks:
        est.setChannel(b)
    est.setArrayGeometry(a, th_s, ph_s); est.setSearchParam(0.0, np.pi, -np.pi, np.pi, 0.5, 0.5)
    for _ in est:
        pass
    est.getFinalNBestHypotheses()
    theta, phi = est.getNBestDOAs()[0]
    bf = BF.SphericalDSBeamformerPtr(FS, 256, maxOrder=3)
    for b in _banks(protos, xt)[0]:
        bf.setChannel(b)
    bf.setArrayGeometry(a, th_s, ph_s); bf.setLookDirection(theta, phi)
    h = est._handle(); th, ph = h.grid()
    k = int(np.flatnonzero((th == theta) & (ph == phi))[0])
    assert np.abs(bf._handle().lookWeights()[1:] - h.steering(k)[1:]).max() <= 1e-15 * np.abs(h.steering(k)).max()
    assert sum(1 for _ in bf) == _snap(protos, xt)[0].shape[1]


def _rigid_sphere_time(theta0, phi0, maxOrder, n, seed=13):
    """EigenMike signals of white noise arriving as a rigid-sphere plane wave from (theta0, phi0): each channel's spectrum times
    4 pi sum_n i^n b_n(ka) sum_m conj(Y_n^m(theta0, phi0)) Y_n^m(theta_c, phi_c), b_n at every frequency of one long DFT"""
    a, th_s, ph_s = S.eigenmike()
    N2 = 1 << int(np.ceil(np.log2(n)))
    X = np.fft.rfft(np.random.default_rng(seed).standard_normal(N2))
    ka = 2 * np.pi * np.arange(X.size) * FS * a / (N2 * S.SSPEED)
    nidx = np.array([o for o in range(maxOrder) for m in range(-o, o + 1)])
    B = np.array([[S.mode_amplitude(o, x) for o in range(maxOrder)] for x in ka])
    g = 4 * np.pi * np.array([1, 1j, -1, -1j])[nidx % 4] * B[:, nidx]                          # [K][dim]
    Ys = np.stack([S.harmonics_at(maxOrder, t, p) for t, p in zip(th_s, ph_s)])                # [C][dim]
    resp = (g * np.conj(S.harmonics_at(maxOrder, theta0, phi0))) @ Ys.T                       # [K][C]
    return (np.fft.irfft(X[:, None] * resp, N2, axis=0)[:n].T * 100.0).astype(np.float32)


@pytest.mark.parametrize("cls,mo", [("DOAEstimatorSRPEBPtr", 4), ("DOAEstimatorSRPSphDSBPtr", 3)])
def test_plane_wave_through_stream_classes(dsr, cuda, protos, cls, mo):
    """the stream classes end to end, analysis banks included: getFinalNBestHypotheses returns the grid point nearest (theta0, phi0)"""
    import dsr.btk.beamformer as BF
    theta0, phi0 = 1.13, -0.71
    xt = _rigid_sphere_time(theta0, phi0, mo, 128 * 70)
    est = getattr(BF, cls)(2, FS, 256, maxOrder=mo)
    for b in _banks(protos, xt)[0]:
        est.setChannel(b)
    est.setEigenMikeGeometry(); est.setSearchParam(); est.setFrequencyRange(20, 100)
    n = sum(1 for _ in est)
    assert n >= 70
    est.getFinalNBestHypotheses()
    th, ph = est._handle().grid()
    k = np.argmin((th - theta0) ** 2 + (ph - phi0) ** 2)
    assert tuple(est.getNBestDOAs()[0]) == (th[k], ph[k]), (est.getNBestDOAs()[0], th[k], ph[k])


def test_settings_changed_mid_stream(dsr, cuda, protos):
    """setLookDirection and setArrayGeometry between pulls: the frames after the change use the new weights / harmonics"""
    import dsr.btk.beamformer as BF
    Cn = 4
    xt = (np.random.default_rng(21).standard_normal((Cn, 128 * 80)) * 100).astype(np.float32)
    a, th, ph = _geometry(Cn)
    bf = BF.EigenBeamformerPtr(FS, 256, maxOrder=2)
    for b in _banks(protos, xt)[0]:
        bf.setChannel(b)
    bf.setArrayGeometry(a, th, ph)
    X, M = _snap(protos, xt)
    it = iter(bf)
    for _ in range(10):
        v = next(it)
    h = bf._handle()
    bf.setLookDirection(0.4, 1.7)
    v = next(it)
    yr, _ = S.apply(X[None], [X.shape[1]], h.harmonics(), h.lookWeights())
    assert np.abs(v[: M // 2 + 1] - yr[0, 10]).max() <= 2e-7 * np.abs(yr[0, 10]).max()
    bf.setArrayGeometry(60.0, th[::-1].copy(), ph[::-1].copy())
    v = next(it)
    F = bf.getSnapShotArray()
    yr, Fr = S.apply(X[None], [X.shape[1]], h.harmonics(), h.lookWeights())
    assert np.abs(v[: M // 2 + 1] - yr[0, 11]).max() <= 2e-7 * np.abs(yr[0, 11]).max()
    assert np.abs(F - Fr[0, 11]).max() <= 2e-7 * np.abs(Fr[0, 11]).max()
