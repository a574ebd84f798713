"""Steered-response-power DOA on the device (dsr_doa_srp, the DOAEstimatorSRPDSBLAPtr stream) against the numpy restatement
tests/doa_srp_np.py: energy bit for bit, the gate, rp / acc to 1e-12, the N-best, the last unit's beamformed bins, block-wise accumulation,
the stream face's state while iterating, and a plane wave through the analysis bank."""
import ctypes as C

import numpy as np
import pytest

from tests import doa_srp_np as D

pytestmark = pytest.mark.gpu
FS = 16000


def _snapshots(U, Cn, T, M, seed, silent=()):
    """random array snapshots [U][C][T][M/2+1] complex64 with a common source (so the directions differ) and planted silent segments"""
    rng = np.random.default_rng(seed)
    F = M // 2 + 1
    S = rng.standard_normal((U, 1, T, F)) + 1j * rng.standard_normal((U, 1, T, F))
    ph = np.exp(1j * rng.uniform(-np.pi, np.pi, (1, Cn, 1, F)))
    X = S * ph + 0.3 * (rng.standard_normal((U, Cn, T, F)) + 1j * rng.standard_normal((U, Cn, T, F)))
    for u, a, b in silent:
        X[u, :, a:b] *= 1e-4
    return X.astype(np.complex64)


def _check_nbest(Rd, Id, Rr, Ir):
    """every rank's power within rel 1e-12; the index equal wherever the neighbouring ranks are more than 1e-9 apart (no order among near-ties)"""
    scale = np.maximum(np.abs(Rr).max(axis=-1, keepdims=True), 1e-300)
    assert np.all(np.abs(Rd - Rr) <= 1e-12 * scale)
    nB = Rr.shape[-1]
    for n in range(nB):
        sep = np.ones(Rr.shape[:-1], bool)
        if n > 0:
            sep &= np.abs(Rr[..., n] - Rr[..., n - 1]) > 1e-9 * scale[..., 0]
        if n + 1 < nB:
            sep &= np.abs(Rr[..., n] - Rr[..., n + 1]) > 1e-9 * scale[..., 0]
        assert np.array_equal(Id[..., n][sep], Ir[..., n][sep])


CASES = [  # C, M, (minTheta, maxTheta, width) or None = the constructor's 31 directions, frequency range or None = default, nBest
    (2, 64, (0.0, 0.1, 0.1), None, 1),
    (3, 64, (0.0, np.pi, 0.185), (0, 32), 3),
    (8, 64, None, None, 4),
    (8, 64, None, (32, 32), 2),
    (64, 32, (0.0, np.pi + np.pi / 180, np.pi / 180), (0, 16), 5),
    (64, 32, (0.3, 2.0, 0.1), None, 3),
]


@pytest.mark.parametrize("Cn,M,search,rng,nBest", CASES)
def test_srp_matches_restatement(dsr, cuda, Cn, M, search, rng, nBest):
    import torch
    U, T = 3, 150
    nframes = [T, 97, 1]
    X = _snapshots(U, Cn, T, M, seed=Cn * 7 + M, silent=[(0, 20, 40), (1, 60, 70)])
    x = np.sort(np.random.default_rng(Cn).uniform(0, 2e-3, Cn + 1))
    d = dsr.DoaSRP(nBest, FS, M, Cn)
    d.setArrayGeometry(x)
    if search is not None:
        d.setSearchParam(*search)
    if rng is not None:
        d.setFrequencyRange(*rng)
    fmin, fmax = d.frequencyRange()
    thetas = d.thetas()
    assert len(thetas) == (31 if search is None else len(D.theta_grid(*search)))
    ref0 = D.run(X, nframes, x, FS, M, nBest, thetas, fmin, fmax, 0.0)
    thr = float(np.float32(np.sqrt(ref0["energy"][0, 20:40].max() * ref0["energy"][0, 45:].min())))    # between the silent and the rest
    d.setEnergyThreshold(thr)
    ref = D.run(X, nframes, x, FS, M, nBest, thetas, fmin, fmax, thr)
    assert ref["gated"][0, 20:40].all() and ref["gated"][1, 60:70].all() and ref["gated"].sum() == 30

    Xd = torch.from_numpy(X).to(cuda)
    nf = torch.tensor(nframes, dtype=torch.int32, device=cuda)
    # every output pre-filled with a sentinel: the frames past nframes must keep it
    sent = dict(energy=torch.full((U, T), -7.0, dtype=torch.float32, device=cuda), rp=torch.full((U, T, len(thetas)), -7.0, dtype=torch.float64, device=cuda),
                nbr=torch.full((U, T, nBest), -7.0, dtype=torch.float64, device=cuda), nbi=torch.full((U, T, nBest), -7, dtype=torch.int32, device=cuda),
                y=torch.full((U, T, M // 2 + 1, 2), -7.0, dtype=torch.float32, device=cuda), g=torch.full((U, T), -7, dtype=torch.int32, device=cuda))
    acc = torch.zeros((U, len(thetas)), dtype=torch.float64, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())
    dsr.check(dsr._lib.dsr_doa_srp(d.h, p(torch.view_as_real(Xd)), p(nf), U, T, p(sent["energy"]), p(sent["rp"]), p(sent["nbr"]), p(sent["nbi"]),
                                   p(acc), p(sent["y"]), p(sent["g"]), dsr.cur_stream()))
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in sent.items()}
    accd = acc.cpu().numpy()
    for u, N in enumerate(nframes):
        for k, v in h.items():
            assert np.all(v[u, N:] == -7), (k, u)
        assert np.array_equal(h["energy"][u, :N], ref["energy"][u, :N])                 # bit for bit
        assert np.array_equal(h["g"][u, :N], ref["gated"][u, :N])
        rr = ref["rp"][u, :N]
        assert np.all(np.abs(h["rp"][u, :N] - rr) <= 1e-12 * rr.max(axis=1, keepdims=True))
        _check_nbest(h["nbr"][u, :N], h["nbi"][u, :N], ref["nbest_rp"][u, :N], ref["nbest_idx"][u, :N])
        yd = h["y"][u, :N, :, 0] + 1j * h["y"][u, :N, :, 1]
        yr = ref["y"][u, :N]
        rms = np.sqrt((np.abs(yr[:, fmin:fmax + 1]) ** 2).mean(axis=1, keepdims=True))
        assert np.all(np.abs(yd[:, fmin:fmax + 1] - yr[:, fmin:fmax + 1]) <= 2e-6 * np.maximum(rms, 1e-30))
    assert np.all(np.abs(accd - ref["acc"]) <= 1e-12 * np.abs(ref["acc"]).max(axis=1, keepdims=True))
    Rf, If = d.finalNBest(accd)
    for u in range(U):
        Rr, Ir = D.nbest(ref["acc"][u], nBest)
        _check_nbest(Rf[u][None], If[u][None], Rr[None], Ir[None])


def test_acc_carried_over_two_blocks(dsr, cuda):
    import torch
    U, Cn, T, M = 2, 8, 200, 64
    X = _snapshots(U, Cn, T, M, seed=3, silent=[(0, 50, 90)])
    x = np.arange(Cn + 1) * 6.25e-5
    d = dsr.DoaSRP(3, FS, M, Cn); d.setArrayGeometry(x); d.setEnergyThreshold(1e-3)
    Xd = torch.from_numpy(X).to(cuda)
    one = d.srp(Xd)["acc"]
    acc = torch.zeros_like(one)
    d.srp(Xd[:, :, :77].contiguous(), acc=acc)
    d.srp(Xd[:, :, 77:].contiguous(), acc=acc)
    a1, a2 = one.cpu().numpy(), acc.cpu().numpy()
    assert np.all(np.abs(a1 - a2) <= 1e-13 * np.abs(a1).max())


def _stream_setup(protos, x_time, positions, nBest=3):
    from dsr.btk.feature import SampleFeaturePtr
    from dsr.btk.modulated import OverSampledDFTAnalysisBankPtr
    from dsr.btk.beamformer import DOAEstimatorSRPDSBLAPtr
    M, m, r, h, g = protos["M256-m4-r1"]
    D_ = M >> r
    est = DOAEstimatorSRPDSBLAPtr(nBest, FS, M)
    banks = []
    for c in range(x_time.shape[0]):
        s = SampleFeaturePtr(blockLen=D_, shiftLen=D_, padZeros=True); s.setSamples(x_time[c], FS)
        est.setChannel(OverSampledDFTAnalysisBankPtr(s, prototype=h, M=M, m=m, r=r))
        s2 = SampleFeaturePtr(blockLen=D_, shiftLen=D_, padZeros=True); s2.setSamples(x_time[c], FS)
        banks.append(OverSampledDFTAnalysisBankPtr(s2, prototype=h, M=M, m=m, r=r))
    est.setArrayGeometry(positions)
    X = np.stack([np.array([np.array(b) for b in bank]) for bank in banks])[:, :, : M // 2 + 1].astype(np.complex64)   # [C][T][F]
    return est, X, M


def _plane_wave_time(Cn, n, theta0, spacing, seed=11):
    """white noise arriving from theta0: channel c delayed by c spacing cos(theta0) seconds (a fractional delay in the DFT domain)"""
    rng = np.random.default_rng(seed)
    N2 = 1 << int(np.ceil(np.log2(n)))
    S = np.fft.rfft(rng.standard_normal(N2))
    k = np.arange(S.size)
    return np.stack([np.fft.irfft(S * np.exp(-2j * np.pi * k * c * spacing * np.cos(theta0) * FS / N2), N2)[:n] for c in range(Cn)]).astype(np.float32)


def test_stream_face_state_while_iterating(dsr, cuda, protos):
    Cn, n = 4, 6000
    xt = _plane_wave_time(Cn, n, 1.1, 1.0 / FS) * 1000.0
    xt[:, 2000:3500] = 0.0                                                   # a silent stretch: gated frames
    pos = np.arange(Cn) / FS
    est, X, M = _stream_setup(protos, xt, pos, nBest=3)
    est.setEnergyThreshold(1e-6)
    thetas = D.theta_grid(-np.pi / 2, np.pi / 2, 0.1)
    T = X.shape[1]
    ref = D.run(X[None], [T], pos, FS, M, 3, thetas, 1, M // 2, 1e-6)
    assert 0 < ref["gated"].sum() < T
    last = np.zeros(M, np.complex128)
    for t, v in enumerate(est):
        assert np.float32(est.getEnergy()) == ref["energy"][0, t]
        R, Dm = est.getNBestRPs(), est.getNBestDOAs()
        if ref["gated"][0, t]:
            assert np.all(R == -10e10) and np.all(Dm == -np.pi)
            np.testing.assert_array_equal(v, last)                           # the previous frame's output
        else:
            _check_nbest(R[None], np.array([thetas.tolist().index(th) for th in Dm[:, 0]])[None], ref["nbest_rp"][0, t][None], ref["nbest_idx"][0, t][None])
            assert np.all(Dm[:, 1] == 0.0)
            rpm = est.getResponsePowerMatrix()
            assert rpm.shape == (len(thetas), 1)
            assert np.all(np.abs(rpm[:, 0] - ref["rp"][0, t]) <= 1e-12 * ref["rp"][0, t].max())
            y = ref["y"][0, t]
            rms = np.sqrt((np.abs(y[1:M // 2 + 1]) ** 2).mean())
            assert np.abs(v[1:M // 2 + 1] - y[1:M // 2 + 1]).max() <= 2e-6 * rms
            assert np.abs(v[M // 2 + 1:] - np.conj(y[1:M // 2][::-1])).max() <= 2e-6 * rms
            assert v[0] == 0                                                 # outside [fbinMin, fbinMax]: never written
        acc_ref = D.run(X[None, :, :t + 1], [t + 1], pos, FS, M, 3, thetas, 1, M // 2, 1e-6)["acc"][0] if t in (0, T // 2) else None
        if acc_ref is not None:
            assert np.all(np.abs(est.getAccumulators() - acc_ref) <= 1e-12 * np.abs(acc_ref).max())
        last = np.array(v)
    assert np.all(est.getNBestRPs() == -10e10)                               # the pull that ended the stream reset the N-best first
    est.getFinalNBestHypotheses()
    Rr, Ir = D.nbest(ref["acc"][0], 3)
    _check_nbest(est.getNBestRPs()[None], np.array([thetas.tolist().index(th) for th in est.getNBestDOAs()[:, 0]])[None], Rr[None], Ir[None])
    np.testing.assert_allclose(est.getResponsePowerMatrix()[:, 0], est.getAccumulators(), rtol=0, atol=0)
    # reset() keeps the accumulators: a second pass doubles them
    for _ in est:
        pass
    assert np.all(np.abs(est.getAccumulators() - 2 * ref["acc"][0]) <= 1e-12 * np.abs(ref["acc"][0]).max())
    est.initAccs()
    assert np.all(est.getAccumulators() == 0)
    # setSearchParam clears them and rebuilds the grid: the Python default (0, pi/2, 0.1)
    est.setSearchParam()
    for _ in est:
        pass
    th2 = D.theta_grid(0.0, np.pi / 2, 0.1)
    ref2 = D.run(X[None], [T], pos, FS, M, 3, th2, 1, M // 2, 1e-6)
    assert est.getAccumulators().shape == (len(th2),)
    assert np.all(np.abs(est.getAccumulators() - ref2["acc"][0]) <= 1e-12 * np.abs(ref2["acc"][0]).max())


def test_plane_wave_end_to_end(dsr, cuda, protos):
    Cn, theta0 = 8, 0.7
    xt = _plane_wave_time(Cn, 8000, theta0, 1.0 / FS) * 1000.0
    pos = np.arange(Cn) / FS
    est, X, M = _stream_setup(protos, xt, pos, nBest=2)
    est.setSearchParam(0.0, np.pi, 0.05)
    for _ in est:
        pass
    est.getFinalNBestHypotheses()
    grid = D.theta_grid(0.0, np.pi, 0.05)
    assert est.getNBestDOAs()[0, 0] == grid[np.argmin(np.abs(grid - theta0))]
