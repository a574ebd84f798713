"""GPU tests of the noise-suppression and binaural-mask operators (include/dsr.h 6a-2, 6a-3): the device through the C-ABI against the numpy
restatement (tests/postfilter2_np.py) on the shared cases; carried runs against whole runs; rows past nframes; untouched state for nframes = 0.

Tolerances (none invented here): fp64 state 1e-12 of its scale (as test_gpu_gcc.py, test_gpu_doa.py); complex64 outputs: the 2e-5 of the frame's RMS of
test_gpu_parity.py:48 tightened to twice the largest error of the first GPU run (C64 below); mu bit for bit on comparable items; estimator accumulators 4 n 2^-53 relative plus the measured pow() difference (postfilter2_cases.acc_bound);
calcThreshold the same candidate index.
Every test prints its largest error before it asserts."""
import numpy as np
import pytest

from tests import postfilter2_cases as K
from tests import postfilter2_np as P
from tests.test_postfilter2_np_cpu import comparable

pytestmark = pytest.mark.gpu

F64 = 1e-12
C64 = 4.08e-7      # twice the largest complex64 output error the GPU tests print, 2.04e-7 of the frame RMS; the inherited bound is 2e-5


def _t(x, cuda, dt=None):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).to(cuda) if dt is None else torch.tensor(x, dtype=dt, device=cuda)


def _nf(v, cuda):
    import torch
    return torch.tensor(v, dtype=torch.int32, device=cuda)


def _out_err(got, want, nframes, label):
    """largest error of a frame relative to the frame's RMS; rows past nframes must be zero"""
    worst = 0.0
    for u, n in enumerate(nframes):
        assert not np.any(got[u, n:]), (label, u, "rows past nframes are not zero")
        for t in range(n):
            rms = np.sqrt(np.mean(np.abs(want[u, t]) ** 2))
            if rms > 0:
                worst = max(worst, np.abs(got[u, t] - want[u, t]).max() / rms)
    print("%s: output error %.3g of the frame RMS" % (label, worst))
    return worst


@pytest.mark.parametrize("full", [False, True])
@pytest.mark.parametrize("c", K.SS_CASES, ids=lambda c: c["name"])
def test_spectral_subtractor_against_restatement(dsr, cuda, c, full):
    X = K.ss_input(c); want, est = K.ss_reference(c, full); U = X[0].shape[0]
    s = dsr.SpectralSubtractor(c["M"], False, c["ft"], c["floor"])
    for a in c["alphas"]:
        s.setChannel(a)
    st = s.newState(U, cuda)
    for b in range(3):
        if b == 1:
            s.stopTraining(st); s.startNoiseSubtraction()
        if b == 2:
            s.startTraining()
        got = s.apply(_t(X[b], cuda), st, _nf(c["nframes"][b], cuda), full=full).cpu().numpy()
        assert _out_err(got, want[b], c["nframes"][b], "%s block %d" % (c["name"], b)) <= C64
    for u in range(U):
        for ch in range(len(c["alphas"])):
            e = s.read(st, 0, u, ch); scale = max(np.abs(est[u, ch]).max(), 1e-300)
            assert np.abs(e - est[u, ch]).max() <= F64 * scale, (c["name"], u, ch)


def test_spectral_subtractor_controls(dsr, cuda, tmp_path):
    """a zero-frame call leaves the state alone; stopTraining without a sample is refused; clear / clearNoiseSamples; noise file through the state"""
    import torch
    M, F = 64, 33
    s = dsr.SpectralSubtractor(M); s.setChannel(-1.0); s.setChannel(0.5); st = s.newState(2, cuda)
    X = _t(K.snapshots(5, (2, 2, 4, F)), cuda)
    s.apply(X, st, _nf([4, 0], cuda)); before = st.clone()
    s.apply(X, st, _nf([0, 0], cuda)); assert torch.equal(before, st)
    assert s.read(st, 2, 0, 0).tolist() == [4.0, 0.0] and s.read(st, 2, 0, 1).tolist() == [0.0, 1.0] and s.read(st, 2, 1, 1).tolist() == [0.0, 0.0]
    with pytest.raises(dsr.DsrError) as e:
        s.stopTraining(st)                                                  # utterance 1 has no sample to average
    assert e.value.status == 3 and torch.equal(before, st)
    s.startTraining(); s.apply(X, st, _nf([0, 2], cuda)); s.stopTraining(st)
    x = X.cpu().numpy().astype(np.complex128)
    assert np.abs(s.read(st, 0, 0, 0) - np.mean(np.abs(x[0, 0, :4]) ** 2, axis=0)).max() <= F64 * 10
    s.clearNoiseSamples(st); assert s.read(st, 2, 0, 0).tolist() == [0.0, 0.0] and s.read(st, 2, 0, 1).tolist() == [0.0, 1.0]
    s.clear(st); assert s.read(st, 2, 0, 1).tolist() == [0.0, 0.0]
    s.startTraining(); fn = tmp_path / "n.txt"; s.writeNoiseFile(fn, st, 0, 0); est = s.read(st, 0, 0, 0)
    assert open(fn).read() == "".join("%f\n" % v for v in est)
    s2 = dsr.SpectralSubtractor(M); s2.setChannel(-1.0); st2 = s2.newState(2, cuda); s2.readNoiseFile(fn, st2)
    assert not dsr.load().dsr_specsub_is_training(s2.h)                     # readNoiseFile stops training
    assert np.array_equal(s2.read(st2, 0, 1, 0), np.array([float("%f" % v) for v in est]))


@pytest.mark.parametrize("c", K.WIENER_CASES, ids=lambda c: c["name"])
def test_wiener_against_restatement_carried_and_whole(dsr, cuda, c):
    X = K.wiener_input(c); want, fin = K.wiener_reference(c); U = X[0][0].shape[0]; F = c["M"] // 2 + 1
    w = dsr.WienerFilter(c["M"], False, c["alpha"], c["floor"], c["beta"]); w.carry(True); st = w.newState(U, cuda)
    for b in range(3):
        (w.stopUpdatingNoisePSD if b == 1 else w.startUpdatingNoisePSD)()
        got = w.apply(_t(X[b][0], cuda), _t(X[b][1], cuda), st, _nf(c["nframes"][b], cuda)).cpu().numpy()
        assert _out_err(got, want[b], c["nframes"][b], "%s block %d" % (c["name"], b)) <= C64
    for u in range(U):
        for what in (0, 1):
            g = w.read(st, what, u); r = fin[u][what]; assert np.abs(g - r).max() <= F64 * max(np.abs(r).max(), 1e-300), (c["name"], u, what)
        assert w.read(st, 2, u)[0] == fin[u][2]
    # whole run = carried run: utterance 0's frames of the updating blocks in one call, against two calls
    n0, n2 = c["nframes"][0][0], c["nframes"][2][0]
    S = np.concatenate([X[0][0][:1, :n0], X[2][0][:1, :n2]], axis=1); N = np.concatenate([X[0][1][:1, :n0], X[2][1][:1, :n2]], axis=1)
    w.startUpdatingNoisePSD(); w.carry(False); s1 = w.newState(1, cuda); whole = w.apply(_t(S, cuda), _t(N, cuda), s1).cpu().numpy()
    w.carry(True); s2 = w.newState(1, cuda)
    parts = [w.apply(_t(S[:, :n0], cuda), _t(N[:, :n0], cuda), s2).cpu().numpy(), w.apply(_t(S[:, n0:], cuda), _t(N[:, n0:], cuda), s2).cpu().numpy()]
    assert np.array_equal(whole, np.concatenate(parts, axis=1)) and np.array_equal(w.read(s1, 0, 0), w.read(s2, 0, 0))
    # fresh start without carry: the state of the call before does not matter
    w.carry(False); again = w.apply(_t(S, cuda), _t(N, cuda), s2).cpu().numpy(); assert np.array_equal(again, whole)


def test_wiener_refusals_and_upper_half(dsr, cuda):
    w = dsr.WienerFilter(64, True); st = w.newState(1, cuda); X = _t(K.snapshots(3, (1, 2, 33)), cuda)
    with pytest.raises(dsr.DsrError) as e:
        w.apply(X, X, st)
    assert e.value.status == 1                                              # j_error on the first next (spectralsubtraction.cc:334-337)
    w = dsr.WienerFilter(64); st = w.newState(1, cuda)
    full = w.apply(X, X, st, full=True).cpu().numpy(); half = w.apply(X, X, st).cpu().numpy()
    assert np.array_equal(full[:, :, :33], half) and not np.any(full[:, :, 33:])       # bins above M/2 stay zero


@pytest.mark.parametrize("c", K.MASK_CASES, ids=lambda c: c["name"])
def test_masks_against_restatement(dsr, cuda, c):
    X = K.mask_input(c); want, prev = K.mask_reference(c); wantFull, _ = K.mask_reference(c, True); U = X[0][0].shape[0]
    m = dsr.BinaryMask(c["kind"], c["chanX"], c["M"], c["threshold"], c["alpha"], c["dEta"]); m.carry(True); st = m.newState(U, cuda)
    dropped = np.zeros((U, c["M"] // 2 + 1), bool)
    for b in range(2):
        if b == 1 and c["perbin"]:
            m.setThresholds(K.mask_thresholds(c)); m.setThresholds(K.mask_thresholds(c))
        nf = c["nframes"][b]
        r = m.apply(_t(X[b][0], cuda), _t(X[b][1], cuda), st, _nf(nf, cuda), want_mu=True, want_itd=True)
        out, mu, itd = r["out"].cpu().numpy(), r["mu"].cpu().numpy(), r["itd"].cpu().numpy()
        ok = comparable(want[b]["a"], want[b]["b"]); total = 0; left = 0; worst = 0.0
        for u, n in enumerate(nf):
            assert not np.any(out[u, n:]) and not np.any(mu[u, n:]), (c["name"], b, u)
            for t in range(n):
                dropped[u] |= ~ok[u, t]                                      # mu remembers: a bin stays out once a decision was not comparable
                keep = ~dropped[u]; total += keep.size - 1; left += int((~keep[1:]).sum())
                assert np.array_equal(mu[u, t][keep].view(np.uint32), want[b]["mu"][u, t][keep].view(np.uint32)), (c["name"], b, u, t)
                rms = np.sqrt(np.mean(np.abs(want[b]["out"][u, t]) ** 2))
                if rms > 0:
                    worst = max(worst, np.abs(out[u, t] - want[b]["out"][u, t])[keep].max() / rms)
                if c["kind"] == 1:
                    a = want[b]["a"][u, t, 1:]; assert np.abs(itd[u, t, 1:] - a).max() <= F64 * max(a.max(), 1.0), (c["name"], b, u, t)
        assert total == 0 or left <= 0.02 * total, (c["name"], b, left, total)
        full = m_full(dsr, cuda, c, b, X, nf) if b == 0 else None
        if full is not None:
            for u, n in enumerate(nf):
                for t in range(n):
                    rms = np.sqrt(np.mean(np.abs(wantFull[0]["out"][u, t]) ** 2))
                    worst = max(worst, 0.0 if rms == 0 else np.abs(full[u, t] - wantFull[0]["out"][u, t]).max() / rms)
        print("%s block %d: output error %.3g of the frame RMS" % (c["name"], b, worst))
        assert worst <= C64, (c["name"], b, worst)
    for u in range(U):
        keep = ~dropped[u]; assert np.array_equal(m.read(st, u)[keep], prev[u][keep]), (c["name"], u)
    if c["kind"] == 2 and c["perbin"]:
        assert m.getThreshold() == float(np.float32(K.mask_thresholds(c)[-1]))          # the scalar was overwritten bin by bin


def m_full(dsr, cuda, c, b, X, nf):
    """block 0 again from a fresh state with the fftLen-bin row"""
    m = dsr.BinaryMask(c["kind"], c["chanX"], c["M"], c["threshold"], c["alpha"], c["dEta"]); st = m.newState(len(nf), cuda)
    return m.apply(_t(X[b][0], cuda), _t(X[b][1], cuda), st, _nf(nf, cuda), full=True)["out"].cpu().numpy()


def test_mask_state_untouched_without_frames_and_fresh_without_carry(dsr, cuda):
    import torch
    m = dsr.BinaryMask("iid", 0, 64, 0.1, 0.6); st = m.newState(2, cuda); X = _t(K.snapshots(8, (2, 5, 33)), cuda); Y = _t(K.snapshots(9, (2, 5, 33)), cuda)
    assert torch.all(st == 1)
    a = m.apply(X, Y, st, _nf([5, 0], cuda))["out"]; assert torch.all(st[1] == 1) and not torch.all(st[0] == 1)
    b = m.apply(X, Y, st, _nf([5, 0], cuda))["out"]; assert torch.equal(a, b)           # carry off: every call starts from mu = 1
    m.carry(True); c2 = m.apply(X, Y, st, _nf([5, 0], cuda))["out"]; assert not torch.equal(a, c2)
    m.resetState(st); assert torch.all(st == 1)


@pytest.mark.parametrize("c", K.EST_CASES, ids=lambda c: c["name"])
def test_estimators_against_restatement(dsr, cuda, c):
    X = K.est_input(c); ref = K.est_reference(c); U = X[0][0].shape[0]
    e = dsr.ThresholdEstimator(c["kind"], c["M"], c["rng"][0], c["rng"][1], c["rng"][2], c["band"][0], c["band"][1], c["band"][2], c["dEta"], c["pc"])
    st = e.newState(U, cuda)
    for b in range(2):
        e.run(_t(X[b][0], cuda), _t(X[b][1], cuda), st, _nf(c["nframes"][b], cuda))
    for u in range(U):
        got = e.read(st, u); want = ref[u].flat()
        assert got[-1] == want[-1], (c["name"], u, "sample count")
        if want[-1] == 0:
            assert not np.any(got); continue
        bound = K.acc_bound(K.est_terms(c, ref[u]))
        with np.errstate(all="ignore"):
            rel = np.abs(got[:-1] - want[:-1]) / np.abs(want[:-1])
        rel = np.where(want[:-1] == got[:-1], 0.0, rel)
        print("%s u%d: accumulator error %.3g (bound %.3g)" % (c["name"], u, np.nanmax(rel), bound))
        assert np.nanmax(rel) <= bound, (c["name"], u, np.nanmax(rel), bound)
        g = e.calcThreshold(got); th, idx, cost, rho, ths = P.calc_threshold(c["kind"], ref[u].cand, ref[u].nCand, ref[u].F, want)
        assert g["index"] == idx and g["threshold"] == th, (c["name"], u)
        if c["kind"] == 2:
            assert np.array_equal(g["thresholds"], ths), (c["name"], u)


def test_estimator_whole_run_equals_carried_run_and_reset(dsr, cuda):
    import torch
    c = K.EST_CASES[1]; X = K.est_input(c)
    for kind in (0, 1, 2):
        e = dsr.ThresholdEstimator(kind, c["M"], 0.5 if kind == 0 else -2.0, 20.0 if kind == 0 else 2.0, 0.25, dEta=0.05, dPowerCoeff=0.5)
        L = np.concatenate([X[0][0][:1], X[1][0][:1]], axis=1); R = np.concatenate([X[0][1][:1], X[1][1][:1]], axis=1); T = c["T"]
        s1 = e.newState(1, cuda); e.run(_t(L, cuda), _t(R, cuda), s1)
        s2 = e.newState(1, cuda); e.run(_t(L[:, :T], cuda), _t(R[:, :T], cuda), s2); keep = s2.clone()
        e.run(_t(L[:, T:], cuda), _t(R[:, T:], cuda), s2, _nf([0], cuda)); assert torch.equal(keep, s2)       # nframes = 0: untouched
        e.run(_t(L[:, T:], cuda), _t(R[:, T:], cuda), s2)
        a, b = e.read(s1, 0), e.read(s2, 0); n = (c["M"] // 2) * 2 * T
        with np.errstate(all="ignore"):
            rel = np.where(a == b, 0.0, np.abs(a - b) / np.abs(a))
        assert a[-1] == b[-1] == 2 * T and np.nanmax(rel) <= K.acc_bound(n), (kind, np.nanmax(rel))
        assert e.calcThreshold(a)["index"] == e.calcThreshold(b)["index"]
        e.resetState(s2); assert not torch.any(s2)


def test_stream_classes_against_restatement(dsr, cuda):
    """the reference names over the stream protocol: fftLen-bin rows with the upper half as the reference leaves it"""
    from dsr.btk import postfilter as pf
    from dsr.btk.stream import PyVectorComplexFeatureStreamPtr

    class Src:
        def __init__(self, rows):
            self.rows = rows

        def size(self):
            return self.rows.shape[1]

        def reset(self):
            pass

        def __iter__(self):
            return iter(self.rows)

    M, F, T = 64, 33, 6
    half = [K.snapshots(70 + i, (T, F)).astype(np.complex128) for i in range(2)]
    rows = [np.array([P.upper_mirror(r, M) for r in h]) for h in half]
    mk = lambda i: PyVectorComplexFeatureStreamPtr(Src(rows[i]))

    def frames(s):
        return np.array([np.array(v) for v in s])

    def close(got, want):
        rms = np.sqrt(np.mean(np.abs(want) ** 2, axis=1, keepdims=True)); rms[rms == 0] = 1
        err = (np.abs(got - want) / rms).max() if got.shape == want.shape else np.inf
        print("stream classes: output error %.3g of the frame RMS" % err)
        return err <= C64

    ss = pf.SpectralSubtractorPtr(M, False, 1.2, 0.01); ss.setChannel(mk(0)); ss.setChannel(mk(1), 0.7)
    ref = P.SpectralSubtractor(M, 1.2, 0.01); ref.setChannel(-1.0); ref.setChannel(0.7)
    X = np.stack(half)
    assert close(frames(ss), ref.run(X, True))                              # training, not subtracting: the channel average
    ss.stopTraining(); ss.startNoiseSubtraction(); ref.stopTraining(); ref.subtract = True
    assert close(frames(ss), ref.run(X, True))                              # reset() keeps the noise estimates
    wf = pf.WienerFilterPtr(mk(0), mk(1), False, 0.6, 0.001, 2.0); wr = P.WienerFilter(M, 0.6, 0.001, 2.0)
    want = np.zeros((T, M), complex); want[:, :F] = wr.run(half[0], half[1]); assert close(frames(wf), want)
    want[:, :F] = wr.run(half[0], half[1]); assert close(frames(wf), want)  # the frame counter and the PSD memories outlive reset()
    for kind, cls in ((1, pf.KimBinaryMaskFilterPtr), (2, pf.IIDBinaryMaskFilterPtr)):
        mf = cls(1, mk(0), mk(1), M, 0.7, 0.5, 0.05); mr = P.MaskFilter(kind, 1, M, 0.7, 0.5, 0.05)
        assert close(frames(mf), mr.run(half[0], half[1], True)[0]) and close(frames(mf), mr.run(half[0], half[1], True)[0])
    assert not np.any(frames(pf.BinaryMaskFilterPtr(0, mk(0), mk(1), M, 0.5, 0.0)))
    for kind, cls, args in ((0, pf.KimITDThresholdEstimatorPtr, (0.5, 20.0, 0.25, -1, -1, -1, 0.05, 0.5)), (1, pf.IIDThresholdEstimatorPtr, (-2.0, 2.0, 0.25, -1, -1, -1, 0.05, 0.5)),
                            (2, pf.FDIIDThresholdEstimatorPtr, (-2.0, 2.0, 0.25, 0.05, 0.5))):
        est = cls(mk(0), mk(1), M, *args); out = frames(est); assert out.shape == (T, M) and not np.any(out)
        if kind == 2:
            r = P.ThresholdEstimator(2, M, args[0], args[1], args[2], dEta=args[3], dPowerCoeff=args[4]).run(half[0], half[1])
        else:
            r = P.ThresholdEstimator(kind, M, *args).run(half[0], half[1])
        th, idx, cost, rho, ths = P.calc_threshold(kind, r.cand, r.nCand, F, r.flat())
        assert est.calcThreshold() == th
        c1 = np.array(est.getCostFunction(5) if kind == 2 else est.getCostFunction())
        assert np.allclose(c1, cost[5] if kind == 2 else cost, rtol=1e-9, equal_nan=True)
        if kind == 2:
            assert np.array_equal(np.array(est.getThresholds()), ths)
        est.calcThreshold(); c2 = np.array(est.getCostFunction(5) if kind == 2 else est.getCostFunction())
        assert not np.array_equal(c1, c2, equal_nan=True)                   # the second call divides again, as the reference
    ap = pf.averagePSDEstimatorPtr(M // 2, -1.0)
    for r_ in rows[0]:
        ap.addSample(r_)
    assert np.allclose(ap.average(), np.mean(np.abs(half[0]) ** 2, axis=0), rtol=1e-12)
