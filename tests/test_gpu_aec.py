"""The echo cancellers on the device (dsr_aec_*, dsr.btk.cancelVP) against the numpy restatement tests/aec_np.py.

Tolerances (the project's standing ones for an fp64 recursion with complex64 output): the output within 2e-6 of the
frame's largest bin magnitude (fp32 output rounding is 6e-8; the rest is room for summation order), the final filter coefficients, the
covariances and the noise variances within 1e-8 of their largest entry.  Carried state is compared bit for bit."""
import numpy as np
import pytest

from tests import aec_np as N

pytestmark = pytest.mark.gpu
KIND = {N.NLMS: "nlms", N.KALMAN: "kalman", N.BLOCK: "block", N.DTD: "dtd"}
WORST = {"out": 0.0, "R": 0.0, "K": 0.0, "sv": 0.0}


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _check_out(Ed, Er, tag=""):
    """every frame of every utterance: |Ed - Er| <= 2e-6 max_f |Er[frame]|"""
    scale = np.abs(Er).max(axis=-1, keepdims=True)
    err = np.abs(Ed - Er)
    rel = (err / np.maximum(scale, 1e-300)).max() if err.size else 0.0
    WORST["out"] = max(WORST["out"], rel)
    print("%s out rel %.2e" % (tag, rel))
    assert np.all(err <= 2e-6 * scale), (tag, rel)


def _check_state(a, st, U, objs, tag=""):
    R = a.read(st, U, a.FILTER); Rr = np.stack([o.R for o in objs])
    e = np.abs(R - Rr).max() / max(np.abs(Rr).max(), 1e-300); WORST["R"] = max(WORST["R"], e)
    msg = "%s R %.2e" % (tag, e)
    assert e <= 1e-8, msg
    if a.kind != 0:
        Kd = a.read(st, U, a.K); Kr = np.stack([o.K for o in objs])
        e = np.abs(Kd - Kr).max() / np.abs(Kr).max(); WORST["K"] = max(WORST["K"], e); msg += " K %.2e" % e
        assert e <= 1e-8, msg
        sd = a.read(st, U, a.SIGMA2V); sr = np.stack([o.sv for o in objs])
        e = np.abs(sd - sr).max() / np.abs(sr).max(); WORST["sv"] = max(WORST["sv"], e); msg += " sv %.2e" % e
        assert e <= 1e-8, msg
    if a.kind >= 2:
        Hd = a.read(st, U, a.HISTORY); Hr = np.stack([o.hist for o in objs])
        assert np.array_equal(Hd, Hr), tag                                          # scaled inputs: exact
    if a.kind == 3:
        dd = a.read(st, U, a.DTD); dr = np.stack([o.dtd for o in objs])
        assert np.all(np.abs(dd - dr) <= 1e-8 * np.abs(dr).max()), (tag, dd, dr)
    print(msg)


def _inputs(U, T, F, L, seed, quiet=((20, 27), (60, 61))):
    VA = [N.echo_case(T, F, L, seed * 10 + u, quiet=quiet)[:2] for u in range(U)]
    return np.stack([v for v, _ in VA]), np.stack([a for _, a in VA])


def _run(dsr, cuda, kind, M, L, V, A, nf, params, frame0=0, mode=0):
    import torch
    a = dsr.Aec(KIND[kind], M, L, frameMode=mode, **params)
    U = V.shape[0]; st = a.newState(U, cuda)
    E = a.apply(_t(V, cuda), _t(A, cuda), _t(np.asarray(nf, np.int32), cuda), st, frame0)
    torch.cuda.synchronize()
    return a, st, E.cpu().numpy()


CASES = ([(N.NLMS, M, 1, {}) for M in (64, 256, 512)] + [(N.KALMAN, M, 1, {}) for M in (64, 256, 512)] +
         [(N.KALMAN, 64, 1, dict(beta=0.8, sigma2=2.0, threshold=400.0)), (N.NLMS, 64, 1, dict(delta=10.0, epsilon=1e-2, threshold=900.0))] +
         [(N.BLOCK, 64, L, {}) for L in (1, 2, 3, 4, 8, 16, 32)] +
         [(N.BLOCK, 64, L, dict(amp4play=0.37, beta=0.9, sigmau2=5e-3, sigmak2=2.0, threshold=30.0)) for L in (1, 3, 8, 32)] +
         [(N.BLOCK, 256, 4, {}), (N.BLOCK, 256, 32, dict(amp4play=1.7)), (N.BLOCK, 512, 1, {}), (N.BLOCK, 512, 16, {}), (N.BLOCK, 96, 5, {})])


@pytest.mark.parametrize("kind,M,L,params", CASES)
def test_matches_restatement(dsr, cuda, kind, M, L, params):
    U, T, F = 3, 150, M // 2 + 1
    nf = [T, (2 * T) // 3, 1]
    V, A = _inputs(U, T, F, L, seed=kind * 1000 + M + L)
    a, st, Ed = _run(dsr, cuda, kind, M, L, V, A, nf, params)
    Er, objs = N.run_batch(lambda: N.Aec(kind, M, L, **params), V, A, nf)
    tag = "%s M=%d L=%d" % (KIND[kind], M, L)
    for u in range(U):
        assert np.all(Ed[u, nf[u]:] == 0), tag                                      # frames from nframes[u] on are written as zero
    _check_out(Ed, Er, tag); _check_state(a, st, U, objs, tag)
    if kind == N.BLOCK:                                                             # the planted quiet stretch is below the gate and above it elsewhere
        amp = params.get("amp4play", 1.0); thr = params.get("threshold", 100.0)
        p2 = np.abs(V[0].astype(np.complex128) * amp) ** 2
        assert (p2[20:27] < thr).all() and (p2[:20] > thr).mean() > 0.5


@pytest.mark.parametrize("M,L,mode,seed", N.DTD_CASES)
def test_dtd_matches_restatement(dsr, cuda, M, L, mode, seed):
    """no frame or bin is left out: tests/test_aec_np_cpu.py shows that no gate decision of these inputs lies within 1e-6 of its threshold"""
    V, A, nf = N.dtd_inputs(M, L, seed)
    a, st, Ed = _run(dsr, cuda, N.DTD, M, L, V, A, nf, {}, mode=mode)
    Er, objs = N.run_batch(lambda: N.Aec(N.DTD, M, L), V, A, nf, 0, mode)
    tag = "dtd M=%d L=%d mode=%d" % (M, L, mode)
    _check_out(Ed, Er, tag); _check_state(a, st, 3, objs, tag)


def test_dtd_with_amp4play_and_quiet_stretches(dsr, cuda):
    M, L = 64, 4; T = 180
    VA = [N.echo_case(T, M // 2 + 1, L, 900 + u, switch=(0.5, 12.0, 30), quiet=[(110, 118)])[:2] for u in range(3)]
    V = np.stack([v for v, _ in VA]); A = np.stack([x for _, x in VA]); nf = [T, 120, 1]
    params = dict(amp4play=0.6, snrTh=1.5, engTh=50.0, smooth=0.8)
    a, st, Ed = _run(dsr, cuda, N.DTD, M, L, V, A, nf, params, frame0=37)
    objs = [N.Aec(N.DTD, M, L, **params) for _ in range(3)]
    Er = np.zeros(V.shape, np.complex128)
    for u in range(3):
        Er[u, :nf[u]] = objs[u].run(V[u, :nf[u]], A[u, :nf[u]], frame0=37)
    assert min(o.margin for o in objs) >= 1e-6
    _check_out(Ed, Er, "dtd amp"); _check_state(a, st, 3, objs, "dtd amp")


def test_first_unsupported_sample_n(dsr):
    with pytest.raises(dsr.DsrError) as e:
        dsr.Aec("block", 64, 33)
    assert e.value.status == 13 and "sampleN" in str(e.value)                        # DSR_E_PARAMETER, as include/dsr.h documents
    with pytest.raises(dsr.DsrError):
        dsr.Aec("dtd", 64, 33)


def test_more_chains_than_the_device_holds(dsr, cuda):
    """block L = 32: one wave per chain, 160 x 33 = 5280 waves against 2048 resident (256 CUs x 4 SIMDs x 2); Kalman / NLMS: 20000 x 33 threads"""
    M, L, U, T = 64, 32, 160, 24
    V, A = _inputs(U, T, 33, L, seed=77, quiet=((5, 7),))
    nf = np.full(U, T, np.int32); nf[::7] = 11
    a, st, Ed = _run(dsr, cuda, N.BLOCK, M, L, V, A, nf, {})
    Er, objs = N.run_batch(lambda: N.Aec(N.BLOCK, M, L), V, A, nf)
    _check_out(Ed, Er, "block U=160"); _check_state(a, st, U, objs, "block U=160")
    for kind in (N.NLMS, N.KALMAN):
        V8, A8 = _inputs(8, 40, 33, 1, seed=78)
        reps = 2500; Vb = np.tile(V8, (reps, 1, 1)); Ab = np.tile(A8, (reps, 1, 1)); nfb = np.full(8 * reps, 40, np.int32)
        a, st, Ed = _run(dsr, cuda, kind, M, 1, Vb, Ab, nfb, {})
        Er, objs = N.run_batch(lambda: N.Aec(kind, M), V8, A8, nfb[:8])
        _check_out(Ed[:8], Er, KIND[kind] + " U=20000")
        assert np.array_equal(Ed.reshape(reps, 8, 40, 33), np.broadcast_to(Ed[:8], (reps, 8, 40, 33)))
        R = a.read(st, 8 * reps, a.FILTER)
        assert np.array_equal(R.reshape(reps, 8, 33, 1), np.broadcast_to(R[:8], (reps, 8, 33, 1)))
        assert np.abs(R[:8] - np.stack([o.R for o in objs])).max() <= 1e-8 * np.abs(R[:8]).max()


@pytest.mark.parametrize("kind,L", [(N.NLMS, 1), (N.KALMAN, 1), (N.BLOCK, 1), (N.BLOCK, 3), (N.BLOCK, 16), (N.BLOCK, 32), (N.DTD, 1), (N.DTD, 4), (N.DTD, 32)])
def test_carried_state_is_bit_identical(dsr, cuda, kind, L):
    import torch
    M, U, T = 64, 3, 230; F = 33
    if kind == N.DTD:
        V, A, _ = N.dtd_inputs(M, L, 500 + L, T=T)
    else:
        V, A = _inputs(U, T, F, L, seed=300 + kind * 40 + L)
    nf = np.array([T, 153, 1], np.int32)
    a, st0, E0 = _run(dsr, cuda, kind, M, L, V, A, nf, {})
    parts = [a.read(st0, U, w) for w in ([0, 4] if kind == 0 else [0, 1, 2, 4] + ([3] if kind == 3 else []))]
    Vd, Ad = _t(V, cuda), _t(A, cuda)
    for blk in (1, 7, 100):
        st = a.newState(U, cuda); E = np.zeros_like(E0)
        for t0 in range(0, T, blk):
            t1 = min(T, t0 + blk)
            n = torch.from_numpy(np.clip(nf - t0, 0, t1 - t0).astype(np.int32)).to(cuda)
            E[:, t0:t1] = a.apply(Vd[:, t0:t1].contiguous(), Ad[:, t0:t1].contiguous(), n, st, frame0=t0).cpu().numpy()
        assert np.array_equal(E.view(np.float32), E0.view(np.float32)), blk
        for w, p in zip(([0, 4] if kind == 0 else [0, 1, 2, 4] + ([3] if kind == 3 else [])), parts):
            assert np.array_equal(a.read(st, U, w).view(np.float64), p.view(np.float64)), (blk, w)


def test_null_state_is_a_fresh_state_and_reset_filter(dsr, cuda):
    import torch
    M, T = 64, 90
    for kind, L in [(N.NLMS, 1), (N.KALMAN, 1), (N.BLOCK, 4), (N.DTD, 4)]:
        V, A = _inputs(2, T, 33, L, seed=600 + kind)
        a = dsr.Aec(KIND[kind], M, L); st = a.newState(2, cuda)
        E1 = a.apply(_t(V, cuda), _t(A, cuda), None, st).cpu().numpy()
        E2 = a.apply(_t(V, cuda), _t(A, cuda), None, None).cpu().numpy()
        assert np.array_equal(E1.view(np.float32), E2.view(np.float32)), kind
        # reset(): NLMS / Kalman zero the coefficients and keep sigma2_v, K; the block variants keep everything
        before = [a.read(st, 2, w) for w in ((0,) if kind == 0 else (0, 1, 2))]
        a.resetFilter(st, 2); torch.cuda.synchronize()
        after = [a.read(st, 2, w) for w in ((0,) if kind == 0 else (0, 1, 2))]
        if kind in (N.NLMS, N.KALMAN):
            assert np.abs(before[0]).max() > 0 and not after[0].any()
        else:
            assert np.array_equal(before[0], after[0])
        for b, c in zip(before[1:], after[1:]):
            assert np.array_equal(b, c)
        # the second utterance continues from there, as the restatement's object does
        o = [N.Aec(kind, M, L) for _ in range(2)]
        for u in range(2):
            o[u].run(V[u], A[u]); o[u].reset()
        E3 = a.apply(_t(V, cuda), _t(A, cuda), None, st).cpu().numpy()
        Er = np.stack([o[u].run(V[u], A[u]) for u in range(2)])
        _check_out(E3, Er, "second pass %s" % KIND[kind]); _check_state(a, st, 2, o, "second pass %s" % KIND[kind])


class _Src:
    def __init__(self, frames):
        self.frames = frames

    def size(self):
        return self.frames.shape[1]

    def reset(self):
        pass

    def __iter__(self):
        return iter(self.frames)


@pytest.mark.parametrize("name,kind,kw", [("NLMSAcousticEchoCancellationFeaturePtr", N.NLMS, {}), ("KalmanFilterEchoCancellationFeaturePtr", N.KALMAN, {}),
                                          ("BlockKalmanFilterEchoCancellationFeaturePtr", N.BLOCK, dict(sampleN=4)),
                                          ("DTDBlockKalmanFilterEchoCancellationFeaturePtr", N.DTD, dict(sampleN=4))])
def test_python_classes(dsr, cuda, name, kind, kw):
    from dsr.btk import cancelVP
    from dsr.btk.stream import PyVectorComplexFeatureStreamPtr
    M, T = 64, 130; L = kw.get("sampleN", 1)
    if kind == N.DTD:
        Vh, Ah, _ = N.dtd_inputs(M, L, 700, T=T); Vh, Ah = Vh[0], Ah[0]
    else:
        Vh, Ah, _ = N.echo_case(T, 33, L, seed=701, quiet=[(30, 35)])
    ref = N.Aec(kind, M, L)
    Ah = Ah[:T - 9]                                                                 # the recorded stream ends first: so does the canceller
    played = PyVectorComplexFeatureStreamPtr(_Src(ref.full(Vh.astype(np.complex128))))
    recorded = PyVectorComplexFeatureStreamPtr(_Src(ref.full(Ah.astype(np.complex128))))
    aec = getattr(cancelVP, name)(played, recorded, **kw)
    assert aec.size() == M
    mode = 1                                                                        # `for x in aec` calls next() with the default -5
    p1 = np.stack([np.array(x) for x in aec])
    p2 = np.stack([np.array(x) for x in aec])
    assert p1.shape == (T - 9, M) and aec.isEnd()
    r1 = ref.run(Vh[:T - 9], Ah, 0, mode); ref.reset(); r2 = ref.run(Vh[:T - 9], Ah, 0, mode)
    _check_out(p1[:, :33], r1, name + " pass 1"); _check_out(p2[:, :33], r2, name + " pass 2")
    for p in (p1, p2):                                                              # all M bins: bin M - k = conj(bin k)
        assert np.array_equal(p[:, 33:], np.conj(p[:, 1:32][:, ::-1]))
    if kind == N.NLMS:
        assert np.array_equal(p1, p2)                                               # reset() zeroes all the state NLMS has
    else:
        assert np.abs(p1 - p2).max() > 50 * 2e-6 * np.abs(p1).max()                 # the covariances (and, block, the filter) live on: far outside the tolerance
    e = np.abs(aec.filterCoefficients() - ref.R).max() / np.abs(ref.R).max()
    assert e <= 1e-8, e
    # explicit frame indices: a repeated one returns the cached vector, a skipped one is an index error
    aec.reset()
    a0 = np.array(aec.next(0)); a1 = np.array(aec.next(1)); a1b = np.array(aec.next(1))
    assert np.array_equal(a1, a1b) and aec.frameX() == 1 and not np.array_equal(a0, a1)
    with pytest.raises(dsr.DsrError) as ex:
        aec.next(5)
    assert ex.value.status == 6                                                     # jindex_error


def test_end_to_end_through_the_filter_banks(dsr, cuda, protos):
    from dsr.btk import cancelVP
    from dsr.btk.feature import SampleFeaturePtr
    from dsr.btk.modulated import OverSampledDFTAnalysisBankPtr, OverSampledDFTSynthesisBankPtr
    M, m, r, h, g = protos["M256-m4-r1"]; D = M >> r; L = 8
    rng = np.random.default_rng(5); n = 400 * D
    play = (3000.0 * rng.standard_normal(n)).astype(np.float32)
    room = 0.5 * np.exp(-np.arange(6 * D) / (1.5 * D)) * rng.standard_normal(6 * D)
    echo = np.convolve(play, room)[:n]
    near = 60.0 * rng.standard_normal(n)
    rec = (echo + near).astype(np.float32)

    def bank(x):
        s = SampleFeaturePtr(blockLen=D, shiftLen=D, padZeros=True); s.setSamples(x, 16000)
        return OverSampledDFTAnalysisBankPtr(s, h, M, m, r)
    pa, ra = bank(play), bank(rec)
    P = np.stack([np.array(x) for x in pa]); R = np.stack([np.array(x) for x in ra])
    aec = cancelVP.BlockKalmanFilterEchoCancellationFeaturePtr(pa, ra, sampleN=L)
    syn = OverSampledDFTSynthesisBankPtr(aec, g, M, m, r)
    y = np.concatenate([np.array(x) for x in syn])
    assert np.isfinite(y).all() and y.size > n // 2
    aec2 = cancelVP.BlockKalmanFilterEchoCancellationFeaturePtr(pa, ra, sampleN=L)
    E = np.stack([np.array(x) for x in aec2])
    F = M // 2 + 1
    ref = N.Aec(N.BLOCK, M, L); Er = ref.run(P[:, :F], R[:, :F])
    _check_out(E[:, :F], Er, "end to end")
    erle = N.erle_db(R[:, 1:F - 1], E[:, 1:F - 1])
    print("end to end ERLE %.1f dB" % erle)
    assert erle >= 15.0


def test_zz_report_worst_errors():
    print("worst errors seen: " + ", ".join("%s %.2e" % kv for kv in WORST.items()))
