"""The information-filter echo cancellers on the device (dsr_aec_create_info, kinds "info" and "sqrtinfo" of dsr.Aec, dsr.btk.cancelVP) against
the numpy restatement tests/aec_info_np.py.

Tolerances: those of tests/test_gpu_aec.py.  The output within 2e-6 of the frame's largest bin magnitude (fp32 output rounding is 6e-8, the
rest is room for summation order), every state item within 1e-8 of its largest entry; the played history, the skip counter and the number
of resets exactly.  Carried state is compared bit for bit.  tests/test_aec_info_np_cpu.py shows that no gate decision of the compared
inputs lies within 1e-6 of its threshold and that the plain kind's inversion routes agree to 1e-10, so no frame or bin is left out."""
import numpy as np
import pytest

from tests import aec_info_np as I
from tests import aec_np as N

pytestmark = pytest.mark.gpu
KIND = {I.INFO: "info", I.SQRT_INFO: "sqrtinfo"}
WORST = {}


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _worst(key, e):
    WORST[key] = max(WORST.get(key, 0.0), float(e))


def _check_out(Ed, Er, tag=""):
    """every frame of every utterance: |Ed - Er| <= 2e-6 max_f |Er[frame]|"""
    scale = np.abs(Er).max(axis=-1, keepdims=True)
    err = np.abs(Ed - Er)
    rel = (err / np.maximum(scale, 1e-300)).max() if err.size else 0.0
    _worst(tag.split()[0] + " out", rel)
    print("%s out rel %.2e" % (tag, rel))
    assert np.all(err <= 2e-6 * scale), (tag, rel)


def _items(kind):
    return [("R", 0), ("K", 1), ("sv", 2), ("scal", 5)] + ([("info", 6)] if kind == I.SQRT_INFO else [])


def _check_state(a, st, U, objs, tag=""):
    kind = a.kind; msg = tag
    for name, what in _items(kind):
        d = a.read(st, U, what); r = I.state(objs, U, name)
        e = np.abs(d - r).max() / max(np.abs(r).max(), 1e-300); _worst(tag.split()[0] + " " + name, e); msg += " %s %.2e" % (name, e)
        assert e <= 1e-8, msg
    assert np.array_equal(a.read(st, U, a.HISTORY), I.state(objs, U, "hist")), tag       # scaled inputs: exact
    if kind == I.INFO:
        assert list(a.read(st, U, a.SKIPPED)) == [o.skipped for o in objs], tag
        assert list(a.read(st, U, a.RESETS)) == [o.resets for o in objs], tag
        msg += " resets %s" % [o.resets for o in objs]
    else:
        assert not np.triu(a.read(st, U, a.K), 1).any(), tag                             # the inverse Cholesky factor: lower triangular
    print(msg)


def _run(dsr, cuda, kind, M, L, V, A, nf, params, frame0=0, mode=0):
    import torch
    a = dsr.Aec(KIND[kind], M, L, frameMode=mode, **params)
    U = V.shape[0]; st = a.newState(U, cuda)
    E = a.apply(_t(V, cuda), _t(A, cuda), _t(np.asarray(nf, np.int32), cuda), st, frame0)
    torch.cuda.synchronize()
    return a, st, E.cpu().numpy()


@pytest.mark.parametrize("M,L,mode,seed", I.INFO_CASES)
@pytest.mark.parametrize("kind", [I.INFO, I.SQRT_INFO])
def test_matches_restatement(dsr, cuda, kind, M, L, mode, seed):
    V, A, nf, Er, objs = I.reference(kind, M, L, mode, seed)
    a, st, Ed = _run(dsr, cuda, kind, M, L, V, A, nf, {}, mode=mode)
    tag = "%s M=%d L=%d mode=%d" % (KIND[kind], M, L, mode)
    for u in range(3):
        assert np.all(Ed[u, nf[u]:] == 0), tag                                       # frames from nframes[u] on are written as zero
    _check_out(Ed, Er, tag); _check_state(a, st, 3, objs, tag)


@pytest.mark.parametrize("L", [1, 3, 32])
@pytest.mark.parametrize("kind", [I.INFO, I.SQRT_INFO])
def test_carried_state_is_bit_identical(dsr, cuda, kind, L):
    import torch
    M, U, T = 64, 3, 130
    V, A, _ = I.info_inputs(M, L, 500 + L, T=T)
    nf = np.array([T, 87, 1], np.int32)
    a, st0, E0 = _run(dsr, cuda, kind, M, L, V, A, nf, {})
    whats = [0, 1, 2, 4, 5] + ([6] if kind == I.SQRT_INFO else [7, 8])
    parts = [a.read(st0, U, w) for w in whats]
    assert np.abs(parts[0][0] - parts[0][2]).max() > 0                                # the filters moved
    Vd, Ad = _t(V, cuda), _t(A, cuda)
    for blk in (1, 7, 100):
        st = a.newState(U, cuda); E = np.zeros_like(E0)
        for t0 in range(0, T, blk):
            t1 = min(T, t0 + blk)
            n = torch.from_numpy(np.clip(nf - t0, 0, t1 - t0).astype(np.int32)).to(cuda)
            E[:, t0:t1] = a.apply(Vd[:, t0:t1].contiguous(), Ad[:, t0:t1].contiguous(), n, st, frame0=t0).cpu().numpy()
        assert np.array_equal(E.view(np.float32), E0.view(np.float32)), blk
        for w, p in zip(whats, parts):
            assert np.array_equal(a.read(st, U, w).view(np.float64), p.view(np.float64)), (blk, w)


@pytest.mark.parametrize("kind", [I.INFO, I.SQRT_INFO])
def test_amp4play_quiet_stretches_and_a_silent_frame(dsr, cuda, kind):
    """quiet stretches close the |v0|^2 gate (the plain kind counts them towards its reset rule); one frame of digital silence in both
    streams, two frames after another so that the history is all zero: the plain kind's residual is exactly 0 there and leaves as NaN"""
    M, L, T = 64, 2, 180; F = 33
    VA = [N.echo_case(T, F, L, 900 + u, switch=(0.5, 12.0, 30), quiet=[(110, 118)])[:2] for u in range(3)]
    V = np.stack([v for v, _ in VA]); A = np.stack([x for _, x in VA]); nf = [T, 120, 1]
    V[0, 140:142] = 0; A[0, 141] = 0
    params = dict(amp4play=0.6, snrTh=1.5, engTh=50.0, smooth=0.8, loading=0.02, beta=0.9, sigmau2=5e-3)
    with np.errstate(all="ignore"):
        Er, objs = I.run_batch(kind, M, L, V, A, nf, 37, 0, **params)
    assert min(min(o.margin.values()) for o in objs) >= 1e-6
    a, st, Ed = _run(dsr, cuda, kind, M, L, V, A, nf, params, frame0=37)
    nan = np.isnan(Er)
    if kind == I.INFO:
        assert nan[0, 141].all() and nan.sum() == F and objs[0].decisions["v0"][0] >= 10 * F and sum(o.resets for o in objs) > 0
    else:
        assert not nan.any() and not Er[0, 141].any()
    assert np.array_equal(np.isnan(Ed), nan)
    _check_out(np.where(nan, 0, Ed), np.where(nan, 0, Er), KIND[kind] + " amp"); _check_state(a, st, 3, objs, KIND[kind] + " amp")
    # the silent frame left the state as it was: run up to it, read, run it, read
    b = dsr.Aec(KIND[kind], M, L, **params); sb = b.newState(1, cuda)
    b.apply(_t(V[:1, :141], cuda), _t(A[:1, :141], cuda), None, sb, 37)
    whats = [0, 1, 2, 5] + ([6] if kind == I.SQRT_INFO else [])
    before = [b.read(sb, 1, w) for w in whats]
    resets = b.read(sb, 1, b.RESETS)[0] if kind == I.INFO else 0
    b.apply(_t(V[:1, 141:142], cuda), _t(A[:1, 141:142], cuda), None, sb, 37 + 141)
    for w, p in zip(whats, before):
        now = b.read(sb, 1, w)
        if kind == I.INFO and w == 0:                                               # the F skips count towards the reset rule: a reset bin is (1, 0), the others are as they were
            moved = np.any(now.view(np.float64) != p.view(np.float64), axis=-1)[0]
            assert moved.sum() == b.read(sb, 1, b.RESETS)[0] - resets and 1 <= moved.sum() <= 2 and np.array_equal(now[0][moved], np.tile([1.0, 0.0], (moved.sum(), 1)))
            continue
        assert np.array_equal(now.view(np.float64), p.view(np.float64)), w


@pytest.mark.parametrize("kind", [I.INFO, I.SQRT_INFO])
def test_more_chains_than_the_device_holds(dsr, cuda, kind):
    """U = 600, M = 64, L = 1, T = 8: 19800 chains (the square-root kind packs 32 a wave: 619 workgroups), 600 workgroups of the plain kind"""
    M, L, U0, reps, T = 64, 1, 40, 15, 8
    VA = [N.echo_case(T, 33, L, 7700 + u, quiet=((5, 6),))[:2] for u in range(U0)]
    V0 = np.stack([v for v, _ in VA]); A0 = np.stack([x for _, x in VA]); nf0 = np.full(U0, T, np.int32); nf0[::7] = 5
    V = np.tile(V0, (reps, 1, 1)); A = np.tile(A0, (reps, 1, 1)); nf = np.tile(nf0, reps)
    a, st, Ed = _run(dsr, cuda, kind, M, L, V, A, nf, {})
    Er, objs = I.run_batch(kind, M, L, V0, A0, nf0)
    tag = KIND[kind] + " U=600"
    _check_out(Ed[:U0], Er, tag)
    assert np.array_equal(Ed.reshape(reps, U0, T, 33), np.broadcast_to(Ed[:U0], (reps, U0, T, 33)))
    for name, what in _items(kind):
        d = a.read(st, U0 * reps, what); r = I.state(objs, U0, name)
        assert np.array_equal(d.reshape((reps,) + r.shape), np.broadcast_to(d[:U0], (reps,) + r.shape)), name
        assert np.abs(d[:U0] - r).max() <= 1e-8 * np.abs(r).max(), name


def test_zero_norm_is_reported(dsr, cuda):
    """sigmau2 = inf makes Sigma_u = K = 0: the first rotation has norm zero, the reference's jarithmetic_error"""
    V, A, _ = N.echo_case(4, 33, 2, seed=3)
    a = dsr.Aec("sqrtinfo", 64, 2, sigmau2=float("inf")); st = a.newState(1, cuda)
    with pytest.raises(dsr.DsrError) as e:
        a.apply(_t(V[None], cuda), _t(A[None], cuda), None, st)
    assert e.value.status == 3 and "Norm is zero" in str(e.value)                     # DSR_E_ARITHMETIC
    with pytest.raises(ArithmeticError):
        I.InfoAec(I.SQRT_INFO, 64, 2, sigmau2=float("inf")).run(V, A)


def test_state_parts_of_another_kind_are_refused(dsr, cuda):
    a = dsr.Aec("info", 64, 2); b = dsr.Aec("sqrtinfo", 64, 2); sa = a.newState(1, cuda); sb = b.newState(1, cuda)
    for x, s, what in ((a, sa, a.INFO), (a, sa, a.DTD), (b, sb, b.SKIPPED), (b, sb, b.RESETS), (b, sb, b.DTD)):
        with pytest.raises(dsr.DsrError) as e:
            x.read(s, 1, what)
        assert e.value.status == 13
    assert np.array_equal(a.read(sa, 1, a.FILTER)[0], np.tile([1.0, 0.0], (33, 1)))    # R = (1, 0) at the start
    assert np.array_equal(b.read(sb, 1, b.K)[0], np.tile(np.eye(2) / np.sqrt(10e-4), (33, 1, 1)))


class _Src:
    def __init__(self, frames):
        self.frames = frames

    def size(self):
        return self.frames.shape[1]

    def reset(self):
        pass

    def __iter__(self):
        return iter(self.frames)


@pytest.mark.parametrize("name,kind", [("InformationFilterEchoCancellationFeaturePtr", I.INFO), ("SquareRootInformationFilterEchoCancellationFeaturePtr", I.SQRT_INFO)])
def test_python_classes(dsr, cuda, name, kind):
    from dsr.btk import cancelVP
    from dsr.btk.stream import PyVectorComplexFeatureStreamPtr
    M, T, L = 64, 130, 4
    Vh, Ah, _ = I.info_inputs(M, L, 700, T=T); Vh, Ah = Vh[0], Ah[0]
    ref = I.InfoAec(kind, M, L)
    Ah = Ah[:T - 9]                                                                 # the recorded stream ends first: so does the canceller
    played = PyVectorComplexFeatureStreamPtr(_Src(ref.full(Vh.astype(np.complex128))))
    recorded = PyVectorComplexFeatureStreamPtr(_Src(ref.full(Ah.astype(np.complex128))))
    aec = getattr(cancelVP, name)(played, recorded, sampleN=L)
    assert aec.size() == M
    mode = 1                                                                        # `for x in aec` calls next() with the default -5
    p1 = np.stack([np.array(x) for x in aec])
    p2 = np.stack([np.array(x) for x in aec])
    assert p1.shape == (T - 9, M) and aec.isEnd()
    r1 = ref.run(Vh[:T - 9], Ah, 0, mode); ref.reset(); r2 = ref.run(Vh[:T - 9], Ah, 0, mode)      # reset() resets nothing: one run over both
    _check_out(p1[:, :33], r1, name + " pass 1"); _check_out(p2[:, :33], r2, name + " pass 2")
    for p in (p1, p2):                                                              # all M bins: bin M - k = conj(bin k)
        assert np.array_equal(p[:, 33:], np.conj(p[:, 1:32][:, ::-1]))
    assert np.abs(p1 - p2).max() > 50 * 2e-6 * np.abs(p1).max()                     # the state lives on: far outside the tolerance
    e = np.abs(aec.filterCoefficients() - ref.R).max() / np.abs(ref.R).max()
    assert e <= 1e-8, e
    e = np.abs(aec.bandScalars() - ref.scal).max() / np.abs(ref.scal).max()
    assert e <= 1e-8, e
    if kind == I.INFO:
        assert aec.skippedN() == (ref.skipped, ref.resets)
    else:
        assert np.abs(aec.informationState() - ref.info).max() <= 1e-8 * np.abs(ref.info).max()
        assert np.abs(aec.covariance() - ref.K).max() <= 1e-8 * np.abs(ref.K).max()
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
    rng = np.random.default_rng(5); n = 300 * D
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
    aec = cancelVP.SquareRootInformationFilterEchoCancellationFeaturePtr(pa, ra, sampleN=L)
    syn = OverSampledDFTSynthesisBankPtr(aec, g, M, m, r)
    y = np.concatenate([np.array(x) for x in syn])
    assert np.isfinite(y).all() and y.size > n // 2
    aec2 = cancelVP.SquareRootInformationFilterEchoCancellationFeaturePtr(pa, ra, sampleN=L)
    E = np.stack([np.array(x) for x in aec2])
    F = M // 2 + 1
    ref = I.InfoAec(I.SQRT_INFO, M, L); Er = ref.run(P[:, :F], R[:, :F], 0, 1)
    _check_out(E[:, :F], Er, "end to end")
    erle = N.erle_db(R[:, 1:F - 1], E[:, 1:F - 1], last=100)
    print("end to end ERLE %.1f dB" % erle)
    # what is compared is the restatement, above.  The bar here only says that it is a canceller at all: with the echo 48 dB above the near-end
    # noise, a residual that keeps more than half of the recorded power would mean that nothing was cancelled.
    assert erle >= 3.0


def test_zz_report_worst_errors():
    print("worst errors seen: " + ", ".join("%s %.2e" % kv for kv in sorted(WORST.items())))
