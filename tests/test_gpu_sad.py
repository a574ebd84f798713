"""GPU tests of speech activity detection (include/dsr.h section 7b, csrc/k_sad.hip) against the numpy restatement of tests/sad_np.py on the
cases of tests/sad_cases.py.

Compared on bits (0 elements differ, a NaN equals a NaN): the energies, decisions and the whole carried state of EnergyVADMetric and
SimpleEnergyVAD; the per-channel powers, the decisions and the PowerSpectrumVADMetric score; start / length / consumed / decisionMetric of the
three segmenters and the gathered frames; BandEnergyRatio and SignificantSubbands.  EnergyDiffusion and NegativeEntropy (fp64 log on the device,
float output): 0 or 1 unit in the last place, the count of 1-ulp elements is printed.  NormalizedEnergyMetric and TSPS scores (sqrt / log on the device): relative 1e-12.  CCC scores:
absolute 1e-12 (a PHAT correlation is bounded by 1).  Negentropy, mutual-information and likelihood-ratio scores and the rho state: 1e-12 x the
restatement's sum of absolute per-bin terms / binN (rho: 1e-12, |rho| <= 0.9).  A decision of a toleranced metric must be equal wherever the restatement's score is
farther from its threshold than that tolerance; at most 2 % of a case's frames may be left out (tests/test_sad_np_cpu.py holds the cases to
that with a second evaluation order)."""
import numpy as np
import pytest

from tests import sad_cases as Cs
from tests import sad_np as R

pytestmark = pytest.mark.gpu


class Frames:
    """a Python iterable with size()/reset(), as the PyVector*FeatureStreamPtr classes take it; every reset() moves on to the next utterance"""

    def __init__(self, *utts): self.utts, self.i = utts, 0
    def size(self): return self.utts[0].shape[1]
    def reset(self): self.i = min(self.i + 1, len(self.utts) - 1)
    def __iter__(self): return iter(self.utts[self.i])


def _dev(a, cuda):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to(cuda)                 # a copy: the shared cases are read-only


def _same(tag, got, ref):
    got = np.asarray(got); ref = np.asarray(ref)
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    nd = R.differing(got, ref)
    print("%s: %d of %d elements differ in bits" % (tag, nd, ref.size))
    assert nd == 0, (tag, nd)


def _values(metric):
    """(decision, score) of every frame a metric serves until end of samples"""
    dec, score = [], []
    while True:
        try:
            dec.append(metric.next()); score.append(metric.score())
        except StopIteration:
            return np.array(dec, np.float64), np.array(score, np.float64)


def _rows(stream):
    rows = []
    while True:
        try:
            rows.append(np.array(stream.next(), copy=True))
        except StopIteration:
            return rows


# ---------------------------------------------------------------- EnergyVADMetric
@pytest.mark.parametrize("cfg", Cs.ENERGY_CONFIGS, ids=str)
def test_energy_metric_configs(dsr, cuda, cfg):
    N, blockLen, headN, tailN, thr = cfg
    dec, score, hist, cnt, updates, seg = Cs.energy_reference(cfg)
    x = Cs.energy_blocks(blockLen)
    gd, gs, (gh, gc), gu = dsr.sad_energy(_dev(x[None], cuda), thr, headN, tailN, initialEnergy=Cs.ENERGY_INITIAL, energiesN=N, return_updates=True)
    _same("energy %s score" % (cfg,), gs.cpu().numpy()[0], score)
    _same("energy %s decision" % (cfg,), gd.cpu().numpy()[0], dec)
    _same("energy %s history" % (cfg,), gh.cpu().numpy()[0], hist)
    _same("energy %s counters" % (cfg,), gc.cpu().numpy()[0], cnt)
    assert int(gu.cpu()[0]) == updates
    m = R.EnergyVADMetric(Cs.ENERGY_INITIAL, thr, headN, tailN, N); m.hist = np.array(hist)
    for pct in (0.0, 50.0, 99.0):
        assert dsr.sad_energy_percentile((gh, gc), pct) == m.energyPercentile(pct)
    # the hangover walk over the metric's own decisions: the segment tests/test_sad_np_cpu.py pins
    st, ln, cons, _ = dsr.sad_hangover(gd[None].contiguous(), (0.5,), headN, tailN)
    assert (int(st.cpu()[0]), int(st.cpu()[0]) + int(ln.cpu()[0])) == seg


def test_energy_ragged_batch_two_calls_and_next_speaker(dsr, cuda):
    import torch
    N, headN, tailN, thr, T = 65, 1, 10, 0.31, 300
    x = Cs.energy_blocks(160)
    rng = np.random.default_rng(5)
    xb = (rng.standard_normal((3, T, 160)) * 1e6).astype(np.float32)         # what lies beyond a count must not be read
    xb[0] = x[:T]; xb[1, :5] = x[400:405]
    nf = np.array([T, 5, 0], np.int32)
    refs = []
    for u in range(3):
        m = R.EnergyVADMetric(Cs.ENERGY_INITIAL, thr, headN, tailN, N); d, s = m.run(xb[u, :nf[u]]); refs.append((d, s, m))
    gd, gs, (gh, gc) = dsr.sad_energy(_dev(xb, cuda), thr, headN, tailN, initialEnergy=Cs.ENERGY_INITIAL, energiesN=N, nframes=_dev(nf, cuda))
    for u in range(3):
        d, s, m = refs[u]; n = nf[u]
        _same("ragged %d decision" % u, gd.cpu().numpy()[u, :n], d); _same("ragged %d score" % u, gs.cpu().numpy()[u, :n], s)
        assert not gd.cpu().numpy()[u, n:].any() and not gs.cpu().numpy()[u, n:].any()
        _same("ragged %d history" % u, gh.cpu().numpy()[u], m.state()[0]); _same("ragged %d counters" % u, gc.cpu().numpy()[u], m.state()[1])
    # two calls that carry the state equal one
    first = np.array([113, 2, 0], np.int32)
    st = dsr.sad_energy_state(3, N, Cs.ENERGY_INITIAL, cuda)
    da, sa, st = dsr.sad_energy(_dev(xb[:, :113], cuda), thr, headN, tailN, state=st, nframes=_dev(first, cuda))
    rest = np.ascontiguousarray(np.stack([xb[0, 113:], np.concatenate([xb[1, 2:], xb[1, :2]])[:T - 113], xb[2, 113:]]))
    db, sb, st = dsr.sad_energy(_dev(rest, cuda), thr, headN, tailN, state=st, nframes=_dev(nf - first, cuda))
    for u in range(3):
        d = np.concatenate([da.cpu().numpy()[u, :first[u]], db.cpu().numpy()[u, :nf[u] - first[u]]])
        _same("two calls %d decision" % u, d, refs[u][0])
        _same("two calls %d history" % u, st[0].cpu().numpy()[u], refs[u][2].state()[0]); _same("two calls %d counters" % u, st[1].cpu().numpy()[u], refs[u][2].state()[1])
    # reset() keeps the history, nextSpeaker() refills it
    dsr.sad_energy_reset(st); refs[0][2].reset()
    _same("reset history", st[0].cpu().numpy()[0], refs[0][2].state()[0]); _same("reset counters", st[1].cpu().numpy()[0], refs[0][2].state()[1])
    d2, _, st = dsr.sad_energy(_dev(x[None, 300:420], cuda), thr, headN, tailN, state=(st[0][:1].contiguous(), st[1][:1].contiguous()))
    _same("after reset decision", d2.cpu().numpy()[0], refs[0][2].run(x[300:420])[0])
    fresh = dsr.sad_energy_state(1, N, Cs.ENERGY_INITIAL, cuda)
    assert torch.all(fresh[0] == Cs.ENERGY_INITIAL) and not fresh[1].any()


def test_energy_refusals(dsr, cuda):
    x = _dev(Cs.energy_blocks(160)[None, :8], cuda)
    for thr in (1.0, -0.1, 1.5):
        with pytest.raises(dsr.DsrError) as e:
            dsr.sad_energy(x, thr)
        assert e.value.status == dsr.E_DIMENSION
    st = dsr.sad_energy_state(1, 5, 1.0, cuda)
    with pytest.raises(dsr.DsrError) as e:
        dsr.sad_energy_percentile(st, 100.0)
    assert e.value.status == dsr.E_DIMENSION
    with pytest.raises(dsr.DsrError):
        dsr.sad_energy_percentile(st, -1.0)


# ---------------------------------------------------------------- SimpleEnergyVAD
def test_simple_energy_vad(dsr, cuda):
    X = Cs.channels(2, 64, 40)[0]
    nf = np.array([40, 7], np.int32)
    refs = [R.SimpleEnergyVAD(1.5, 0.9) for _ in range(2)]
    out = [refs[u].run(X[u, :nf[u]]) for u in range(2)]
    gd, gs, E = dsr.sad_simple_energy(_dev(X, cuda), 1.5, 0.9, nframes=_dev(nf, cuda))
    for u in range(2):
        _same("simple %d decision" % u, gd.cpu().numpy()[u, :nf[u]], out[u][0]); _same("simple %d score" % u, gs.cpu().numpy()[u, :nf[u]], out[u][1])
        assert not gd.cpu().numpy()[u, nf[u]:].any()
    _same("simple state", E.cpu().numpy(), np.array([r.E for r in refs]))
    da, sa, E2 = dsr.sad_simple_energy(_dev(X[:1, :13], cuda), 1.5, 0.9)
    db, sb, E2 = dsr.sad_simple_energy(_dev(X[:1, 13:], cuda), 1.5, 0.9, state=E2)
    _same("simple two calls", np.concatenate([sa.cpu().numpy()[0], sb.cpu().numpy()[0]]), out[0][1])
    _same("simple two calls state", E2.cpu().numpy(), np.array([refs[0].E]))


# ---------------------------------------------------------------- the power family
@pytest.mark.parametrize("case", Cs.POWER_CASES, ids=str)
def test_power_family(dsr, cuda, case):
    C, N, lo, hi = case
    P = Cs.channels(C, N, Cs.POWER_T)[1]
    lowX, highX, binN = R.band(N, Cs.RATE, lo, hi)
    assert dsr.sad_band(N, Cs.RATE, lo, hi) == (lowX, highX, binN)
    Pb = np.stack([P, P[:, ::-1]]); nf = np.array([Cs.POWER_T, 9], np.int32)      # a second, shorter utterance
    for kind in range(3):
        gd, gp, gs = dsr.sad_power(_dev(Pb, cuda), N, kind, Cs.RATE, lo, hi, nframes=_dev(nf, cuda))
        for u in range(2):
            n = nf[u]
            dec, pw, score = R.power_metric(Pb[u][:, :n], N, lowX, highX, kind)
            _same("power %s kind %d powers" % (case, kind), gp.cpu().numpy()[u, :n], pw)
            got = gs.cpu().numpy()[u, :n]
            if kind == 0:
                _same("power %s score" % (case,), got, score); _same("power %s decision" % (case,), gd.cpu().numpy()[u, :n], dec)
            else:
                rel = np.abs(got - score) / np.abs(score)
                print("power %s kind %d: max relative error %.3g" % (case, kind, rel.max()))
                assert rel.max() <= 1e-12
                thr = 1.0 / C if kind == 1 else 0.0
                out = Cs.left_out(score, thr, 1e-12 * np.abs(score))
                assert out.mean() <= Cs.LEFT_OUT_CAP and np.array_equal(gd.cpu().numpy()[u, :n][~out], dec[~out])
            assert not gp.cpu().numpy()[u, n:].any() and not gd.cpu().numpy()[u, n:].any()
    dec, pw, score = R.power_metric(P, N, lowX, highX, 0, E0=2.5)
    _same("setE0", dsr.sad_power(_dev(P[None], cuda), N, 0, Cs.RATE, lo, hi, E0=2.5)[0].cpu().numpy()[0], dec)


def test_power_cutoff_at_nyquist_is_refused(dsr, cuda):
    P = _dev(Cs.channels(2, 64, 4)[1][None], cuda)
    for kw in (dict(highCutoff=8000.0), dict(lowCutoff=8000.0), dict(highCutoff=9000.0)):
        with pytest.raises(dsr.DsrError) as e:
            dsr.sad_power(P, 64, 0, Cs.RATE, **kw)
        assert e.value.status == dsr.E_DIMENSION


# ---------------------------------------------------------------- CCCVADMetric
@pytest.mark.parametrize("case", Cs.CCC_CASES, ids=str)
def test_ccc_metric(dsr, cuda, case):
    import torch
    C, N, nCand, lowX, highX = case
    hx = N // 2 if highX is None else highX
    X = Cs.ccc_input(case)
    dec, score = Cs.ccc_reference(case)
    Xb = np.stack([X, X[:, ::-1]]); nf = np.array([Cs.CCC_T, 4], np.int32)
    gd, gs = dsr.sad_ccc(_dev(Xb, cuda), nCand, Cs.CCC_THRESHOLD, band=(lowX, hx), nframes=_dev(nf, cuda))
    got = gs.cpu().numpy()[0]
    assert np.array_equal(np.isnan(got), np.isnan(score))
    err = np.nanmax(np.abs(got - score)); print("ccc %s: max absolute error %.3g" % (case, err))
    assert err <= 1e-12
    out = Cs.left_out(score, Cs.CCC_THRESHOLD, 1e-12)
    assert out.mean() <= Cs.LEFT_OUT_CAP and np.array_equal(gd.cpu().numpy()[0][~out], dec[~out])
    d1, s1 = R.ccc_metric(Xb[1][:, :4], lowX, hx, nCand, Cs.CCC_THRESHOLD)
    assert np.nanmax(np.abs(gs.cpu().numpy()[1, :4] - s1)) <= 1e-12 and not gs.cpu().numpy()[1, 4:].any() and not gd.cpu().numpy()[1, 4:].any()
    out1 = Cs.left_out(s1, Cs.CCC_THRESHOLD, 1e-12)
    assert out1.mean() <= Cs.LEFT_OUT_CAP and np.array_equal(gd.cpu().numpy()[1, :4][~out1], d1[~out1])
    # complex64 input: the same values widened
    X32 = X.astype(np.complex64)
    d32, s32 = R.ccc_metric(X32, lowX, hx, nCand, Cs.CCC_THRESHOLD)
    gd32, g32 = [t.cpu().numpy()[0] for t in dsr.sad_ccc(_dev(X32[None], cuda), nCand, Cs.CCC_THRESHOLD, band=(lowX, hx))]
    assert np.array_equal(np.isnan(g32), np.isnan(s32)) and np.nanmax(np.abs(g32 - s32)) <= 1e-12
    out32 = Cs.left_out(s32, Cs.CCC_THRESHOLD, 1e-12)
    assert out32.mean() <= Cs.LEFT_OUT_CAP and np.array_equal(gd32[~out32], d32[~out32])


def test_ccc_refusals(dsr, cuda):
    import torch
    X = torch.zeros((1, 2, 3, 96), dtype=torch.complex128, device=cuda)
    with pytest.raises(dsr.DsrError) as e:
        dsr.sad_ccc(X, 2)
    assert e.value.status == dsr.E_DIMENSION
    X = torch.zeros((1, 2, 3, 64), dtype=torch.complex128, device=cuda)
    for nCand in (0, 65):
        with pytest.raises(dsr.DsrError):
            dsr.sad_ccc(X, nCand)


# ---------------------------------------------------------------- the segmenters
def test_hangover_cases_in_one_ragged_batch(dsr, cuda):
    for kind in (0, 1, 2):
        for K in sorted({len(c[2]) for c in Cs.HANGOVER_CASES if c[1] == kind}):
            cases = [c for c in Cs.HANGOVER_CASES if c[1] == kind and len(c[2]) == K]
            for headN, tailN in sorted({(c[3], c[4]) for c in cases}):
                group = [c for c in cases if (c[3], c[4]) == (headN, tailN)]
                T = max(len(c[2][0]) for c in group); U = len(group)
                dec = np.full((K, U, T), 1.0); nf = np.zeros(U, np.int32)       # 1.0 beyond a count: reading it would start or prolong a segment
                for u, c in enumerate(group):
                    d = Cs.hangover_input(c); nf[u] = d.shape[1]; dec[:, u, :nf[u]] = d
                st, ln, cons, dm = [t.cpu().numpy() for t in dsr.sad_hangover(_dev(dec, cuda), [0.5] * K, headN, tailN, kind, nframes=_dev(nf, cuda))]
                src = np.arange(U * T * 3, dtype=np.float32).reshape(U, T, 3)
                packed = dsr.sad_gather(_dev(src, cuda), _dev(st, cuda), _dev(ln, cuda)).cpu().numpy()
                for u, c in enumerate(group):
                    r = R.hangover(Cs.hangover_input(c), [0.5] * K, headN, tailN, kind)
                    assert (st[u], ln[u], cons[u]) == (r["start"], r["length"], r["consumed"]), (c[0], st[u], ln[u], cons[u])
                    codes = np.zeros(T, np.int32); codes[:nf[u]] = r["codes"]
                    _same("hangover %s decisionMetric" % c[0], dm[u], codes)
                    _same("hangover %s frames" % c[0], packed[u], R.gather(src[u], max(r["start"], 0), r["length"]))


def test_hangover_refusals(dsr, cuda):
    dec = _dev(np.ones((2, 1, 4)), cuda)
    with pytest.raises(dsr.DsrError):
        dsr.sad_hangover(dec, [0.5, 0.5], 2, 2, 1)                            # the MI segmenter takes three metrics
    with pytest.raises(dsr.DsrError):
        dsr.sad_hangover(dec, [0.5, 0.5], 0, 2, 0)


# ---------------------------------------------------------------- the generalised-Gaussian metrics
def _gg_check(tag, got_dec, got_score, ref_dec, ref_score, base, thr):
    """scores within 1e-12 x the restatement's sum of absolute per-bin terms / binN; decisions equal wherever the score is farther from the threshold"""
    tol = 1e-12 * base
    err = np.abs(got_score - ref_score)
    print("%s: max |error| / (sum |terms| / binN) = %.3g" % (tag, (err / np.where(base > 0, base, 1.0)).max()))
    assert np.all(err <= tol), (tag, err.max())
    out = Cs.left_out(ref_score, thr, tol)
    assert out.mean() <= Cs.LEFT_OUT_CAP and np.array_equal(got_dec[~out], ref_dec[~out]), tag


@pytest.mark.parametrize("case", Cs.GG_CASES, ids=str)
def test_gg_metrics(dsr, cuda, case, tmp_path):
    fftLen, mixed, twiddle, lo, hi = case
    r = Cs.gg_reference(case); m = r["model"]
    X1, X2, e1, e2 = Cs.gg_input(fftLen); T = Cs.GG_T
    if mixed:
        Cs.write_shape_factors(tmp_path, Cs.gg_shape_factors(fftLen))     # read back from the reference's directory layout
        _same("shape factors", dsr.sad_read_shape_factors(tmp_path, fftLen), np.array(Cs.gg_shape_factors(fftLen)))
    g = dsr.SadGG(fftLen, str(tmp_path) if mixed else None, Cs.RATE, lo, hi)
    assert R.differing(g.table, m.table) == 0 and g.fixedThreshold == m.fixed      # the host model: the same C library functions on both sides
    # a ragged batch of two: the second utterance is the first one's tail, with noise beyond its count
    n2 = 9; nf = np.array([T, n2], np.int32)
    rng = np.random.default_rng(1)

    def two(a, noise):
        b = np.array(noise, a.dtype); b[:n2] = a[T - n2:]
        return _dev(np.stack([a, b]), cuda)
    cn = lambda a: (rng.standard_normal(a.shape) + 1j * rng.standard_normal(a.shape)) * 1e3          # noqa: E731
    B1, B2 = two(X1, cn(X1)), two(X2, cn(X2))
    E1, E2 = two(e1, np.abs(rng.standard_normal(e1.shape)) * 1e3), two(e2, np.abs(rng.standard_normal(e2.shape)) * 1e3)
    nfd = _dev(nf, cuda)
    d, s = [t.cpu().numpy() for t in g.run(dsr.SAD_NEGENTROPY, B1, E1, nframes=nfd)]
    rd, rs, base = r["negentropy"]
    _gg_check("negentropy %s" % (case,), d[0], s[0], rd, rs, base, Cs.GG_THRESHOLDS["negentropy"])
    if not mixed:
        assert not s.any(), "a Gaussian model gives exactly 0 on the device too"
    t2 = R.negentropy(m, X1[T - n2:], e1[T - n2:], Cs.GG_THRESHOLDS["negentropy"])
    _gg_check("negentropy tail", d[1, :n2], s[1, :n2], t2[0], t2[1], t2[2], Cs.GG_THRESHOLDS["negentropy"])
    assert not s[1, n2:].any() and not d[1, n2:].any()
    d, s = [t.cpu().numpy() for t in g.run(dsr.SAD_LIKELIHOOD_RATIO, B1, E1, B2, E2, nframes=nfd)]
    rd, rs, base = r["lr"]
    _gg_check("likelihood ratio %s" % (case,), d[0], s[0], rd, rs, base, Cs.GG_THRESHOLDS["lr"])
    assert not s[1, n2:].any()
    d, s, rho, thr = g.run(dsr.SAD_MUTUAL_INFORMATION, B1, E1, B2, E2, twiddle=twiddle, nframes=nfd, return_threshold=True)
    d, s, rho, thr = d.cpu().numpy(), s.cpu().numpy(), rho.cpu().numpy(), thr.cpu().numpy()
    rd, rs, rthr, base, clamped = r["mi"]
    _gg_check("mutual information %s" % (case,), d[0], s[0], rd, rs, base, rthr)
    assert np.all(np.abs(thr[0] - rthr) <= 1e-12 * np.maximum(base, 1.0)) and not s[1, n2:].any()
    assert np.abs(rho[0] - r["rho"]).max() <= 1e-12 and np.abs(rho[0]).max() == pytest.approx(0.9, abs=1e-12)
    rho2 = np.zeros(m.F, np.complex128); t2 = R.mutual_information(m, X1[T - n2:], X2[T - n2:], e1[T - n2:], e2[T - n2:], rho2, twiddle)
    assert np.all(np.abs(s[1, :n2] - t2[1]) <= 1e-12 * t2[3]) and np.abs(rho[1] - rho2).max() <= 1e-12
    # rho carried over two calls equals one call, bit for bit
    cut = 23
    a = g.run(dsr.SAD_MUTUAL_INFORMATION, B1[:1, :cut].contiguous(), E1[:1, :cut].contiguous(), B2[:1, :cut].contiguous(), E2[:1, :cut].contiguous(), twiddle=twiddle)
    b = g.run(dsr.SAD_MUTUAL_INFORMATION, B1[:1, cut:].contiguous(), E1[:1, cut:].contiguous(), B2[:1, cut:].contiguous(), E2[:1, cut:].contiguous(), twiddle=twiddle, rho=a[2])
    _same("mi two calls score", np.concatenate([a[1].cpu().numpy()[0], b[1].cpu().numpy()[0]]), s[0])
    _same("mi two calls rho", b[2].cpu().numpy()[0].view(np.float64), rho[0].view(np.float64))


def test_gg_refusals_and_streams(dsr, cuda, tmp_path):
    from dsr.btk.sad import (EnergyVADMetricPtr, HangoverMIVADFeaturePtr, HangoverMultiStageVADFeaturePtr, LikelihoodRatioVADMetricPtr,
                             MutualInformationVADMetricPtr, NegentropyVADMetricPtr, PowerSpectrumVADMetricPtr)
    from dsr.btk.stream import PyVectorComplexFeatureStreamPtr, PyVectorFloatFeatureStreamPtr
    with pytest.raises(dsr.DsrError) as e:
        dsr.SadGG(64, np.full(33, 0.01))                                      # the bisection does not converge: JNUMERIC, not an endless loop
    assert e.value.status == 12
    with pytest.raises(dsr.DsrError):
        dsr.SadGG(64, None, Cs.RATE, -1.0, 8000.0)
    fftLen = 64
    X1, X2, e1, e2 = Cs.gg_input(fftLen); T = Cs.GG_T
    sf = Cs.gg_shape_factors(fftLen); Cs.write_shape_factors(tmp_path, sf)
    g = dsr.SadGG(fftLen, sf)
    cs = lambda a, *more: PyVectorComplexFeatureStreamPtr(Frames(a, *more))   # noqa: E731
    fs = lambda a, *more: PyVectorFloatFeatureStreamPtr(Frames(a, *more))     # noqa: E731
    D = lambda a: _dev(a[None], cuda)                                         # noqa: E731
    bd, bs = g.run(dsr.SAD_NEGENTROPY, D(X1), D(e1), threshold=-0.1)
    d, s = _values(NegentropyVADMetricPtr(cs(X1), fs(e1), str(tmp_path), -0.1))
    _same("NegentropyVADMetricPtr decision", d, bd.cpu().numpy()[0]); _same("NegentropyVADMetricPtr score", s, bs.cpu().numpy()[0])
    bd, bs = g.run(dsr.SAD_LIKELIHOOD_RATIO, D(X1), D(e1), D(X2), D(e2), threshold=-0.3)
    d, s = _values(LikelihoodRatioVADMetricPtr(cs(X1), cs(X2), fs(e1), fs(e2), str(tmp_path), -0.3))
    _same("LikelihoodRatioVADMetricPtr decision", d, bd.cpu().numpy()[0]); _same("LikelihoodRatioVADMetricPtr score", s, bs.cpu().numpy()[0])
    # MutualInformationVADMetric: two utterances, rho survives reset() and is zeroed by nextSpeaker()
    h = T // 2
    mi = MutualInformationVADMetricPtr(cs(X1[:h], X1[h:]), cs(X2[:h], X2[h:]), fs(e1[:h], e1[h:]), fs(e2[:h], e2[h:]), str(tmp_path), 1.0, 1.3, 0.9)
    bd, bs, rho = g.run(dsr.SAD_MUTUAL_INFORMATION, D(X1), D(e1), D(X2), D(e2), twiddle=1.0, beta=0.9)
    d1, s1 = _values(mi); mi.reset(); d2, s2 = _values(mi)
    _same("MutualInformationVADMetricPtr decision", np.concatenate([d1, d2]), bd.cpu().numpy()[0])
    _same("MutualInformationVADMetricPtr score", np.concatenate([s1, s2]), bs.cpu().numpy()[0])
    mi.nextSpeaker()
    d3, s3 = _values(mi)                                                      # the sources stay at their last utterance; rho starts from zero
    fresh = g.run(dsr.SAD_MUTUAL_INFORMATION, D(X1[h:]), D(e1[h:]), D(X2[h:]), D(e2[h:]), twiddle=1.0, beta=0.9)
    _same("after nextSpeaker", s3, fresh[1].cpu().numpy()[0])
    # HangoverMIVADFeature with the metric it is named for; the metric's rho advances by the frames the segmenter consumed
    feat = np.ascontiguousarray(e1[:, :8])
    energy = EnergyVADMetricPtr(fs(feat), energiesN=5, headN=2, tailN=3, initialEnergy=1.0)
    mim = MutualInformationVADMetricPtr(cs(X1), cs(X2), fs(e1), fs(e2), str(tmp_path), -1.0, 0.2, 0.95)
    lr = LikelihoodRatioVADMetricPtr(cs(X1), cs(X2), fs(e1), fs(e2), str(tmp_path), -0.3)
    hang = HangoverMIVADFeaturePtr(fs(feat), energy, mim, lr, headN=2, tailN=3)
    import torch
    edec = dsr.sad_energy(D(feat), 0.5, 2, 3, initialEnergy=1.0, energiesN=5)[0][0]
    mdec, _, rho_all = g.run(dsr.SAD_MUTUAL_INFORMATION, D(X1), D(e1), D(X2), D(e2), threshold=0.2)
    ldec = g.run(dsr.SAD_LIKELIHOOD_RATIO, D(X1), D(e1), D(X2), D(e2), threshold=-0.3)[0]
    dec = torch.stack([edec, mdec[0], ldec[0]]).cpu().numpy()
    r = R.hangover(dec, [0.5] * 3, 2, 3, 1)
    print("HangoverMIVADFeaturePtr over the mutual information: segment %d + %d, consumed %d, codes %s" % (r["start"], r["length"], r["consumed"], r["codes"].tolist()))
    rows, trace = [], []
    while True:
        try:
            rows.append(np.array(hang.next(), copy=True)); trace.append((hang.prefixN(), hang.decisionMetric()))
        except StopIteration:
            break
    assert r["length"] > 0 and trace == r["trace"]
    _same("HangoverMIVADFeaturePtr frames", np.stack(rows), feat[r["start"]:r["start"] + r["length"]])
    hang.reset()                                                              # the second pass starts from the rho after `consumed` frames
    c = r["consumed"]
    part = g.run(dsr.SAD_MUTUAL_INFORMATION, D(X1[:c]), D(e1[:c]), D(X2[:c]), D(e2[:c]), threshold=0.2)
    again = g.run(dsr.SAD_MUTUAL_INFORMATION, D(X1), D(e1), D(X2), D(e2), threshold=0.2, rho=part[2])
    d4, s4 = _values(mim)
    _same("rho committed with the consumed frames", s4, again[1].cpu().numpy()[0])
    # a MutualInformationVADMetric at stage >= 2 of the multi-stage segmenter would be advanced twice a frame
    ms = HangoverMultiStageVADFeaturePtr(fs(feat), EnergyVADMetricPtr(fs(feat)))
    pm = PowerSpectrumVADMetricPtr(fftLen); pm.setChannel(fs(e1)); pm.setChannel(fs(e2))
    ms.setMetric(pm, 0.5)
    with pytest.raises(dsr.DsrError) as e:
        ms.setMetric(MutualInformationVADMetricPtr(cs(X1), cs(X2), fs(e1), fs(e2)), 0.5)
    assert e.value.status == dsr.E_CONSISTENCY
    ms.setMetric(NegentropyVADMetricPtr(cs(X1), fs(e1)), 0.5)                 # a stateless one is welcome


# ---------------------------------------------------------------- the spectral-shape operators
@pytest.mark.parametrize("case", Cs.SHAPE_CASES, ids=str)
def test_shape_operators(dsr, cuda, case):
    dim, T = case
    x = Cs.shape_input(case)
    xb = np.stack([x, (np.random.default_rng(dim).standard_normal(x.shape) * 1e6).astype(np.float32)]); xb[1, :3] = x[T - 3:]
    nf = np.array([T, 3], np.int32)

    def run(op, **kw):
        y = dsr.sad_shape(_dev(xb, cuda), op, nframes=_dev(nf, cuda), **kw).cpu().numpy()
        assert y.shape == (2, T, 1) and not y[1, 3:].any()
        return y[0, :, 0], y[1, :3, 0]

    for thr in (0.0, 1000.0):
        a, b = run(dsr.SAD_BAND_ENERGY_RATIO, sampleRate=16000.0, thresh=thr)
        _same("band energy ratio %s %g" % (case, thr), a, R.band_energy_ratio(x, 16000.0, thr)); _same("second", b, R.band_energy_ratio(x[T - 3:], 16000.0, thr))
    for thr in (0.0, 0.01, 0.2):
        a, b = run(dsr.SAD_SIGNIFICANT_SUBBANDS, thresh=thr)
        _same("significant subbands %s %g" % (case, thr), a, R.significant_subbands(x, thr)); _same("second", b, R.significant_subbands(x[T - 3:], thr))
    for name, op, ref in (("energy diffusion", dsr.SAD_ENERGY_DIFFUSION, R.energy_diffusion), ("negative entropy", dsr.SAD_NEGATIVE_ENTROPY, R.negative_entropy)):
        a, b = run(op)
        u = np.concatenate([R.ulps(a, ref(x)), R.ulps(b, ref(x[T - 3:]))])
        print("%s %s: %d of %d elements are 1 ulp off, the largest distance is %d ulp" % (name, case, int((u == 1).sum()), u.size, int(u.max())))
        assert np.array_equal(np.isnan(a), np.isnan(ref(x))) and u.max() <= 1
    with pytest.raises(dsr.DsrError) as e:
        dsr.sad_shape(_dev(xb, cuda), dsr.SAD_BAND_ENERGY_RATIO, sampleRate=16000.0, thresh=9000.0)      # the low band would be read past the frame
    assert e.value.status == dsr.E_DIMENSION


def test_shape_streams(dsr, cuda):
    from dsr.btk.sad import BandEnergyRatioFeaturePtr, EnergyDiffusionFeaturePtr, NegativeEntropyFeaturePtr, SignificantSubbandsFeaturePtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    x = Cs.shape_input((33, 7)); xd = _dev(x[None], cuda)
    src = lambda: PyVectorFloatFeatureStreamPtr(Frames(x))                    # noqa: E731
    for stream, batch in ((EnergyDiffusionFeaturePtr(src()), dsr.sad_shape(xd, dsr.SAD_ENERGY_DIFFUSION)),
                          (BandEnergyRatioFeaturePtr(src(), 8000.0, 1000.0), dsr.sad_shape(xd, dsr.SAD_BAND_ENERGY_RATIO, 8000.0, 1000.0)),
                          (NegativeEntropyFeaturePtr(src()), dsr.sad_shape(xd, dsr.SAD_NEGATIVE_ENTROPY)),
                          (SignificantSubbandsFeaturePtr(src(), 0.05), dsr.sad_shape(xd, dsr.SAD_SIGNIFICANT_SUBBANDS, thresh=0.05))):
        assert stream.size() == 1
        _same(type(stream).__name__, np.stack(_rows(stream)), batch.cpu().numpy()[0])


# ---------------------------------------------------------------- the stream classes
def test_metric_streams_against_the_batch_result(dsr, cuda):
    from dsr.btk.sad import (CCCVADMetricPtr, EnergyVADMetricPtr, NormalizedEnergyMetricPtr, PowerSpectrumVADMetricPtr, SimpleEnergyVADPtr,
                             TSPSVADMetricPtr)
    from dsr.btk.stream import PyVectorComplexFeatureStreamPtr, PyVectorFloatFeatureStreamPtr
    # EnergyVADMetric: two utterances, reset() between them keeps the history
    x = Cs.energy_blocks(160); a, b = x[:200], x[200:330]
    m = EnergyVADMetricPtr(PyVectorFloatFeatureStreamPtr(Frames(a, b)), energiesN=65, headN=1, threshold=0.31)
    ref = R.EnergyVADMetric(energiesN=65, headN=1, threshold=0.31)
    d, s = _values(m); rd, rs = ref.run(a)
    _same("EnergyVADMetricPtr decision", d, rd); _same("EnergyVADMetricPtr score", s, rs)
    assert m.energyPercentile(50.0) == ref.energyPercentile(50.0)
    m.reset(); ref.reset()
    d, s = _values(m); rd, rs = ref.run(b)
    _same("EnergyVADMetricPtr second utterance", d, rd)
    assert m.energyPercentile(25.0) == ref.energyPercentile(25.0)
    m.nextSpeaker(); ref.nextSpeaker()
    assert m.energyPercentile() == ref.energyPercentile(50.0)
    # the power family and CCC: the streams' values are the batch entries'
    C, N = 3, 64
    X, P = Cs.channels(C, N, 12)
    for cls, kind in ((PowerSpectrumVADMetricPtr, 0), (NormalizedEnergyMetricPtr, 1), (TSPSVADMetricPtr, 2)):
        pm = cls(N, Cs.RATE, 187.0, 1000.0)
        for c in range(C):
            pm.setChannel(PyVectorFloatFeatureStreamPtr(Frames(P[c])))
        bd, bp, bs = dsr.sad_power(_dev(P[None], cuda), N, kind, Cs.RATE, 187.0, 1000.0)
        d = []
        for t in range(12):
            d.append(pm.next(t)); _same("%s getMetrics" % cls.__name__, pm.getMetrics(), bp.cpu().numpy()[0, t])
            if kind > 0:
                assert pm.score() == bs.cpu().numpy()[0, t]
        _same(cls.__name__, np.array(d), bd.cpu().numpy()[0])
        with pytest.raises(StopIteration):
            pm.next()
    with pytest.raises(dsr.DsrError) as e:
        PowerSpectrumVADMetricPtr(N, Cs.RATE, -1.0, 8000.0)
    assert e.value.status == dsr.E_DIMENSION
    cm = CCCVADMetricPtr(N, 3, Cs.RATE)
    for c in range(C):
        cm.setChannel(PyVectorComplexFeatureStreamPtr(Frames(X[c])))
    cm.setThreshold(0.3); cm.setNCand(2)
    bd, bs = dsr.sad_ccc(_dev(X[None], cuda), 2, 0.3)
    d, s = _values(cm)
    _same("CCCVADMetricPtr decision", d, bd.cpu().numpy()[0]); _same("CCCVADMetricPtr score", s, bs.cpu().numpy()[0])
    with pytest.raises(dsr.DsrError):
        CCCVADMetricPtr(96, 2)
    sv = SimpleEnergyVADPtr(PyVectorComplexFeatureStreamPtr(Frames(X[0])), 1.5, 0.9)
    rd, rs = R.SimpleEnergyVAD(1.5, 0.9).run(X[0])
    got = []
    while True:
        try:
            got.append(sv.next())
        except StopIteration:
            break
    assert got == [bool(v) for v in rd]


def test_hangover_streams(dsr, cuda):
    from dsr.btk.sad import (EnergyVADMetricPtr, HangoverMIVADFeaturePtr, HangoverMultiStageVADFeaturePtr, HangoverVADFeaturePtr,
                             NormalizedEnergyMetricPtr, PowerSpectrumVADMetricPtr)
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    # HangoverVADFeature over an EnergyVADMetric: two utterances; the metric's history is carried with the frames the segmenter consumed
    x = Cs.energy_blocks(160); utts = (x[:700], x[560:842])
    headN, tailN = 4, 10
    src = PyVectorFloatFeatureStreamPtr(Frames(*utts))
    h = HangoverVADFeaturePtr(src, EnergyVADMetricPtr(src, headN=headN, tailN=tailN), 0.5, headN, tailN)
    assert h.prefixN() == -headN and h.size() == 160
    ref = R.EnergyVADMetric(headN=headN, tailN=tailN)
    for n, utt in enumerate(utts):
        hist, cnt = ref.hist.copy(), (ref.aboveN, ref.belowN, ref.recognizing, ref.pos)
        dec, _ = ref.run(utt)                                                # the decisions of a walk over the whole utterance ...
        r = R.hangover(dec[None], [0.5], headN, tailN, 0)
        ref.hist, (ref.aboveN, ref.belowN, ref.recognizing, ref.pos) = hist, cnt
        ref.run(utt[:r["consumed"]]); ref.reset()                            # ... but the state of the frames the reference pulls
        rows = _rows(h)
        print("utterance %d: segment %d + %d, consumed %d of %d" % (n, r["start"], r["length"], r["consumed"], len(utt)))
        assert r["length"] > 0 and r["consumed"] < len(utt)                  # both segments end before their source does
        _same("HangoverVADFeaturePtr utterance %d" % n, np.stack(rows), utt[r["start"]:r["start"] + r["length"]])
        assert h.prefixN() == r["start"] and h.isEnd()
        h.reset()
    # the MI and multi-stage segmenters over stateless metrics: prefixN() and decisionMetric() after every next()
    C, N, T = 3, 64, 40
    P = Cs.channels(C, N, T, coherent=False)[1]
    feat = np.ascontiguousarray(P[0][:, :8])

    def power(cls, kind, E0, order):
        m = cls(N, Cs.RATE)
        for c in order:
            m.setChannel(PyVectorFloatFeatureStreamPtr(Frames(P[c])))
        m.setE0(E0)
        return m

    def batch(kind, E0, order):
        return dsr.sad_power(_dev(P[list(order)][None], cuda), N, kind, Cs.RATE, E0=E0)[0][0]

    specs = [(PowerSpectrumVADMetricPtr, 0, 1.5, (1, 0, 2)), (PowerSpectrumVADMetricPtr, 0, 1.55, (2, 0, 1)), (NormalizedEnergyMetricPtr, 1, 1.5, (2, 1, 0))]
    import torch
    for kind, cls, tailN in ((1, HangoverMIVADFeaturePtr, 3), (2, HangoverMultiStageVADFeaturePtr, 2)):
        e = EnergyVADMetricPtr(PyVectorFloatFeatureStreamPtr(Frames(feat)), energiesN=5, headN=2, tailN=3, initialEnergy=1.0)
        others = [power(*s) for s in specs[:2 if kind == 1 else 3]]
        fs = PyVectorFloatFeatureStreamPtr(Frames(feat))
        if kind == 1:
            h = cls(fs, e, others[0], others[1], headN=2, tailN=tailN)
        else:
            h = cls(fs, e, headN=2, tailN=tailN)
            for m in others:
                h.setMetric(m, 0.5)
        edec = dsr.sad_energy(_dev(feat[None], cuda), 0.5, 2, 3, initialEnergy=1.0, energiesN=5)[0][0]
        dec = torch.stack([edec] + [batch(s[1], s[2], s[3]) for s in specs[:len(others)]]).cpu().numpy()
        r = R.hangover(dec, [0.5] * len(dec), 2, tailN, kind)
        print("%s: segment %d + %d, codes %s" % (cls.__name__, r["start"], r["length"], r["codes"].tolist()))
        assert r["length"] > 0
        trace = []
        rows = []
        while True:
            try:
                rows.append(np.array(h.next(), copy=True)); trace.append((h.prefixN(), h.decisionMetric()))
            except StopIteration:
                break
        _same(cls.__name__, np.stack(rows), feat[r["start"]:r["start"] + r["length"]])
        assert trace == r["trace"], (trace, r["trace"])
        assert (h.prefixN(), h.decisionMetric()) == r["last"]
    # a stateful metric at stage >= 2 of the multi-stage segmenter would be advanced twice a frame
    e1 = EnergyVADMetricPtr(PyVectorFloatFeatureStreamPtr(Frames(feat)))
    h = HangoverMultiStageVADFeaturePtr(PyVectorFloatFeatureStreamPtr(Frames(feat)), e1)
    h.setMetric(power(*specs[0]), 0.5)
    with pytest.raises(dsr.DsrError) as err:
        h.setMetric(EnergyVADMetricPtr(PyVectorFloatFeatureStreamPtr(Frames(feat))), 0.5)
    assert err.value.status == dsr.E_CONSISTENCY
