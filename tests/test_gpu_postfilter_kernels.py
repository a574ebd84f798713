"""The Zelinski, McCowan and Lefkimmiatis post-filters (csrc/k_postfilter.hip) in every cell their dispatch can select, on the ragged batches of
tests/pf_dispatch_cases.py: 9 utterances x 17 bins = 153 series in three workgroups of 64 (two of 128 for k_mccowan, 153 wavefronts for k_pf_wave), utterance
boundaries inside workgroups, lengths that end inside a stretch of k_zel_recur, on a stretch edge, around ceil(Tmax / 2) and at 0
(tests/test_pf_dispatch_cases_cpu.py shows that the cases are what they are named for and that the inputs reach the clamps and the range between them).

Every case first asserts its cell through dsr_zelinski_path (ZelinskiPostFilter.path), the helper the launches go through.  What is compared:
  * one shot on the ragged batch with the matching oracle function run per utterance on its own length: weights rtol 1e-6, output 1e-6 of the largest
    reference magnitude (the project's bars: test_zelinski_postfilter, test_mccowan_postfilter, test_lefkimmiatis_postfilter); rows past an utterance's
    length are exactly 0 in both;
  * blocks with carried state -- a first block of one frame, then cuts that leave k_zel_recur's last stretch empty with state carried in and that fall
    inside a stretch -- with the one-shot oracle, at the same bars;
  * after resetState the first block repeats bit for bit;
  * twins on identical input: k_mccowan<C> and k_mccowan<0> (DSR_PF_MEMSTATE) give the same bits (same operations in the same order, no contraction);
    k_zelinski_reg<C> and the sum kernels (DSR_PF_SUM), the thread kernels and k_pf_wave (DSR_PF_WAVE) agree to one fp32 ulp of the weight (their fp64
    sums differ by another summation order only: 1e-13 and 1e-15 relative, k_postfilter.hip's header); the fused beamformer sum and DSR_PF_NOFUSE agree
    at the bars of test_zelinski_postfilter_behind_its_beamformer.

Template instance -> the case that launches it (tests/pf_dispatch_cases.py):
  k_zelinski_reg<2 | 3 | 4 | 6 | 8>        test_cell[zreg2 .. zreg8]
  k_zel_pairs<false> + k_zel_recur         test_cell[zsum5_T1 .. zsum5_T272] (the ladder of Tmax), [zsum16_*] [zsum17_*] [zsum64_*], [zsum2_switch_*] [zsum8_switch_*]
                                           (DSR_PF_SUM), test_zelinski_registers_against_sum, the DSR_PF_NOFUSE twin of test_fused_against_two_calls
  k_zel_pairs<true> + k_zel_recur          test_cell[zbf5_ds_T33] [zbf5_mvdr_T129] [zbf17_ds_T129] [zbf17_mvdr_T17], test_fused_against_two_calls
  k_mccowan<2 | 3 | 4 | 6 | 8>             test_cell[mcreg*] (McCowan), [lfreg*] (Lefkimmiatis)
  k_mccowan<0>                             test_cell[mcmem5 | 7 | 16] [lfmem5 | 7 | 16], [mcmem4_switch] [mcmem8_switch] [lfmem4_switch] [lfmem8_switch]
                                           (DSR_PF_MEMSTATE), test_mccowan_registers_equal_memory
  k_pf_wave<0>                             test_cell[zwave3] [zwave8] (DSR_PF_WAVE: Zelinski above 16 channels takes the sum kernels), test_threads_against_wave
  k_pf_wave<1>                             test_cell[mcwave17] [mcwave64], [mcwave4_switch] [mcwave8_switch] (DSR_PF_WAVE), test_threads_against_wave
  k_pf_wave<2>                             test_cell[lfwave17] [lfwave64], [lfwave4_switch] [lfwave8_switch], test_threads_against_wave
Run with -s for the measured error of every case."""
import numpy as np
import pytest

from tests import pf_dispatch_cases as PC

pytestmark = pytest.mark.gpu

_ID = dict(ids=lambda c: c["name"])
_IN = {}                                                                       # case -> manifold, snapshots, coherence, lambda: computed once


def _set_env(monkeypatch, env):
    for k in PC.SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _inputs(oracle, case):
    if case["name"] not in _IN:
        wq = PC.manifold(oracle, case); X = PC.snapshots(case, wq)
        R = lam = None
        if case["kind"]:
            R = PC.coherence(oracle, case)
            if case["kind"] == 2:
                lam = oracle.lefkimmiatis_lambda(R, wq, PC.MIN_SV)
        for a in (wq, X, R, lam):
            if a is not None:
                a.setflags(write=False)
        _IN[case["name"]] = (wq, X, R, lam)
    return _IN[case["name"]]


def _ulps(a, b):
    """distance of two arrays of positive fp32 values in units of the last place"""
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64); b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


class _Run:
    """a case's filter (and beamformer) and its batch on the device"""

    def __init__(self, dsr, oracle, cuda, case):
        import torch
        self.dsr, self.oracle, self.cuda, self.case, self.torch = dsr, oracle, cuda, case, torch
        self.wq, self.X, self.R, self.lam = _inputs(oracle, case)
        Cn = case["C"]; a = dict(alpha=case["alpha"], type=case["type"], minFrames=case["minFrames"])
        if case["kind"] == 0:
            self.pf = dsr.ZelinskiPostFilter(PC.M, Cn, self.wq, **a)
        else:
            if case["kind"] == 1:
                self.pf = dsr.McCowanPostFilter(PC.M, Cn, self.wq, threshold=PC.THRESHOLD, **a)
            else:
                self.pf = dsr.LefkimmiatisPostFilter(PC.M, Cn, self.wq, minSV=PC.MIN_SV, fbinX1=PC.FBINX1, threshold=PC.THRESHOLD, **a)
            self.pf.setDiffuseNoiseModel(PC.geometry(case), 16000.0); self.pf.setAllLevelsOfDiagonalLoading(PC.LOADING)
        self.bf = None
        if case["bf"]:
            mp = PC.geometry(case)
            self.bf = dsr.Beamformer(PC.M, Cn); self.bf.calcArrayManifoldVectors(16000.0, PC.look_delays(oracle, case))
            if case["bf"] == "mvdr":
                self.bf.setDiffuseNoiseModel(mp, 16000.0); self.bf.divideAllNonDiagonalElements(0.01); self.bf.calcMVDRWeights(16000.0, 1e-8)
            self.bf.select(case["bf"])
            assert np.abs(self.bf.get(0)[:PC.F] - self.wq).max() <= 1e-12       # the filter's manifold is its beamformer's
            self.Y = PC.beamformed(self.X, self.bf.get(4))
        else:
            self.Y = PC.beamformed(self.X, self.wq)
        self.Xd = torch.from_numpy(np.array(self.X)).to(cuda); self.Yd = torch.from_numpy(self.Y).to(cuda)

    def cell(self, expect=None):
        got = self.pf.path(self.bf)
        expect = expect or self.case["expect"]
        assert got == expect, "%s: the dispatch takes %s with template argument %d, the case is there for %s with %d" % (
            self.case["name"], PC.CELL_NAMES[got[0]], got[1], PC.CELL_NAMES[expect[0]], expect[1])

    def apply(self, lo=0, hi=None):
        """frames [lo, hi) of the batch -> (out, weights, the beamformer's output the filter worked on) as numpy arrays [U][hi - lo][F]"""
        torch = self.torch
        hi = self.case["Tmax"] if hi is None else hi
        nf = torch.tensor(PC.block_lens(self.case["lens"], lo, hi), dtype=torch.int32, device=self.cuda)
        Xb = self.Xd[:, :, lo:hi].contiguous()
        if self.bf is not None:
            out, w, Yf = self.pf.apply_bf(self.bf, Xb, nf, want_weights=True, want_bf_output=True)
        else:
            Yf = self.Yd[:, lo:hi].contiguous()
            out, w = self.pf.apply(Xb, Yf, nf, want_weights=True)
        return out.cpu().numpy(), w.cpu().numpy(), Yf.cpu().numpy()

    def against_oracle(self, what, out, w, Yf):
        """the project's bars, the oracle per utterance on its own length fed with the beamformer output the device worked on"""
        case = self.case; worst_w = worst_o = 0.0
        for u, n in enumerate(case["lens"]):
            assert not out[u, n:].any() and not w[u, n:].any(), "%s %s: utterance %d has non-zero rows past its %d frames" % (case["name"], what, u, n)
            if n == 0:
                continue
            ro, rw = PC.oracle_run(self.oracle, case, self.X, Yf, self.wq, u, n, self.R, self.lam)
            assert np.isfinite(w[u, :n]).all() and np.isfinite(out[u, :n]).all()
            worst_w = max(worst_w, float((np.abs(w[u, :n] - rw) / np.abs(rw)).max()))
            worst_o = max(worst_o, float(np.abs(out[u, :n] - ro).max() / np.abs(ro).max()))
        print("%s %s: weights %.3g relative (bar 1e-6), output %.3g of the largest magnitude (bar 1e-6)" % (case["name"], what, worst_w, worst_o))
        assert worst_w <= 1e-6, "%s %s: weights off by %.3g relative" % (case["name"], what, worst_w)
        assert worst_o <= 1e-6, "%s %s: output off by %.3g of the largest magnitude" % (case["name"], what, worst_o)


@pytest.mark.parametrize("case", PC.ALL_CASES, **_ID)
def test_cell(dsr, oracle, cuda, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    r = _Run(dsr, oracle, cuda, case)
    r.cell()
    out, w, Yf = r.apply()
    if r.bf is not None:                                                       # the beamformer's sum formed in the filter's pass: dsr_bf_apply's bar
        assert np.abs(Yf - r.Y).max() <= 2e-6 * np.abs(r.Y).max()
    r.against_oracle("one shot", out, w, Yf)
    # blocks with carried state against the one-shot oracle
    r.pf.carry(True)
    parts = [r.apply(lo, hi) for lo, hi in case["blocks"]]
    r.cell()
    ob, wb, Yb = (np.concatenate([p[i] for p in parts], axis=1) for i in range(3))
    r.against_oracle("%d carried blocks" % len(parts), ob, wb, Yb)
    r.pf.resetState()                                                          # new streams: the densities start from scratch again
    again = r.apply(*case["blocks"][0])
    assert np.array_equal(again[0].view(np.uint32), parts[0][0].view(np.uint32)) and np.array_equal(again[1].view(np.uint32), parts[0][1].view(np.uint32)), \
        "%s: the first block after resetState is not the first block's bits" % case["name"]


def _twins(dsr, oracle, cuda, monkeypatch, case, env_a, cell_a, env_b, cell_b):
    """the case's batch, one shot and in carried blocks, through two kernels -> [(out, w) of a, (out, w) of b] for the one shot and for the blocks"""
    res = []
    for env, cell in ((env_a, cell_a), (env_b, cell_b)):
        _set_env(monkeypatch, env)
        r = _Run(dsr, oracle, cuda, case)
        r.cell(cell)
        one = r.apply()[:2]
        r.pf.carry(True)
        parts = [r.apply(lo, hi) for lo, hi in case["blocks"]]
        res.append((one, tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(2))))
    return list(zip(*res))


@pytest.mark.parametrize("case", PC.MC_REG_CASES + PC.LF_REG_CASES, **_ID)
def test_mccowan_registers_equal_memory(dsr, oracle, cuda, monkeypatch, case):
    """densities in registers (copied in and out of the carried array) and in the state array in place: the same operations in the same order"""
    for what, (a, b) in zip(("one shot", "carried blocks"),
                            _twins(dsr, oracle, cuda, monkeypatch, case, {}, (PC.MCCOWAN_REG, case["C"]), PC.MEMSTATE, (PC.MCCOWAN_MEM, 0))):
        for name, x, y in (("weights", a[1], b[1]), ("output", a[0], b[0])):
            diff = np.argwhere(np.ascontiguousarray(x).view(np.uint32 if name == "weights" else np.uint64) != np.ascontiguousarray(y).view(np.uint32 if name == "weights" else np.uint64))
            assert len(diff) == 0, "%s %s: %d %s differ between k_mccowan<%d> and k_mccowan<0>, first (utterance, frame, bin) %s" % (
                case["name"], what, len(diff), name, case["C"], diff[0])


def _one_ulp(case, what, names, a, b):
    d = _ulps(a[1], b[1])
    print("%s %s: weights of %s and %s differ by at most %d fp32 ulp (%d of %d differ)" % (case["name"], what, names[0], names[1], d.max(), (d > 0).sum(), d.size))
    at = np.unravel_index(d.argmax(), d.shape)
    assert d.max() <= 1, "%s %s: weights of %s and %s differ by %d fp32 ulp at (utterance, frame, bin) %s: %r against %r" % (
        case["name"], what, names[0], names[1], d.max(), at, a[1][at], b[1][at])


@pytest.mark.parametrize("case", PC.ZEL_REG_CASES, **_ID)
def test_zelinski_registers_against_sum(dsr, oracle, cuda, monkeypatch, case):
    """every density kept and summed in the reference's pair order, against the recursion of the sum over 16 stretches: 1e-13 relative in fp64"""
    for what, (a, b) in zip(("one shot", "carried blocks"),
                            _twins(dsr, oracle, cuda, monkeypatch, case, {}, (PC.ZEL_REG, case["C"]), PC.SUM, (PC.ZEL_SUM, 0))):
        _one_ulp(case, what, ("k_zelinski_reg<%d>" % case["C"], "k_zel_pairs + k_zel_recur"), a, b)


@pytest.mark.parametrize("case", PC.ZEL_WAVE_CASES + PC.MC_WAVE_CASES[2:] + PC.LF_WAVE_CASES[2:], **_ID)
def test_threads_against_wave(dsr, oracle, cuda, monkeypatch, case):
    """a thread per (utterance, bin) summing in the reference's pair order, against a wavefront per (utterance, bin) summing in a tree: 1e-15 relative in fp64"""
    assert case["env"] == PC.WAVE_ENV and case["C"] in PC.REG_SET
    thread = (PC.ZEL_REG, case["C"]) if case["kind"] == 0 else (PC.MCCOWAN_REG, case["C"])
    for what, (a, b) in zip(("one shot", "carried blocks"),
                            _twins(dsr, oracle, cuda, monkeypatch, case, {}, thread, PC.WAVE_ENV, (PC.WAVE, case["kind"]))):
        _one_ulp(case, what, (PC.CELL_NAMES[thread[0]], "k_pf_wave<%d>" % case["kind"]), a, b)


@pytest.mark.parametrize("case", PC.ZEL_BF_CASES, **_ID)
def test_fused_against_two_calls(dsr, oracle, cuda, monkeypatch, case):
    """the beamformer's sum formed in k_zel_pairs<true> against dsr_bf_apply_frames followed by the filter (DSR_PF_NOFUSE), at the bars of
    test_zelinski_postfilter_behind_its_beamformer: beamformer output 2e-6 of its largest value, filtered output 1e-5 of its largest value, weights 1e-5"""
    res = []
    for env, cell in (({}, (PC.ZEL_SUM_BF, 0)), (PC.NOFUSE, (PC.ZEL_SUM, 0))):
        _set_env(monkeypatch, env)
        r = _Run(dsr, oracle, cuda, case)
        r.cell(cell)
        one = r.apply()
        r.pf.carry(True)
        parts = [r.apply(lo, hi) for lo, hi in case["blocks"]]
        res.append((one, tuple(np.concatenate([p[i] for p in parts], axis=1) for i in range(3))))
    for what, (a, b) in zip(("one shot", "carried blocks"), zip(*res)):
        eY = np.abs(a[2] - b[2]).max() / np.abs(b[2]).max(); eo = np.abs(a[0] - b[0]).max() / np.abs(b[0]).max(); ew = np.abs(a[1] - b[1]).max()
        print("%s %s, fused against two calls: beamformer output %.3g (bar 2e-6), filtered output %.3g (bar 1e-5), weights %.3g (bar 1e-5)" % (case["name"], what, eY, eo, ew))
        assert eY <= 2e-6 and eo <= 1e-5 and ew <= 1e-5
