"""dsr_mfcc_run (csrc/k_mfcc.hip) at every kernel and size class its dispatch can select, on the ragged batches of tests/mfcc_cases.py (an utterance of
0 samples, one too short for a frame, one of exactly one frame, one with fewer frames than delta, one that sets Tmax;
tests/test_mfcc_cases_cpu.py shows the cases are what they are named for and that each size formula falls on the named side of its gate).

Every case asserts the kernels it means to launch through dsr_mfcc_paths (dsr.Mfcc.paths), the helper dsr_mfcc_run itself launches from.
What is compared:
  * stages 4 (power), 3 (log-mel), 1 (cepstra), 2 (normalised) and 0 (features) with oracle.mfcc_chain at the project's tolerances (power 1e-5
    relative in test_mfcc_chain's form, log-mel 1e-5, the others 1e-4 absolute) at fftLen 256 and 512; at the other FFT lengths the oracle's
    radix-2 FFT and the kernel's radix-4 FFT round differently, and the assert is twice the error measured on the GPU (mfcc_cases.MEASURED,
    DESIGN 4.4), never looser than ten times the project's figure;
  * rows past an utterance's last frame are exactly 0, and no output is ever not finite (the 0/0 mean of an empty utterance stays inside k_cmn);
  * each fast kernel returns its plain twin's bits (DSR_MFCC_PLAIN / DSR_CMN_PLAIN / DSR_LDA_PLAIN, read on every call);
  * each later stage alone has the reference's order of operations: the device's own cepstra through oracle.cmn_batch / cmn_runon are the
    device's stage 2 bit for bit, and its stage 2 through oracle.adjacent + oracle.sgemv_rows is its stage 0 bit for bit (both sides are built
    without FMA contraction: -ffp-contract=off in both Makefiles).

Template instance -> the case that launches it (lists in tests/mfcc_cases.py):
  k_mfcc_frames<32 | 64 | 128 | 1024 | 2048 | 4096>   test_frames_kernels[plain32 .. plain4096] (4096: two frames a workgroup, 128 KB of LDS)
  k_mfcc_frames<256>                                  [plain256_switch] (DSR_MFCC_PLAIN), [plain256_tables] (ldsW 54 KB), test_w_returns_plain_bits[w256_*]
  k_mfcc_frames<512>                                  [plain512_switch], [plain512_tables], [plain512_gate_outside] (ldsW 53 336 > 53 248),
                                                      test_w_returns_plain_bits[w512_*]
  k_mfcc_frames_w<256, 8>                             test_frames_kernels[w256_*]: the radix-2 tail of the N = 128 FFT; Tmax 1, 31, 32, 33, 65
  k_mfcc_frames_w<512, 8>                             test_frames_kernels[w512_*], [w512_gate_inside] (ldsW 53 176)
  k_mfcc_frames_w<1024, 8>                            none: removed, its tables never fit the 52 KB gate (5 * 1024 * 16 bytes = 80 KB alone)
  k_cmn_lds                                           test_cmn[cmn_lds_*] (n64_T256: exactly 64 KB)
  k_cmn, batch mode                                   test_cmn[cmn_plain_*] (Tmax 257 at 64 cepstra, 65 cepstra, Tmax 1261 at 13), test_cmn_lds_returns_plain_bits
  k_cmn, run-on                                       test_cmn[cmn_runon*]
  k_splice_lda_b<8>                                   test_splice_transform[ldab_*]: nG 256, 6, 4, 2, 2, 1; Tmax on, one short of and one past 4 FB frames
  k_splice_lda with a transform                       test_splice_transform[lda_plain_*], test_splice_lda_b_returns_plain_bits
  k_splice_lda without                                test_splice_transform[lda_splice_only], test_whole_chain[chain_plain128]
Run with -s for the measured error of every case and stage."""
import numpy as np
import pytest

from tests import mfcc_cases as MC

pytestmark = pytest.mark.gpu

SWITCHES = ("DSR_MFCC_PLAIN", "DSR_CMN_PLAIN", "DSR_LDA_PLAIN", "DSR_LDA_FB")
_ID = dict(ids=lambda c: c["name"])
_REF = {}                                                                      # (case, stage) -> the oracle's output per utterance, computed once


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _ref(oracle, case, y, lens, stage):
    key = (case["name"], stage)
    if key not in _REF:
        c = case["cfg"]
        cfg = oracle.mfcc_cfg(lda=MC.lda_of(case), **MC.oracle_kw(case))
        refs = []
        for u, n in enumerate(lens):
            if stage == 2 and c["cmnMode"] == 2:
                cep = oracle.mfcc_chain(y[u, :n], cfg, stage=1)
                refs.append(oracle.cmn_runon(cep, c["devNormFactor"]) if len(cep) else cep)
            else:
                refs.append(oracle.mfcc_chain(y[u, :n], cfg, stage=stage))
        for r in refs:
            r.setflags(write=False)
        _REF[key] = refs
    return _REF[key]


class _Run:
    """a case's plan and batch on the device"""

    def __init__(self, dsr, cuda, headset, case):
        import torch
        self.case = case; self.c = case["cfg"]
        self.y, self.lens = MC.batch(case, headset)
        self.Tmax = MC.tmax_of(case)
        self.T = [MC.raw_frames(n, self.c) for n in self.lens]
        self.mf = dsr.Mfcc(lda=MC.lda_of(case), **self.c)
        self.yd = torch.from_numpy(self.y).to(cuda)
        self.nd = torch.tensor(self.lens, dtype=torch.int32, device=cuda)

    def paths(self, expect=None):
        got = self.mf.paths(self.Tmax)
        for e, g in zip(expect or self.case["expect"], got):
            assert e is None or e == g, "%s: the dispatch takes kernels %s, the case is there for %s" % (self.case["name"], got, expect or self.case["expect"])
        return got

    def run(self, stage):
        out = self.mf.run(self.yd, self.nd, stage=stage).cpu().numpy()
        assert out.shape[:2] == (len(self.lens), self.Tmax)
        assert np.isfinite(out).all(), "%s stage %d: %d outputs are not finite" % (self.case["name"], stage, int((~np.isfinite(out)).sum()))
        return out

    def against_oracle(self, oracle, out, stage, T=None):
        """max error of the stage over the batch in test_mfcc_chain's form; asserts the tolerance and the zero rows"""
        refs = _ref(oracle, self.case, self.y, self.lens, stage)
        worst = 0.0
        for u, ref in enumerate(refs):
            Tu = (T or self.T)[u]
            assert ref.shape[0] == Tu, (u, ref.shape, Tu)
            assert np.all(out[u, Tu:] == 0), "%s stage %d: utterance %d has non-zero rows past its %d frames" % (self.case["name"], stage, u, Tu)
            worst = max(worst, MC.stage_error(out[u, :Tu], ref, stage))
        tol = MC.tol(self.c["fftLen"], stage)
        print("%s fftLen %d stage %d: max error %.3g (assert %.3g)" % (self.case["name"], self.c["fftLen"], stage, worst, tol))
        ok = worst < tol if self.c["fftLen"] in (256, 512) else worst <= tol  # (a measured error of 0 asks for equality)
        assert ok, "%s stage %d: error %.3g, tolerance %.3g" % (self.case["name"], stage, worst, tol)
        return worst


# ------------------------------------------------------------------------------------------------ frames kernels
@pytest.mark.parametrize("case", MC.FRAME_CASES, **_ID)
def test_frames_kernels(dsr, oracle, cuda, headset, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    r = _Run(dsr, cuda, headset, case)
    r.paths()
    for stage in (4, 3, 1):
        r.against_oracle(oracle, r.run(stage), stage)


@pytest.mark.parametrize("case", MC.W_CASES + MC.W_GATE[:1], **_ID)
def test_w_returns_plain_bits(dsr, cuda, headset, monkeypatch, case):
    """tables in LDS, wave-private frames, the neighbouring lane's sample as the pre-emphasis prior: the same bits as one wavefront per frame"""
    r = _Run(dsr, cuda, headset, case)
    _set_env(monkeypatch, {})
    r.paths((MC.FRAMES_W, None, None))
    fast = [r.run(stage) for stage in (4, 3, 1)]
    _set_env(monkeypatch, {"DSR_MFCC_PLAIN": "1"})
    r.paths((MC.FRAMES_PLAIN, None, None))
    for stage, a in zip((4, 3, 1), fast):
        b = r.run(stage)
        diff = np.argwhere(_bits(a) != _bits(b))
        assert len(diff) == 0, "%s stage %d: %d values differ between the two kernels, first (utterance, frame, index) %s" % (
            case["name"], stage, len(diff), diff[0])


# ------------------------------------------------------------------------------------------------ mean normalisation
def _cmn_of_device_cepstra(oracle, c, cep):
    if c["cmnMode"] == 2:
        return oracle.cmn_runon(cep, c["devNormFactor"])
    return oracle.cmn_batch(cep, c["devNormFactor"])[0]


@pytest.mark.parametrize("case", MC.CMN_CASES, **_ID)
def test_cmn(dsr, oracle, cuda, headset, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    r = _Run(dsr, cuda, headset, case)
    r.paths()
    cep = r.run(1); out = r.run(2)
    for u, Tu in enumerate(r.T):                                               # the stage alone: the reference's sums in the reference's order
        assert np.all(out[u, Tu:] == 0)
        if Tu:
            ref = _cmn_of_device_cepstra(oracle, r.c, cep[u, :Tu])
            diff = np.argwhere(_bits(out[u, :Tu]) != _bits(ref))
            assert len(diff) == 0, "%s utterance %d (%d frames): %d values are not the reference's bits, first (frame, dim) %s: %r against %r" % (
                case["name"], u, Tu, len(diff), diff[0], out[u][tuple(diff[0])], ref[tuple(diff[0])])
    r.against_oracle(oracle, out, 2)                                           # the chain up to here


@pytest.mark.parametrize("case", [c for c in MC.CMN_CASES if c["expect"][1] == MC.CMN_LDS], **_ID)
def test_cmn_lds_returns_plain_bits(dsr, cuda, headset, monkeypatch, case):
    r = _Run(dsr, cuda, headset, case)
    _set_env(monkeypatch, {})
    r.paths((None, MC.CMN_LDS, None))
    fast = r.run(2)
    _set_env(monkeypatch, {"DSR_CMN_PLAIN": "1"})
    r.paths((None, MC.CMN_PLAIN, None))
    assert np.array_equal(_bits(fast), _bits(r.run(2)))


# ------------------------------------------------------------------------------------------------ splice + linear transform
@pytest.mark.parametrize("case", MC.LDA_CASES, **_ID)
def test_splice_transform(dsr, oracle, cuda, headset, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    r = _Run(dsr, cuda, headset, case)
    r.paths()
    lda = MC.lda_of(case)
    cmn = r.run(2); out = r.run(0)
    Tc = [MC.chain_frames(n, r.c) for n in r.lens]
    for u, n in enumerate(r.lens):                                             # the stage alone: gsl_blas_sgemv's reference loop over the spliced rows
        assert r.mf.frames(n) == Tc[u]
        assert np.all(out[u, Tc[u]:] == 0), "utterance %d has non-zero rows past its %d frames" % (u, Tc[u])
        X = oracle.adjacent(cmn[u, :r.T[u]], r.c["delta"])
        ref = oracle.sgemv_rows(lda, X) if lda is not None else X
        assert ref.shape[0] == Tc[u]
        diff = np.argwhere(_bits(out[u, :Tc[u]]) != _bits(ref))
        assert len(diff) == 0, "%s utterance %d (%d frames): %d values are not the reference loop's bits, first (frame, dim) %s" % (
            case["name"], u, Tc[u], len(diff), diff[0])
    r.against_oracle(oracle, out, 0, Tc)                                       # the whole chain


@pytest.mark.parametrize("case", MC.LDA_B_CASES, **_ID)
def test_splice_lda_b_returns_plain_bits(dsr, cuda, headset, monkeypatch, case):
    r = _Run(dsr, cuda, headset, case)
    _set_env(monkeypatch, {})
    r.paths((None, None, MC.LDA_B))
    fast = r.run(0)
    _set_env(monkeypatch, {"DSR_LDA_PLAIN": "1"})
    r.paths((None, None, MC.LDA_PLAIN))
    assert np.array_equal(_bits(fast), _bits(r.run(0)))


def test_transform_too_large_is_an_error_status(dsr, cuda, headset, monkeypatch):
    """a transform that needs more than the 160 KB of LDS a CU has: DSR_E_DIMENSION from dsr_mfcc_run, no launch; the earlier stages still run"""
    _set_env(monkeypatch, {})
    case = MC.LDA_TOO_LARGE_CASE
    r = _Run(dsr, cuda, headset, case)
    assert r.paths()[2] == dsr.MFCC_LDA_TOO_LARGE
    r.run(2)
    with pytest.raises(dsr.DsrError) as e:
        r.run(0)
    assert e.value.status == dsr.E_DIMENSION and "LDS" in str(e.value)
    import torch
    torch.cuda.synchronize()                                                   # (nothing was launched that could fail later)


# ------------------------------------------------------------------------------------------------ whole chain
@pytest.mark.parametrize("case", MC.CHAIN_CASES, **_ID)
def test_whole_chain(dsr, oracle, cuda, headset, monkeypatch, case):
    _set_env(monkeypatch, case["env"])
    r = _Run(dsr, cuda, headset, case)
    assert r.paths() == case["expect"]
    Tc = [MC.chain_frames(n, r.c) for n in r.lens]
    assert [r.mf.frames(n) for n in r.lens] == Tc
    r.against_oracle(oracle, r.run(2), 2)
    r.against_oracle(oracle, r.run(0), 0, Tc)
