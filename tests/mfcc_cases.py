"""Inputs shared by tests/test_mfcc_cases_cpu.py and tests/test_gpu_mfcc_kernels.py: the configurations that reach every kernel dsr_mfcc_run
(csrc/k_mfcc.hip) can select, on both sides of every size gate of its dispatch, and the ragged batches they run on.

A case is a dict:
  name     its id
  cfg      the full dsr_mfcc_cfg as keywords (DEFAULTS overridden)
  frames   what each utterance of the batch is: "empty" (0 samples), "short" (blockLen - 1 samples: no frame without padZeros), or the number of
           frames SampleFeature cuts from it (the shortest sample count that gives it, so the last frame always reads up to the last sample and,
           with padZeros, past it)
  silence  (utterance, first frame, last frame) spans of digital silence, or (utterance, None, None) for a silent utterance
  expect   (frames, cmn, lda) kernel the case is there to launch, None where the case does not care; the values of dsr.h's DSR_MFCC_* enums
  gates    {formula name: True (within its gate) / False (past it)} for the size formulas the choice rests on; test_mfcc_cases_cpu.py states
           the formulas and shows each falls on the named side
  env      the switches the case sets (monkeypatch)
Samples are slices of the committed headset recording (int16 range)."""
import numpy as np

FRAMES_PLAIN, FRAMES_W = 0, 1                                   # dsr.h: DSR_MFCC_FRAMES_*
CMN_NONE, CMN_PLAIN, CMN_LDS = 0, 1, 2                          # DSR_MFCC_CMN_*
LDA_TOO_LARGE, LDA_SPLICE, LDA_PLAIN, LDA_B = -1, 0, 1, 2       # DSR_MFCC_LDA_*

DEFAULTS = dict(blockLen=320, shiftLen=160, padZeros=0, mu=0.95, fftLen=512, powN=257, vtlnRatio=1.0, vtlnEdge=1.0, vtlnVersion=1,
                rate=16000.0, low=0.0, up=0.0, filterN=30, melVersion=1, logM=1.0, logA=1.0, sphinxFlooring=0, ncep=13, dctType=1,
                cmnMode=1, devNormFactor=0.0, delta=7, outDim=0)

# The project's tolerances (test_mfcc_chain): power relative in that test's form, log-mel absolute, cepstra / normalised cepstra / features absolute.
PROJECT_TOL = {4: 1e-5, 3: 1e-5, 1: 1e-4, 2: 1e-4, 0: 1e-4}
# FFT lengths other than 256 and 512: the oracle's radix-2 FFT and the kernel's radix-4 FFT round differently in fp64.  Maximum error of each
# stage against the oracle as measured on an MI355X on the cases below: none -- the difference does not survive the rounding of
# the power spectrum to fp32 on any frame of any case, and every later stage is then the oracle's bits.  The assert is twice the measurement
# (never looser than ten times the project's figure), so at these lengths it asks for the oracle's bits.
MEASURED = {
    32: {4: 0.0, 3: 0.0, 1: 0.0},
    64: {4: 0.0, 3: 0.0, 1: 0.0},
    128: {4: 0.0, 3: 0.0, 1: 0.0, 2: 0.0, 0: 0.0},
    1024: {4: 0.0, 3: 0.0, 1: 0.0, 2: 0.0, 0: 0.0},
    2048: {4: 0.0, 3: 0.0, 1: 0.0},
    4096: {4: 0.0, 3: 0.0, 1: 0.0},
}


def tol(fftLen, stage):
    if fftLen in (256, 512):
        return PROJECT_TOL[stage]
    return min(2.0 * MEASURED[fftLen][stage], 10.0 * PROJECT_TOL[stage])


def stage_error(got, ref, stage):
    """the error figure of test_mfcc_chain: stage 4 relative to |ref| + 1e-3 max(ref) of the utterance, the other stages absolute"""
    if ref.size == 0:
        return 0.0
    got = got.astype(np.float64); ref = ref.astype(np.float64)
    if stage == 4:
        return float((np.abs(got - ref) / (np.abs(ref) + 1e-3 * ref.max() + 1e-300)).max())
    return float(np.abs(got - ref).max())


def _case(name, frames, expect=(None, None, None), gates=None, env=None, silence=(), **kw):
    unknown = set(kw) - set(DEFAULTS)
    assert not unknown, unknown
    return dict(name=name, cfg=dict(DEFAULTS, **kw), frames=list(frames), expect=tuple(expect), gates=dict(gates or {}), env=dict(env or {}),
                silence=list(silence))


def oracle_kw(case):
    """keywords of oracle.mfcc_cfg for the case: the oracle's chain has no cmnMode (batch always; run-on is oracle.cmn_runon) and applies the
    pre-emphasis whatever mu is -- a negative mu switches the operator off on the device (dsr.h), which is the chain with mu = 0 (b - 0 prior = b)"""
    kw = {k: v for k, v in case["cfg"].items() if k != "cmnMode"}
    if kw["mu"] < 0:
        kw["mu"] = 0.0
    return kw


def lda_of(case):
    """the case's transform [outDim][(2 delta + 1) ncep], or None"""
    c = case["cfg"]
    if c["outDim"] <= 0:
        return None
    W = (2 * c["delta"] + 1) * c["ncep"]
    rng = np.random.default_rng(1234 + 7 * c["outDim"] + W)
    return (rng.standard_normal((c["outDim"], W)) / np.sqrt(W)).astype(np.float32)


def raw_frames(n, c):
    """SampleFeature's frame count (feature.cc:619-653)"""
    if c["padZeros"]:
        return (n + c["shiftLen"] - 1) // c["shiftLen"]
    return max(0, -(-(n - c["blockLen"]) // c["shiftLen"]))


def chain_frames(n, c):
    """frames the whole chain yields: AdjacentFeature needs delta frames to prime (feature.cc:2861-2866)"""
    T = raw_frames(n, c)
    return 0 if (c["delta"] > 0 and T < c["delta"]) else T


def samples_for(spec, c):
    if spec == "empty":
        return 0
    if spec == "short":
        return c["blockLen"] - 1
    assert spec >= 1
    return (spec - 1) * c["shiftLen"] + 1 + (0 if c["padZeros"] else c["blockLen"])


def lens_of(case):
    return [samples_for(s, case["cfg"]) for s in case["frames"]]


def tmax_of(case):
    return max(1, max(raw_frames(n, case["cfg"]) for n in lens_of(case)))


def batch(case, headset):
    """-> (y float32 [U][max length], lens): utterance u is a slice of the recording from sample 1000 + 500 u (earlier where it would not fit)"""
    c = case["cfg"]; lens = lens_of(case)
    y = np.zeros((len(lens), max(max(lens), 1)), np.float32)
    for u, n in enumerate(lens):
        off = min(1000 + 500 * u, len(headset) - n)
        assert off >= 0, (case["name"], n)
        y[u, :n] = headset[off:off + n]
    for u, a, b in case["silence"]:
        if a is None:
            y[u, :] = 0.0
        else:
            y[u, a * c["shiftLen"]: b * c["shiftLen"] + c["blockLen"]] = 0.0
    return y, lens


# ------------------------------------------------------------------------------------------------ frames kernels
RAGGED41 = ["empty", "short", 1, 3, 41]            # 41: not a multiple of the 4 (2 at fftLen 4096) frames of a workgroup

# k_mfcc_frames<FFTN> at the lengths only it serves: blockLen below fftLen and no multiple of 64, few enough filters that each keeps a tap
PLAIN_FFT = [
    _case("plain32", RAGGED41, (FRAMES_PLAIN, None, None), fftLen=32, powN=17, blockLen=25, shiftLen=10, filterN=6, ncep=5),
    _case("plain64", RAGGED41, (FRAMES_PLAIN, None, None), fftLen=64, powN=33, blockLen=50, shiftLen=20, filterN=10, ncep=8),
    _case("plain128", RAGGED41, (FRAMES_PLAIN, None, None), fftLen=128, powN=65, blockLen=100, shiftLen=40, filterN=16, ncep=10),
    _case("plain1024", RAGGED41, (FRAMES_PLAIN, None, None), {"ldsW": False}, fftLen=1024, powN=513, blockLen=800, shiftLen=400),
    _case("plain2048", RAGGED41, (FRAMES_PLAIN, None, None), fftLen=2048, powN=1025, blockLen=1500, shiftLen=700, filterN=40),
    _case("plain4096", RAGGED41, (FRAMES_PLAIN, None, None), fftLen=4096, powN=2049, blockLen=3000, shiftLen=1500, filterN=40),
]

F256 = dict(fftLen=256, powN=129, blockLen=200, shiftLen=80, filterN=24)
# k_mfcc_frames<256> / <512>: by the switch, and with no switch through tables too large for the 52 KB gate (ncep x filterN DCT entries in LDS)
PLAIN_256_512 = [
    _case("plain256_switch", RAGGED41, (FRAMES_PLAIN, None, None), {"ldsW": True}, {"DSR_MFCC_PLAIN": "1"}, **F256),
    _case("plain512_switch", RAGGED41, (FRAMES_PLAIN, None, None), {"ldsW": True}, {"DSR_MFCC_PLAIN": "1"}),
    _case("plain256_tables", RAGGED41, (FRAMES_PLAIN, None, None), {"ldsW": False}, **dict(F256, filterN=40, ncep=200)),
    _case("plain512_tables", RAGGED41, (FRAMES_PLAIN, None, None), {"ldsW": False}, filterN=40, ncep=48),
]
# the last ncep at filterN 40 whose tables still fit: one cepstrum more (160 bytes of DCT row) and the plain kernel runs
W_GATE = [_case("w512_gate_inside", RAGGED41, (FRAMES_W, None, None), {"ldsW": True, "ldsW_next": False}, filterN=40, ncep=45),
          _case("plain512_gate_outside", RAGGED41, (FRAMES_PLAIN, None, None), {"ldsW": False}, filterN=40, ncep=46)]


def _ragged(Tmax):
    return ["empty", "short", 1, min(3, Tmax), Tmax]


_VT1 = dict(vtlnRatio=1.1, vtlnEdge=0.8, vtlnVersion=1)
_VT2 = dict(vtlnRatio=0.9, vtlnEdge=0.8, vtlnVersion=2)
_W = (FRAMES_W, None, None)
# k_mfcc_frames_w<512, 8> / <256, 8>: a workgroup is 4 waves x 8 frames, so Tmax 1 / 31 / 32 / 33 / 65 end inside the first wave's run, one short
# of a workgroup, on it, one past it and one past two; block lengths that end inside a 64-lane run (200, 400), on one (320) and at fftLen; shifts
# below, at and past the block length (past it the carried pre-emphasis prior is a sample no frame holds).  One case per edge, then combined ones.
W_CASES = [
    _case("w512_T1", _ragged(1), _W),
    _case("w512_T31_b200", _ragged(31), _W, blockLen=200, shiftLen=80),
    _case("w512_T32_b400_mu_off", _ragged(32), _W, blockLen=400, shiftLen=160, mu=-1.0),
    _case("w512_T33_b512_s512", _ragged(33), _W, blockLen=512, shiftLen=512),
    _case("w512_T65_s357", _ragged(65), _W, blockLen=320, shiftLen=357),
    _case("w512_T33_pad", _ragged(33), _W, blockLen=400, shiftLen=160, padZeros=1),
    _case("w512_T33_powN512", _ragged(33), _W, blockLen=200, shiftLen=237, powN=512, up=7000.0),
    _case("w512_T65_vtln1", _ragged(65), _W, blockLen=400, shiftLen=80, **_VT1),
    _case("w512_T33_vtln2", _ragged(33), _W, **_VT2),
    _case("w512_T33_sphinx", _ragged(33), _W, silence=[(4, 5, 14), (3, None, None)], sphinxFlooring=1),
    _case("w512_T65_combined", _ragged(65), _W, blockLen=512, shiftLen=549, padZeros=1, mu=-1.0, powN=512, up=7000.0, melVersion=2, **_VT2),
    _case("w256_T1", _ragged(1), _W, **F256),
    _case("w256_T31_b256_s256", _ragged(31), _W, **dict(F256, blockLen=256, shiftLen=256)),
    _case("w256_T32_s237_mu_off", _ragged(32), _W, **dict(F256, shiftLen=237, mu=-1.0)),
    _case("w256_T33_pad", _ragged(33), _W, **dict(F256, shiftLen=160, padZeros=1)),
    _case("w256_T65_b256", _ragged(65), _W, **dict(F256, blockLen=256)),
    _case("w256_T33_powN256", _ragged(33), _W, **dict(F256, powN=256, up=7000.0)),
    _case("w256_T33_vtln1", _ragged(33), _W, **dict(F256, **_VT1)),
    _case("w256_T65_vtln2", _ragged(65), _W, **dict(F256, **_VT2)),
    _case("w256_T33_sphinx", _ragged(33), _W, silence=[(4, 5, 14), (3, None, None)], **dict(F256, sphinxFlooring=1)),
    _case("w256_T65_combined", _ragged(65), _W, **dict(F256, blockLen=256, shiftLen=293, padZeros=1, mu=-1.0, powN=256, up=7000.0, melVersion=2, **_VT1)),
]
FRAME_CASES = PLAIN_FFT + PLAIN_256_512 + W_GATE + W_CASES

# ------------------------------------------------------------------------------------------------ mean normalisation
# Front end k_mfcc_frames_w<256, 8>.  With dctType 1 the DCT row k = filterN is cos(pi (l + 0.5)) = 0 up to rounding: that cepstral dimension is
# constant, its variance below the 1e-4 floor.  Utterance 4 is digital silence (every dimension constant).
def _cmn_frames(Tmax):
    return ["empty", "short", 1, 3, min(20, Tmax), Tmax]


def _cmn(name, Tmax, expect, gates, env=None, **kw):
    return _case(name, _cmn_frames(Tmax), (None, expect, None), gates, env, [(4, None, None)], **dict(F256, shiftLen=20, **kw))


CMN_CASES = [
    _cmn("cmn_lds_n64_T256", 256, CMN_LDS, {"ldsC": True}, ncep=64),                              # 256 * 64 * 4 = 65 536 bytes: on the gate
    _cmn("cmn_lds_n64_T256_dev", 256, CMN_LDS, {"ldsC": True}, ncep=64, devNormFactor=2.0),
    _cmn("cmn_plain_n64_T257", 257, CMN_PLAIN, {"ldsC": False}, ncep=64, devNormFactor=2.0),
    _cmn("cmn_plain_n65", 40, CMN_PLAIN, {"ldsC": True}, ncep=65),                                # the LDS kernel keeps 64 means
    _cmn("cmn_plain_n65_dev", 40, CMN_PLAIN, {"ldsC": True}, ncep=65, devNormFactor=2.0),
    _cmn("cmn_lds_n13_T1260", 1260, CMN_LDS, {"ldsC": True}, ncep=13, devNormFactor=2.0),         # 65 520 bytes
    _cmn("cmn_plain_n13_T1261", 1261, CMN_PLAIN, {"ldsC": False}, ncep=13, devNormFactor=2.0),    # 65 572 bytes
    _cmn("cmn_plain_n13_T1261_nodev", 1261, CMN_PLAIN, {"ldsC": False}, ncep=13),
    _cmn("cmn_lds_n40_T33", 33, CMN_LDS, {"ldsC": True}, ncep=40, devNormFactor=0.5),             # ncep > filterN, far inside the gate
    _cmn("cmn_runon", 257, CMN_PLAIN, {"ldsC": True}, ncep=13, cmnMode=2),
    _cmn("cmn_runon_dev", 257, CMN_PLAIN, {"ldsC": True}, ncep=13, cmnMode=2, devNormFactor=3.0),
    _cmn("cmn_runon_T600", 600, CMN_PLAIN, {"ldsC": True}, ncep=13, cmnMode=2, devNormFactor=3.0),   # past the 500 frames where the forgetting factor changes
]


# ------------------------------------------------------------------------------------------------ splice + linear transform
def _lda_frames(delta, FB, Tmax):
    f = ["empty", "short", 1]
    if delta > 1:
        f.append(delta - 1)                        # T < delta: AdjacentFeature is never primed, no frame
    if delta > 0:
        f.append(delta)                            # T == delta: every slot of every frame clamps
    f.append(min(Tmax, (FB if FB < Tmax else 0) + 11))     # ends inside an 8-frame run (of the second group where there is one)
    f.append(Tmax)
    return f


def _lda(name, outDim, ncep, delta, Tmax, expect, gates, env=None, FB=None, **kw):
    if FB is None:
        FB = 8 * (256 // outDim) if outDim <= 256 else 64
    cfg = dict(F256, outDim=outDim, ncep=ncep, delta=delta, **kw)
    return _case(name, _lda_frames(delta, FB, Tmax), (None, None, expect), gates, env, **cfg)


def _lda_b(outDim, ncep, delta, **kw):
    """k_splice_lda_b<8> with nG = 256 / outDim groups: Tmax one short of, on and one past the 4 blocks of FB = 8 nG frames a workgroup walks"""
    FB = 8 * (256 // outDim)
    return [_lda("ldab_o%d_n%d_d%d_T%d" % (outDim, ncep, delta, T), outDim, ncep, delta, T, LDA_B, {"ldsB": True}, **kw)
            for T in (4 * FB - 1, 4 * FB, 4 * FB + 1)]


LDA_B_CASES = (
    _lda_b(39, 13, 7)                              # nG 6 (22 idle threads), Np padded
    + _lda_b(64, 12, 7)                            # nG 4, Np = ncep; 49 KB of the 52
    + _lda_b(100, 16, 1)                           # nG 2 (56 idle threads)
    + _lda_b(128, 13, 1)                           # nG 2
    + _lda_b(256, 12, 1)                           # nG 1
    + _lda_b(256, 16, 0)[2:]                       # no splice at all
    + _lda_b(39, 14, 2)[2:] + _lda_b(39, 15, 2)[2:]   # ncep = 2, 3 mod 4: the other two of the k4 + 1 / + 2 / + 3 < N guards end a row
    + _lda_b(1, 4, 7, shiftLen=16)                 # nG 256: a thread per frame run, FB = 2048
)
LDA_PLAIN_CASES = [
    _lda("lda_plain_o257", 257, 13, 1, 129, LDA_PLAIN, {"lds2": True}),                             # no group of 257 threads in a workgroup
    _lda("lda_plain_o64_n16_d7", 64, 16, 7, 129, LDA_PLAIN, {"ldsB": False, "lds2": True}),         # ldsB 62 KB
    _lda("lda_plain_o64_n14_d7", 64, 14, 7, 65, LDA_PLAIN, {"ldsB": False, "lds2": True}),
    _lda("lda_plain_o1_n13", 1, 13, 0, 70, LDA_PLAIN, {"ldsB": False, "lds2": True}),               # nG 256: 2048 input rows of 16 floats do not fit
    _lda("lda_splice_only", 0, 13, 7, 129, LDA_SPLICE, {}, FB=64),
]
LDA_TOO_LARGE_CASE = _lda("lda_too_large", 200, 16, 7, 20, LDA_TOO_LARGE, {"ldsB": False, "lds2": False})
LDA_CASES = LDA_B_CASES + LDA_PLAIN_CASES

# ------------------------------------------------------------------------------------------------ whole chain
CHAIN_CASES = [
    _case("chain_w512", ["empty", "short", 1, 6, 7, 59, 193], (FRAMES_W, CMN_LDS, LDA_B), blockLen=400, shiftLen=160, padZeros=1,
          devNormFactor=2.0, outDim=39, **_VT2),
    _case("chain_w256", ["empty", "short", 1, 75, 129], (FRAMES_W, CMN_LDS, LDA_B), **dict(F256, shiftLen=237, mu=-1.0, delta=1, outDim=100, ncep=16)),
    _case("chain_plain1024", ["empty", "short", 1, 6, 7, 41, 70], (FRAMES_PLAIN, CMN_LDS, LDA_PLAIN), fftLen=1024, powN=513, blockLen=800,
          shiftLen=400, outDim=64, ncep=16, devNormFactor=2.0),
    _case("chain_plain128", ["empty", "short", 1, 6, 7, 41, 70], (FRAMES_PLAIN, CMN_PLAIN, LDA_SPLICE), fftLen=128, powN=65, blockLen=100,
          shiftLen=40, filterN=16, ncep=65, delta=7),
]

ALL_CASES = FRAME_CASES + CMN_CASES + LDA_CASES + [LDA_TOO_LARGE_CASE] + CHAIN_CASES
assert len({c["name"] for c in ALL_CASES}) == len(ALL_CASES)
