"""Inputs shared by tests/test_srp_cases_cpu.py and tests/test_gpu_srp_kernels.py: one case for every cell the dispatches of the fp64-MFMA
steered-response-power kernels and of the multi-beam apply can select (csrc/k_sph.hip, csrc/k_doa.hip, csrc/srp_common.h), and the ragged batch
each runs on.  This is the one list of the channel counts that are no multiple of the MFMA's K step of 4 (tests/sph2_cases.py points here).

SPH_CASES   the spherical estimator (dsr_sph_srp); every case runs on the fused path and on the folded one
  name      its id: t<TG>d<DT> of the k_sph_srp<TG, DT> it is there for, the channel count, the eigenbeam rows
  kind, C, maxOrder (dim = maxOrder^2), grid (a key of GRIDS), rng (fbinMin, fbinMax), nBest, extra (sigma2, normalizeWeight, wgain)
  expect    (TG, DT, BC, KS) of the fused launch: what dsr_sph_srp_cell returns with DSR_SPH_SRP_PATH=fused
DOA_CASES   the linear estimator (dsr_doa_srp): name, C, nTheta, rng, nBest, expect (TG, BC, KS) of k_doa_srp<TG> (dsr_doa_srp_cell)
BEAM_CASES  dsr_sph_beams: (C, NB, kernel, kind, maxOrder, T, expect) with expect = dsr_sph_beams_cell's (0, rows, CC) or (1, BCT, KS)
APPLY_CASES dsr_sph_apply (k_sph_apply, eigenbeams 8 at a time): (kind, C, maxOrder)

Shapes: fftLen 64 (33 bins), 70 frames = two 64-frame workgroup tiles with a partial second one, three utterances: full, one that ends
inside the first tile (its second workgroup exits at once), one frame.  The smallest at which every path named above still differs."""
import numpy as np

from tests import doa_srp_np as D
from tests import sph_np as S
from tests.test_gpu_doa import _snapshots

FS = 16000
M, T, U = 64, 70, 3
F = M // 2 + 1
NFRAMES = [T, 41, 1]
SILENT = [(0, 10, 20), (1, 30, 36)]                            # planted silent stretches (utterance, from, to): the frames the gate must take
LDS_ROWS = 128                                                 # csrc/srp_common.h

# search grids on theta in [0, pi], phi in [-pi, pi]: (widthTheta, widthPhi, nTheta x nPhi as grid_n gives them), and the 1-unit grid of test_gpu_sph.py
GRIDS = {"u15": (1.2, 1.2, 3, 5), "u18": (1.0, 1.0, 3, 6), "u32": (0.8, 0.8, 4, 8), "u40": (0.6, 0.8, 5, 8), "u50": (0.6, 0.6, 5, 10),
         "u78": (0.5, 0.5, 6, 13), "u210": (0.3, 0.3, 10, 21), "u1": None}
ONE_UNIT = (0.5, 0.6, 1.0, 1.1, 0.1, 0.1)


def units_of(grid):
    return 1 if GRIDS[grid] is None else GRIDS[grid][2] * GRIDS[grid][3]


def _sph(name, kind, C, maxOrder, grid, rng, nBest, expect, **extra):
    return dict(name=name, kind=kind, C=C, maxOrder=maxOrder, grid=grid, rng=rng, nBest=nBest, expect=tuple(expect), extra=extra)


EB = dict(sigma2=0.05, normalizeWeight=True, wgain=1.5)        # the EigenBeamformer weights regularised, as test_gpu_sph.py runs them at order 8
SPH_CASES = [
    # TG 1 (NT 1: 15 units, a partial only tile)
    _sph("t1d1_c5_dim9", "DS", 5, 3, "u15", (3, 29), 2, (1, 1, 16, 2)),             # BC 16, 27 bins: a chunk of 11; C 5: K steps 2 with the last masked
    _sph("t1d2_c13_dim25", "EB", 13, 5, "u15", (1, 21), 5, (1, 2, 8, 4), **EB),     # BC 8, 21 bins; nBest 5 of 15 units
    _sph("t1d4_c25_dim36", "DS", 25, 6, "u15", (2, 12), 3, (1, 4, 4, 7)),           # BC 4 (padded rows), 11 bins; KS 7: 2+2+2+1; third tile partial, fourth empty
    # TG 2 (NT 2 and 3)
    _sph("t2d1_c27_dim16", "DS", 27, 4, "u18", (5, 9), 2, (2, 1, 2, 7)),            # BC 2, 5 bins; a full first tile of eigenbeams
    _sph("t2d2_c66_dim25", "DS", 66, 5, "u40", (7, 9), 4, (2, 2, 1, 17)),           # NT 3: the second workgroup has one tile; BC 1; KS 17: 8 pairs + 1
    _sph("t2d4_c128_dim49", "DS", 128, 7, "u32", (0, 32), 1, (2, 4, 1, 32)),        # 32 units: full tiles; LDS 65 536 exactly; fourth tile partial
    # TG 4 (NT 4 and 5)
    _sph("t4d1_c32_dim9", "EB", 32, 3, "u78", (0, 32), 3, (4, 1, 2, 8), **EB),      # the EigenMike; NT 5; the full range: both g = 1 bins
    _sph("t4d2_c5_dim25", "DS", 5, 5, "u50", (0, 32), 2, (4, 2, 16, 2)),            # NT 4; 33 bins at BC 16: chunks 16, 16, 1
    _sph("t4d4_c13_dim64", "DS", 13, 8, "u78", (1, 31), 2, (4, 4, 8, 4), normalizeWeight=True),   # all 64 rows; 31 bins at BC 8
    # TG 8 (NT 14: the second workgroup has 6 tiles)
    _sph("t8d1_c25_dim16", "DS", 25, 4, "u210", (4, 14), 2, (8, 1, 4, 7)),
    _sph("t8d2_c27_dim25", "EB", 27, 5, "u210", (0, 32), 3, (8, 2, 2, 7), **EB),
    _sph("t8d4_c66_dim36", "DS", 66, 6, "u210", (10, 20), 2, (8, 4, 1, 17)),
    _sph("t8d4_c128_dim49", "DS", 128, 7, "u210", (11, 15), 2, (8, 4, 1, 32)),      # the largest case: 128 channels x 210 units
]
# k_sph_frame's ranks beyond the units: nBest 3 on the 1-unit grid; nBest 5 on the 15-unit grid (every rank filled)
FRAME_CASES = [
    _sph("frame_1unit_nbest3", "EB", 5, 3, "u1", (3, 29), 3, (1, 1, 16, 2)),
    _sph("frame_15units_nbest5", "DS", 13, 3, "u15", (1, 21), 5, (1, 1, 8, 4)),
]
assert len({c["name"] for c in SPH_CASES + FRAME_CASES}) == len(SPH_CASES + FRAME_CASES)


def _doa(C, nTheta, rng, nBest, expect):
    return dict(name="c%d_n%d" % (C, nTheta), C=C, nTheta=nTheta, rng=rng, nBest=nBest, expect=tuple(expect))


DOA_CASES = [  # 17 directions: NT 2 (TG 2); 40: NT 3 (TG 2, ragged); 100: NT 7 (TG 4, ragged)
    _doa(5, 40, (3, 29), 3, (2, 16, 2)),
    _doa(13, 17, (1, 21), 2, (2, 8, 4)),
    _doa(25, 100, (2, 12), 4, (4, 4, 7)),                     # KS 7: the K-step ladder 4 + 2 + 1
    _doa(27, 40, (5, 9), 2, (2, 2, 7)),
    _doa(66, 100, (7, 9), 3, (4, 1, 17)),                     # KS 17: 4 x 4 + 1
    _doa(128, 17, (0, 32), 1, (2, 1, 32)),                    # LDS 65 536 exactly
    _doa(128, 100, (11, 15), 2, (4, 1, 32)),
]

VALU, MFMA = 0, 1
BEAM_CASES = [  # (C, NB, kernel, kind, maxOrder, T, expect)
    (25, 5, "mfma", "DS", 3, 37, (MFMA, 4, 7)),               # BCT 4 (padded rows); 11 zero-padded beam rows; K steps 4 + three singles, the last masked
    (16, 16, "mfma", "HWNC", 3, 37, (MFMA, 4, 4)),            # BCT 4 with full K steps and all 16 rows
    (66, 16, "mfma", "SPATIALDS", 2, 37, (MFMA, 1, 17)),      # BCT 1
    (128, 5, "mfma", "EB", 2, 70, (MFMA, 1, 32)),             # BCT 1 at 65 536 bytes of LDS; two frame tiles
    (66, 4, "valu", "DS", 3, 37, (VALU, 4, 23)),              # the staged table in channel chunks of 23, 23 and 20
]

APPLY_CASES = [("DS", 13, 5), ("EB", 66, 7), ("DS", 13, 7), ("EB", 66, 5)]   # dim 25 and 49: groups of 8 eigenbeams with a last group of 1


def geometry(Cn, seed=4):
    """(a, theta_s, phi_s): the EigenMike at 32 channels, else random sensors on a 42 mm sphere (tests/test_gpu_sph.py: _geometry)"""
    if Cn == 32:
        return S.eigenmike()
    rng = np.random.default_rng(seed)
    return 42.0, np.arccos(rng.uniform(-1, 1, Cn)), rng.uniform(0, 2 * np.pi, Cn)


def sph_handle(dsr, case):
    extra = dict(case["extra"])
    s = dsr.SphDoaSRP(case["kind"], case["nBest"], FS, M, case["C"], case["maxOrder"], normalizeWeight=extra.pop("normalizeWeight", False))
    if case["C"] == 32:
        s.setEigenMikeGeometry()
    else:
        s.setArrayGeometry(*geometry(case["C"]))
    if "sigma2" in extra:
        s.setSigma2(extra["sigma2"])
    if "wgain" in extra:
        s.setWeightGain(extra["wgain"])
    g = GRIDS[case["grid"]]
    s.setSearchParam(*(ONE_UNIT if g is None else (0.0, np.pi, -np.pi, np.pi, g[0], g[1])))
    s.setFrequencyRange(*case["rng"])
    return s


def doa_positions(Cn):
    return np.sort(np.random.default_rng(Cn).uniform(0, 2e-3, Cn + 1))


def doa_handle(dsr, case):
    d = dsr.DoaSRP(case["nBest"], FS, M, case["C"])
    d.setArrayGeometry(doa_positions(case["C"]))
    d.setSearchParam(0.0, np.pi, np.pi / case["nTheta"])
    d.setFrequencyRange(*case["rng"])
    return d


def snapshots(case):
    """X complex64 [U][C][T][F] with the planted silent stretches; the seed from the case"""
    seed = case["C"] * 3 + case["rng"][0] * 7 + case.get("maxOrder", 0) + case.get("nTheta", 0)
    return _snapshots(U, case["C"], T, M, seed=seed, silent=SILENT)


def planted():
    """[U][T] bool: the live frames inside a silent stretch"""
    p = np.zeros((U, T), bool)
    for u, a, b in SILENT:
        p[u, a:min(b, NFRAMES[u])] = True
    return p


def live():
    return np.arange(T)[None, :] < np.array(NFRAMES)[:, None]


def gate_threshold(X, fbinMin, fbinMax):
    """-> (threshold, energy [U][T]): the float32 geometric mean of the loudest planted frame and the quietest other live one, from the restatement's
    calcEnergy alone (tests/doa_srp_np.py: energy)"""
    e = np.stack([D.energy(X[u], fbinMin, fbinMax, M) for u in range(U)])
    p, l = planted(), live()
    return float(np.float32(np.sqrt(float(e[p].max()) * float(e[l & ~p].min())))), e
