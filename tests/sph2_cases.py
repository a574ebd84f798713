"""Case lists shared by tests/test_sph2_np_cpu.py and tests/test_gpu_sph2.py (the further spherical-array beamformers)."""
import numpy as np

FS = 16000
LOOK = (1.0, 0.3)

# geometry, maxOrder: the EigenMike at orders 1, 4, 8 and a random 4-sensor sphere at order 2
GEOMS = [("em", 1), ("em", 4), ("em", 8), ("rnd4", 2)]


def geometry(name, seed=4):
    """(a, theta_s, phi_s)"""
    from tests import sph_np as S
    if name == "em":
        return S.eigenmike()
    rng = np.random.default_rng(seed)
    n = int(name[3:])
    return 42.0, np.arccos(rng.uniform(-1, 1, n)), rng.uniform(0, 2 * np.pi, n)


def handle(dsr, kind, M, geom, maxOrder, normalizeWeight=False, NC=1, ratio=None, nBest=1, cls=None):
    a, th, ph = geometry(geom)
    s = (cls or dsr.SphBeamformer)(kind, *(() if cls is None else (nBest,)), FS, M, len(th), maxOrder, normalizeWeight, False, NC, *(() if cls else (ratio,)))
    if geom == "em":
        s.setEigenMikeGeometry()
    else:
        s.setArrayGeometry(a, th, ph)
    return s


# the GPU shapes of dsr_sph_beams: (C, NB, kernel, kind, maxOrder, T)
BEAM_SHAPES = [
    (4, 1, "valu", "HWNC", 2, 40),
    (4, 3, "valu", "GSC", 2, 40),
    (32, 4, "valu", "SPATIALDS", 4, 40),
    (32, 5, "mfma", "MOEN", 4, 40),       # first NB on the MFMA path, 11 padded rows
    (32, 16, "mfma", "HWNCGSC", 4, 40),
    (64, 16, "mfma", "DS", 3, 40),
    (6, 7, "mfma", "EB", 2, 40),          # BCT 8 with a masked K step; the channel counts that are no multiple of 4: tests/srp_cases.py
    (32, 9, "mfma", "HWNC", 3, 17),       # T is no multiple of the 16-frame tile
    (32, 2, "valu", "MOEN", 3, 17),
]


def geom_of(Cn):
    return "em" if Cn == 32 else "rnd%d" % Cn


def beam_dirs(NB, seed=11):
    rng = np.random.default_rng(seed)
    return [(float(t), float(p)) for t, p in zip(rng.uniform(0.2, 2.9, NB), rng.uniform(-3, 3, NB))]
