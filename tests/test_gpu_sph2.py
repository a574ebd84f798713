"""The multi-beam apply (dsr_sph_beams: the VALU kernel up to 4 beams, the fp64-MFMA kernel above) and the five further stream classes on the
device against the numpy restatement tests/sph2_np.py.  The restatement takes the handle's own sensor-domain vectors (dsr_sph_beam_weights, held
to the host restatement by tests/test_sph2_np_cpu.py), so device parity is not confounded with table rounding.  Outputs are complex64 from fp64
accumulation: held to 2e-7 of the frame's largest value, the bound of tests/test_gpu_sph.py."""
import numpy as np
import pytest

from tests import sph2_np as S2
from tests.sph2_cases import BEAM_SHAPES, FS, LOOK, beam_dirs, geom_of, geometry, handle
from tests.test_gpu_doa import _snapshots
from tests.test_gpu_sph import _banks, _snap

pytestmark = pytest.mark.gpu
M, U = 64, 2


def _configure(dsr, kind, Cn, mo, NB):
    s = handle(dsr, kind, M, geom_of(Cn), mo, NC=1, ratio=0.3 if kind.startswith("HWNC") else None)
    dirs = beam_dirs(NB)
    s.setLookDirection(*dirs[0])
    for b in range(1, NB):
        s.setBeam(b, *dirs[b])
    if kind == "MOEN":
        for f in range(M // 2 + 1):
            s.setLevelOfDiagonalLoading(f, 1e-2)
    if kind in ("GSC", "HWNCGSC"):
        rng = np.random.default_rng(3)
        for f in (1, 9, M // 2):
            s.setActiveWeights_f(f, rng.standard_normal(2 * (s.dim - 1)) * 0.1)
    return s


def _check(y, ref, nframes):
    for u, N in enumerate(nframes):
        assert np.all(y[u, :, N:] == 0)                                      # rows beyond nframes are exactly 0
        scale = np.abs(ref[u, :, :N]).max(axis=2, keepdims=True)
        err = np.abs(y[u, :, :N] - ref[u, :, :N])
        print("u %d: max err / frame max = %.3e" % (u, float((err / scale).max())))
        assert np.all(err <= 2e-7 * scale)


@pytest.mark.parametrize("Cn,NB,kernel,kind,mo,T", BEAM_SHAPES)
def test_beams_match_restatement(dsr, cuda, Cn, NB, kernel, kind, mo, T):
    import torch
    assert ("valu", "mfma")[dsr.load().dsr_sph_beams_path(NB)] == kernel
    s = _configure(dsr, kind, Cn, mo, NB)
    X = _snapshots(U, Cn, T, M, seed=Cn + NB)
    nf = [T, 23 if T > 23 else 9]
    y = s.beams(torch.from_numpy(X).to(cuda), torch.tensor(nf, dtype=torch.int32, device=cuda), NB).cpu().numpy()
    assert y.shape == (U, NB, T, M // 2 + 1)
    _check(y, S2.beams(X, nf, s.beamWeights(NB)), nf)


@pytest.mark.parametrize("NB", [5, 16])
def test_valu_kernel_above_its_switch_point(dsr, cuda, monkeypatch, NB):
    """the zero-padded 8- and 16-row instantiations of the VALU kernel that the measurements compare the MFMA kernel with"""
    import torch
    monkeypatch.setenv("DSR_SPH_BEAMS_PATH", "valu")
    s = _configure(dsr, "HWNC", 32, 3, NB)
    X = _snapshots(U, 32, 40, M, seed=NB)
    nf = [40, 23]
    y = s.beams(torch.from_numpy(X).to(cuda), torch.tensor(nf, dtype=torch.int32, device=cuda), NB).cpu().numpy()
    _check(y, S2.beams(X, nf, s.beamWeights(NB)), nf)


@pytest.mark.parametrize("NB,Mb", [(2, 2048), (3, 2048), (1, 8192)])
def test_beams_at_the_valu_table_limit(dsr, cuda, NB, Mb):
    """the VALU kernel stages rows x F entries of conj(v) per channel in 48 KB: 2 x 1025 bins fit one channel at a time (4 chunks), 3 x 1025 and
    1 x 4097 fit none, and the call runs on the MFMA kernel instead of being refused"""
    import torch
    Cn, T, nf = 4, 17, [17, 9]
    s = handle(dsr, "HWNC", Mb, geom_of(Cn), 2, ratio=0.3)
    dirs = beam_dirs(NB)
    s.setLookDirection(*dirs[0])
    for b in range(1, NB):
        s.setBeam(b, *dirs[b])
    X = _snapshots(U, Cn, T, Mb, seed=NB)
    y = s.beams(torch.from_numpy(X).to(cuda), torch.tensor(nf, dtype=torch.int32, device=cuda), NB).cpu().numpy()
    assert y.shape == (U, NB, T, Mb // 2 + 1)
    _check(y, S2.beams(X, nf, s.beamWeights(NB)), nf)


def test_beams_from_nbest_equal_single_beam_calls(dsr, cuda):
    import torch
    Cn, mo, T = 32, 3, 40
    doa = handle(dsr, "DS", M, "em", mo, nBest=3, cls=dsr.SphDoaSRP)
    doa.setSearchParam(0.0, np.pi, -np.pi, np.pi, 0.4, 0.4)
    X = _snapshots(1, Cn, T, M, seed=77)
    Xd = torch.from_numpy(X).to(cuda)
    R, I = doa.finalNBest(doa.srp(Xd)["acc"])
    assert np.all(I[0] >= 0) and len(set(I[0])) == 3
    bf = handle(dsr, "HWNC", M, "em", mo, ratio=0.3)
    assert bf.setBeamsFromNBest(doa, I[0]) == 3
    y3 = bf.beams(Xd, None, 3).cpu().numpy()
    th, ph = doa.grid()
    for b, k in enumerate(I[0]):
        one = handle(dsr, "HWNC", M, "em", mo, ratio=0.3)
        one.setLookDirection(th[k], ph[k])
        y1 = one.beams(Xd, None, 1).cpu().numpy()
        assert np.all(np.abs(y3[0, b] - y1[0, 0]) <= 2e-7 * np.abs(y1[0, 0]).max(axis=1, keepdims=True))


STREAMS = [("SphericalHWNCBeamformerPtr", dict(maxOrder=2, ratio=0.3)), ("SphericalGSCBeamformerPtr", dict(maxOrder=2, normalizeWeight=True)),
           ("SphericalHWNCGSCBeamformerPtr", dict(maxOrder=2, ratio=1.0)), ("SphericalSpatialDSBeamformerPtr", dict(maxOrder=2)),
           ("SphericalMOENBeamformerPtr", dict(maxOrder=2))]


@pytest.mark.parametrize("cls,kw", STREAMS)
def test_stream_classes(dsr, cuda, protos, cls, kw):
    """pulled frame by frame, conjugate-mirrored upper bins included; the GSC classes: new active weights mid-stream apply from that frame on;
    reset() gives a second identical pass"""
    import dsr.btk.beamformer as BF
    Cn = 4
    xt = (np.random.default_rng(1).standard_normal((Cn, 128 * 60)) * 100).astype(np.float32)
    a, th, ph = geometry("rnd4")
    bf = getattr(BF, cls)(FS, 256, **kw)
    banks, Mb = _banks(protos, xt)
    for b in banks:
        bf.setChannel(b)
    bf.setArrayGeometry(a, th, ph); bf.setLookDirection(0.9, 2.0)
    gsc = "GSC" in cls
    if cls == "SphericalMOENBeamformerPtr":
        bf.setLevelOfDiagonalLoading(40, 1e-2)
    X, _ = _snap(protos, xt)
    h = bf._handle()
    ref = S2.beams(X[None], [X.shape[1]], h.beamWeights(1))[0, 0]
    change, ref2 = 20, None
    first = []
    for t, v in enumerate(bf):
        r = ref2 if ref2 is not None else ref
        scale = np.abs(r[t]).max()
        assert np.abs(v[: Mb // 2 + 1] - r[t]).max() <= 2e-7 * scale, t
        assert np.abs(v[Mb // 2 + 1:] - np.conj(r[t, 1:Mb // 2][::-1])).max() <= 2e-7 * scale, t
        if gsc and t == change - 1:                                          # between two pulls: frame `change` is the first with the new weights
            bf.setActiveWeights_f(30, np.linspace(-1, 1, 2 * (h.dim - 1)))
            ref2 = S2.beams(X[None], [X.shape[1]], h.beamWeights(1))[0, 0]
            assert np.abs(ref2[change, 30] - ref[change, 30]) > 1e-3 * np.abs(ref[change]).max()
        first.append(np.array(v))
    assert len(first) == X.shape[1] and len(first) >= 50
    second = [np.array(v) for v in bf]                                       # __iter__ resets
    assert len(second) == len(first)
    for t in range(len(first)):
        if not gsc or t >= change:
            assert np.array_equal(first[t], second[t]), t
