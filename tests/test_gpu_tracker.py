"""GPU tests of the spherical-array speaker trackers (csrc/k_tracker.hip, include/dsr.h section 2c'') against the numpy restatement
tests/tracker_np.py on the cases of tests/tracker_cases.py.

The bound on pos64 is max(64 s_case, 1e-12), s_case being the restatement's own float64-vs-long-double difference of the case
(tests/test_tracker_np_cpu.py prints it): the factor covers another summation order in reductions over up to 32 channels and 2N <= 550 rows.
The 2624 rows of spatial-lds64k are 4.8 times that, which would allow 64 ceil(2N / 550) = 320 s_case; measured on an MI355X the case differs
by 0.35 s_case (DESIGN.md 4.4n has the figures of every case), far below 64, so it keeps the factor 64 of the others.

k_trk_run is one workgroup of NT = 256 threads per utterance.  What the launch code and the kernel branch on, and the case that reaches it:

    branch or loop                                                    case
    F <= NT: a thread owns at most one bin                            every case with M = 32 (F = 17)
    F > NT in the observation loop over F L (modal, L = 9: 2313)      modal-F257
    F > NT in the observation loop over F L (spatial, L = 32: 8224)   spatial-F257
    F > NT in estimateBkl and in the O(F^2) rank selection            modal-F257, spatial-F257 (tests/test_tracker_np_cpu.py: bin 256 is kept)
    rank selection among equal |B|                                    modal-ties (255 bins of |B| = 0; the restatement keeps {200, 256, 0, 1}).  A bin of
                                                                      |B| = 0 adds only zero rows, so which zeros are kept shows in no output: the rule
                                                                      (lower bin first) is pinned on the CPU, here only that the ranking ends and keeps 200, 256
    a kept bin that is thread 0's second bin (256)                    modal-F257, spatial-F257, modal-ties
    2N <= NT rows: a thread owns at most one row of the sweep         modal-*-s4-* (2N = 72)
    2N > NT rows: the row loop of the sweep wraps                     modal-o3-s0-* (544), spatial-* (256 and more)
    LDS <= 64 KiB: launched without asking                            every case but one (at most 2N = 544 rows, 14 KiB)
    LDS > 64 KiB: hipFuncSetAttribute before the launch               spatial-lds64k (2N = 2624 rows, 70 824 bytes), also in blocks of frames
    setV blocks in the prearray (hasV)                                modal-setV, spatial-setV
    the clamp of theta                                                modal-clamp
    dsr_trk_create at max_rows and one bin past it                    tests/test_tracker_np_cpu.py (no kernel runs)"""
import numpy as np
import pytest

from tests import tracker_cases as Cs
from tests import tracker_np as T

pytestmark = pytest.mark.gpu


def make(dsr, case):
    trk = dsr.SphTracker(case["kind"], case["orderN"], case["M"], Cs.A_MM, Cs.FS, case["useSubbandsN"], Cs.SIGMA2_U, Cs.SIGMA2_V, Cs.SIGMA2_INIT, case["maxLocalN"])
    Vs = Cs.inputs(case)[2]
    if Vs is not None:
        for f in range(Cs.dims(case)[1]):
            trk.setV(Vs[f], f)
    if case["init"]:
        trk.setInitialPosition(*case["init"])
    return trk


def run_device(dsr, cuda, case, blocks=None, users=None):
    """the case on the device, in one call or in blocks of frames (a list of lengths); the mid-utterance nextSpeaker of a case splits there.
    -> (pos, pos64, info, final state) as numpy"""
    import torch
    _, _, U, TMAX, frames = Cs.dims(case)
    users = list(range(U)) if users is None else users
    X = torch.from_numpy(Cs.inputs(case)[1][users]).to(cuda)
    nf = np.array([frames[u] for u in users])
    trk = make(dsr, case)
    state = trk.newState(len(users), cuda)
    cuts = [0] + list(np.cumsum(blocks if blocks else [TMAX]))
    if case["mid"]:
        cuts = sorted(set(cuts + [case["mid"][0]]))
    pos, pos64, info = [], [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        if case["mid"] and a == case["mid"][0]:
            trk.nextSpeaker(); trk.setInitialPosition(*case["mid"][1]); trk.initState(state)
        n = torch.from_numpy(np.clip(nf - a, 0, b - a).astype(np.int32)).to(cuda)
        p, p64, i = trk.run(X[:, :, a:b, :].contiguous(), n, state)
        pos.append(p.cpu().numpy()); pos64.append(p64.cpu().numpy()); info.append(i.cpu().numpy())
    return np.concatenate(pos, 1), np.concatenate(pos64, 1), np.concatenate(info, 1), state.cpu().numpy()


@pytest.fixture(scope="module")
def device_runs(dsr, cuda):
    return {c["name"]: run_device(dsr, cuda, c) for c in Cs.CASES}


@pytest.mark.parametrize("case", Cs.CASES, ids=[c["name"] for c in Cs.CASES])
def test_batch_parity(case, device_runs):
    ref = Cs.reference(case)
    pos, pos64, info, _ = device_runs[case["name"]]
    r = ref["ref"]
    _, F, U, TMAX, frames = Cs.dims(case)
    rows = 2 * (case["useSubbandsN"] or F) * (T.CHAN if case["kind"] == "spatial" else (case["orderN"] + 1) ** 2)
    factor = 64                                                          # also for the 2624 rows of spatial-lds64k (module docstring)
    bound = max(factor * ref["s_case"], 1e-12)
    diff = np.abs(pos64 - r["pos64"].astype(np.float64)).max()
    truth = Cs.directions(case)
    err = lambda t: float(np.abs(pos64[0, t] - truth[0, t]).max())
    print("%s: 2N %d s_case %.3e bound %.3e (%d s_case) device difference %.3e = %.2f s_case; angular error frame 0 %.4f, last %.4f" % (
        case["name"], rows, ref["s_case"], bound, factor, diff, diff / ref["s_case"], err(0), err(frames[0] - 1)))
    assert np.array_equal(info, r["info"])
    assert diff <= bound
    assert np.array_equal(pos, pos64.astype(np.float32))
    for u in range(U):
        n = frames[u]
        assert not pos[u, n:].any() and not pos64[u, n:].any() and not info[u, n:].any()
    if case["name"] == "modal-clamp":
        assert (info & 0x100).any()                                      # the case is there for the clamp


def test_plane_wave_kernel(dsr, cuda):
    import torch
    case = Cs.CASES[0]
    src = Cs.inputs(case)[0].astype(np.complex64)
    trk = dsr.SphTracker("modal", Cs.SIM_ORDER, Cs.M, Cs.A_MM, Cs.FS)
    sim = dsr.PlaneWaveSim(trk, 0.6, 0.2)
    dec = Cs.sim_decomposition()
    ref = [T.PlaneWaveSimulator(dec, c, 0.6, 0.2) for c in range(T.CHAN)]
    assert np.abs(sim.coef - np.stack([r.coef for r in ref])).max() <= 1e-13 * np.abs(sim.coef).max()
    nf = torch.tensor(Cs.NFRAMES, dtype=torch.int32, device=cuda)
    full = sim.apply(torch.from_numpy(src).to(cuda), nf, full=True).cpu().numpy()
    half = sim.apply(torch.from_numpy(src).to(cuda), nf).cpu().numpy()
    assert np.array_equal(half, full[..., :Cs.F])
    for u in range(Cs.U):
        for t in range(Cs.TMAX):
            if t >= Cs.NFRAMES[u]:
                assert not full[u, :, t].any()
                continue
            for c in (0, 7, 31):
                want = ref[c].next(src[u, t].astype(np.complex128))
                assert np.abs(full[u, c, t] - want).max() <= 2e-7 * np.abs(want).max()
            k = np.arange(1, Cs.M // 2)
            assert np.array_equal(full[u, :, t, Cs.M - k], np.conj(full[u, :, t, k]))


@pytest.mark.parametrize("name", ["modal-o3-s0-l4", "spatial-o2-s4-l4", "modal-setV"])
def test_carried_state(name, dsr, cuda, device_runs):
    case = Cs.BY_NAME[name]
    one = device_runs[name]
    two = run_device(dsr, cuda, case, blocks=[5, 7])
    for a, b in zip(one, two):
        assert np.array_equal(a, b)


def test_carried_state_above_64k_of_lds(dsr, cuda, device_runs):
    """spatial-lds64k in blocks of 2 and 1 frames: every call sets the kernel's dynamic-LDS limit again, and the result is the single call's bit for bit"""
    case = Cs.BY_NAME["spatial-lds64k"]
    assert Cs.dims(case)[3] == 3
    two = run_device(dsr, cuda, case, blocks=[2, 1])
    for a, b in zip(device_runs[case["name"]], two):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["modal-o2-s4-l4", "spatial-o3-s6-l1"])
def test_utterance_independence(name, dsr, cuda, device_runs):
    case = Cs.BY_NAME[name]
    pos, pos64, info, state = device_runs[name]
    for u in (1, 2):
        p, p64, i, s = run_device(dsr, cuda, case, users=[u])
        assert np.array_equal(p64[0], pos64[u]) and np.array_equal(i[0], info[u]) and np.array_equal(p[0], pos[u]) and np.array_equal(s[0], state[u])


@pytest.mark.parametrize("kind", ["modal", "spatial"])
def test_stream_classes(kind, dsr, cuda):
    """the stream classes pulled frame by frame over PlaneWaveSimulatorPtr channels equal the batch call on the same data"""
    import torch
    from dsr.btk import beamformer as B
    from dsr.btk.stream import PyVectorComplexFeatureStreamPtr

    class Src:
        def __init__(self, rows):
            self.rows = rows

        def size(self):
            return Cs.M

        def reset(self):
            pass

        def __iter__(self):
            return iter(self.rows)

    Tn = 6
    src = Cs.inputs(Cs.CASES[0])[0][0, :Tn].astype(np.complex64)
    rows = np.zeros((Tn, Cs.M), np.complex128); rows[:, :Cs.F] = src
    simdec = B.ModalDecompositionPtr(Cs.SIM_ORDER, Cs.M, Cs.A_MM, Cs.FS)
    dec = (B.ModalDecompositionPtr if kind == "modal" else B.SpatialDecompositionPtr)(2, Cs.M, Cs.A_MM, Cs.FS, 4)
    trk = (B.ModalSphericalArrayTrackerPtr if kind == "modal" else B.SpatialSphericalArrayTrackerPtr)(dec, Cs.SIGMA2_U, Cs.SIGMA2_V, Cs.SIGMA2_INIT, 2)
    chans = [B.PlaneWaveSimulatorPtr(PyVectorComplexFeatureStreamPtr(Src(rows)), simdec, c, 0.65, 0.25) for c in range(32)]
    for c in chans:
        trk.setChannel(c)
    first = np.stack([np.array(trk.next()) for _ in range(Tn)])
    with pytest.raises(StopIteration):
        trk.next()
    # the batch call on the same data
    bt = dsr.SphTracker(kind, 2, Cs.M, Cs.A_MM, Cs.FS, 4, Cs.SIGMA2_U, Cs.SIGMA2_V, Cs.SIGMA2_INIT, 2)
    X = dsr.PlaneWaveSim(dsr.SphTracker("modal", Cs.SIM_ORDER, Cs.M, Cs.A_MM, Cs.FS), 0.65, 0.25).apply(torch.from_numpy(src[None]).to(cuda))
    pos, _, info = bt.run(X)
    assert np.array_equal(first, pos.cpu().numpy()[0]) and (info.cpu().numpy() & 0xff).all()
    # reset keeps the filter's state (the next pass starts where the first ended); nextSpeaker restores the initial output
    trk.reset()
    again = np.stack([np.array(trk.next()) for _ in range(Tn)])
    assert not np.array_equal(again, first)
    trk.nextSpeaker()
    third = np.stack([np.array(trk.next()) for _ in range(Tn)])
    assert np.array_equal(third, first)
