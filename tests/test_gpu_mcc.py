"""GPU tests of the multichannel cross-correlation localiser (include/dsr.h section 2f) against the numpy restatement tests/mcc_np.py, which is
fed the tau table dsr_sgb_enumerate returned, so grid rounding cannot enter the comparison.

Tolerances: the lower-triangular R within 1e-12 max|R| (the project's fp64-against-numpy tolerance, test_gpu_doa.py); a cost within
tol = 8 C kappa 2.2e-16 with kappa from the restatement's own eigenvalues (the first-order bound on a log-determinant from eigenvalues or
pivots carrying absolute error eps ||R||, both sides having it); N-best grid indices equal wherever neighbouring costs differ by more than
2 tol (at most 2 % of the entries left out); tau and positions of the kept entries exactly equal; their eigenvalues within 1e-10 lambda_max.
tests/test_mcc_np_cpu.py checks that the inputs meet the conditions this relies on."""
import numpy as np
import pytest

from tests import mcc_cases as K
from tests import mcc_np as M
from tests.test_mcc_np_cpu import ALL

pytestmark = pytest.mark.gpu


def _t(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _grid(dsr, case):
    sg = K.configure(dsr.SearchGrid(case["kind"], case["C"], True, K.FS), case)
    pos, dl, tau = sg.enumerate()
    return sg, pos, dl, tau


@ALL
def test_mcc_batch_matches_restatement(dsr, cuda, i):
    import torch
    case = K.CASES[i]; Cn, S = case["C"], case["S"]
    sg, pos, dl, tau = _grid(dsr, case)
    loc = dsr.MccLocalizer(sg, S); D = loc.D
    assert D == K.np_grid(case).D() and loc.G == tau.shape[0]
    if i in K.MULTI_GROUP:                                                       # the loop over groups of candidates inside a workgroup runs more than once
        assert K.candidates_per_workgroup(loc.G, case["U"] * case["B"]) >= 8
    b = K.build(case, tau, D); L = b["L"]; ref = K.reference(case, b, tau, D); valid = K.valid_blocks(case, b)
    r = loc.run(_t(b["x"], cuda), L, _t(b["nsamples"], cuda), want_costmap=True, want_R=True)
    torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in r.items()}
    assert np.array_equal(r["valid"].astype(bool), valid)
    entries = left = 0
    for u in range(case["U"]):
        for k in range(case["B"]):
            if not valid[u, k]:                                                  # finite zeros
                for name in ("index", "cost", "tau", "position", "eig", "costmap", "R"):
                    assert not r[name][u, k].any(), (name, u, k)
                continue
            q = ref[(u, k)]
            if (u, k) == b["zero"]:
                assert not r["costmap"][u, k].any() and not r["cost"][u, k].any() and not r["eig"][u, k].any() and not r["R"][u, k].any()
                assert r["index"][u, k].tolist() == list(range(S))               # the tie rule: the first grid points
                continue
            print("case %d (%d, %d): max |cost - ref| / tol = %.3g, max |R - ref| / max|R| = %.3g" % (
                i, u, k, (np.abs(r["costmap"][u, k] - q["costs"]) / K.tolerance(Cn, q["kappa"])).max(), np.abs(r["R"][u, k] - q["Rlast"]).max() / np.abs(q["Rlast"]).max()))
            assert np.all(np.isfinite(r["costmap"][u, k]))
            assert np.all(np.abs(r["costmap"][u, k] - q["costs"]) <= K.tolerance(Cn, q["kappa"])), (u, k)
            assert np.abs(r["R"][u, k] - q["Rlast"]).max() <= 1e-12 * np.abs(q["Rlast"]).max() and not np.triu(r["R"][u, k], 1).any()
            cmp_ok = K.comparable_entries(q, tau, Cn)
            for n, (c, g) in enumerate(q["best"]):
                entries += 1
                assert abs(r["cost"][u, k, n] - c) <= K.tolerance(Cn, q["kappa"][g])
                if not cmp_ok[n]:                                                # the index is open: the eigenvalues still are those of the entry the device kept
                    left += 1; gd = int(r["index"][u, k, n]); evd = np.sort(np.abs(M.eigenvalues(M.covariance(b["x"][u, :, k * L:(k + 1) * L], tau[gd], D))))
                    assert np.abs(r["eig"][u, k, n] - evd).max() <= 1e-10 * evd[-1], (u, k, n)
                    continue
                assert r["index"][u, k, n] == g, (u, k, n)
                assert np.array_equal(r["tau"][u, k, n], tau[g]) and np.array_equal(r["position"][u, k, n], pos[g])
                ev = q["eig"][g]
                print("   entry %d: max |eig - ref| / lambda_max = %.3g" % (n, np.abs(r["eig"][u, k, n] - ev).max() / ev[-1]))
                assert np.abs(r["eig"][u, k, n] - ev).max() <= 1e-10 * ev[-1], (u, k, n)
            # the kept entries always carry the table rows of their own index
            for n in range(S):
                g = r["index"][u, k, n]
                assert np.array_equal(r["tau"][u, k, n], tau[g]) and np.array_equal(r["position"][u, k, n], pos[g]) and r["cost"][u, k, n] == r["costmap"][u, k, g]
            p = b["planted"][u, k]                                               # the planted source: the very shifts; on a line that is within one grid cell
            assert np.array_equal(r["tau"][u, k, 0], tau[p])
            if case["kind"] == "linear":
                assert abs(int(r["index"][u, k, 0]) - int(p)) <= 1
    assert entries > 0 and left <= 0.02 * entries, (entries, left)


@pytest.mark.parametrize("i", [2, 4, 7, 8])
def test_calculator(dsr, cuda, i):
    import torch
    case = K.CASES[i]; Cn = case["C"]
    sg, pos, dl, tau = _grid(dsr, case)
    loc = dsr.MccCalculator(sg); D = loc.D
    b = K.build(case, tau, D); L = b["L"]; valid = K.valid_blocks(case, b)
    g = int(b["planted"][0, 0]); delays = dl[g]
    for nv in (True, False):
        r = loc.calc(_t(b["x"], cuda), L, delays, normalizeVariance=nv, nsamples=_t(b["nsamples"], cuda), want_R=True, want_eig=True)
        torch.cuda.synchronize()
        assert np.array_equal(r["tau"], tau[g])
        cost = r["cost"].cpu().numpy(); R = r["R"].cpu().numpy(); eig = r["eig"].cpu().numpy(); v = r["valid"].cpu().numpy().astype(bool)
        assert np.array_equal(v, valid)
        for u in range(case["U"]):
            for k in range(case["B"]):
                if not valid[u, k] or (u, k) == b["zero"]:
                    assert cost[u, k] == 0.0 and not R[u, k].any() and not eig[u, k].any()
                    continue
                c, t, Rr, ev = M.calculate(b["x"][u, :, k * L:(k + 1) * L], delays, K.FS, D, nv)
                tol = K.tolerance(Cn, ev[-1] / ev[0])
                print("calc case %d nv=%d (%d, %d): |cost - ref| / tol = %.3g" % (i, nv, u, k, abs(cost[u, k] - c) / tol))
                assert abs(cost[u, k] - c) <= tol
                assert np.abs(R[u, k] - Rr).max() <= 1e-12 * np.abs(Rr).max()
                assert np.abs(eig[u, k] - ev).max() <= 1e-10 * ev[-1]
    with pytest.raises(dsr.DsrError) as e:                                       # a shift beyond D: the reference reads outside its buffers
        loc.calc(_t(b["x"], cuda), L, np.full(Cn, (D + 2) / K.FS))
    assert e.value.status == 6


class _Blocks(object):
    """a float stream over the blocks of one channel"""

    def __init__(self, x, L):
        self.x, self.L = x, L

    def size(self):
        return self.L

    def reset(self):
        pass

    def __iter__(self):
        return iter([self.x[k * self.L:(k + 1) * self.L] for k in range(self.x.size // self.L)])


@pytest.mark.parametrize("i", [2, 6, 8])
def test_stream_face_equals_batch_face(dsr, cuda, i):
    import torch
    from dsr.btk.localization import SGB4LinearArrayPtr, SGB4CircularArrayPtr, MCCLocalizerPtr, MCCCalculatorPtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    case = K.CASES[i]; Cn, S = case["C"], case["S"]
    sgb = K.configure((SGB4LinearArrayPtr if case["kind"] == "linear" else SGB4CircularArrayPtr)(Cn, True, K.FS), case)
    pos, dl, tau = sgb.enumerate()
    loc = dsr.MccLocalizer(sgb, S); b = K.build(case, tau, loc.D); L = b["L"]; B = case["B"]
    x0 = b["x"][0][:, :B * L]
    r = loc.run(_t(x0[None], cuda), L, want_R=True); torch.cuda.synchronize()
    r = {k: v.cpu().numpy() for k, v in r.items() if v is not None}
    m = MCCLocalizerPtr(sgb, S)
    for c in range(Cn):
        m.setChannel(PyVectorFloatFeatureStreamPtr(_Blocks(x0[c], L)))
    for k in range(B):
        v = np.array(m.next())
        assert np.array_equal(v, r["position"][0, k, 0]) and np.array_equal(m.getPosition(), r["position"][0, k, 0])
        assert np.array_equal(m.getR(), r["R"][0, k]) and np.array_equal(m.getEigenValues(), r["eig"][0, k, 0])
        assert m.getMaxMCCC() == 1.0 - np.exp(r["cost"][0, k, 0])
        for n in range(S):
            assert np.array_equal(m.getNthBestPosition(n), r["position"][0, k, n]) and m.getNthBestMCCC(n) == 1.0 - np.exp(r["cost"][0, k, n])
            assert [m.getNthBestDelayedSample(n, c) for c in range(Cn)] == r["tau"][0, k, n].tolist()
        assert m.getDelayedSample(Cn - 1) == r["tau"][0, k, 0, Cn - 1]
    with pytest.raises(StopIteration):
        m.next()
    # the best candidate's delays steer a beamformer
    d = m.getChannelDelays()
    assert np.array_equal(d, r["tau"][0, B - 1, 0] / float(K.FS))
    bf = dsr.Beamformer(64, Cn); bf.calcArrayManifoldVectors(float(K.FS), d)
    # the calculator stream, normalisation on and off
    g = int(b["planted"][0, 0])
    for nv in (True, False):
        q = loc.calc(_t(x0[None], cuda), L, dl[g], normalizeVariance=nv); torch.cuda.synchronize()
        cm = MCCCalculatorPtr(sgb, nv)
        for c in range(Cn):
            cm.setChannel(PyVectorFloatFeatureStreamPtr(_Blocks(x0[c], L)))
        with pytest.raises(dsr.DsrError) as e:
            cm.next()
        assert e.value.status == 1 and "setTimeDelays" in str(e.value)
        cm.setTimeDelays(dl[g])
        for k in range(B):
            v = np.array(cm.next())
            assert v[0] == q["cost"].cpu().numpy()[0, k] and cm.getCostV() == v[0] and cm.getMCCC() == 1.0 - np.exp(v[0])
    # a block shorter than 2 D
    short = MCCLocalizerPtr(sgb, 1)
    for c in range(Cn):
        short.setChannel(PyVectorFloatFeatureStreamPtr(_Blocks(x0[c][:4 * (2 * loc.D - 1)], 2 * loc.D - 1)))
    with pytest.raises(dsr.DsrError) as e:
        short.next()
    assert e.value.status == 1 and "insufficient" in str(e.value)
