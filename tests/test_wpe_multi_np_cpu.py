"""The numpy restatement of multi-channel WPE (tests/wpe_multi_np.py) pinned against the CPU oracle at small sizes: cold start, own filters
and one channel's filter for all, a limited bandwidth.  The GPU tests of the tiled path use the restatement where the oracle is too slow
or cannot be seeded with the filters of a previous block."""
import numpy as np
import pytest

from tests import wpe_multi_np as W


def _signal(Cn, N, M, seed):
    rng = np.random.default_rng(seed)
    s = rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M))
    Y = np.zeros((Cn, N, M), np.complex128)
    for c in range(Cn):
        Y[c] = s * np.exp(1j * c) + 0.1 * (rng.standard_normal((N, M)) + 1j * rng.standard_normal((N, M)))
        for k in range(1, 8):
            Y[c, k:] += (0.5 + 0.05 * c) ** k * np.roll(s, k, axis=0)[k:] * np.exp(1j * k * (c + 1))
    F = M // 2 + 1
    Y[:, :, F:] = np.conj(Y[:, :, 1:F - 1][:, :, ::-1])                   # the mirrored half the reference's streams carry
    return Y


@pytest.mark.parametrize("Cn,lowerN,upperN,iters,loadDb,bw,fc", [(3, 2, 4, 2, -20.0, 0.0, -1), (2, 1, 5, 2, -10.0, 0.0, 0), (3, 3, 4, 1, -30.0, 4000.0, 1)])
def test_wpe_multi_np_matches_oracle(oracle, Cn, lowerN, upperN, iters, loadDb, bw, fc):
    M, N = 8, 70
    F = M // 2 + 1
    Y = _signal(Cn, N, M, Cn + lowerN + upperN)
    wo, wg = oracle.wpe_multi(Y, lowerN, upperN, iters, loadDb, bw, 16000.0, filterChan=fc)
    out, gn = W.wpe_multi(Y[:, :, :F], M, lowerN, upperN, iters, loadDb, bw, 16000.0, filterChan=fc)
    np.testing.assert_allclose(gn, wg[:, :F], rtol=1e-9, atol=1e-12)
    assert np.abs(out - wo[:, :, :F]).max() <= 1e-9 * np.abs(wo).max()


def test_wpe_multi_np_seeded():
    """A seeded start is the same chain: zero seed = cold start; iterating k then m times = k + m times from zero."""
    M, N, lowerN, upperN, Cn = 8, 60, 2, 4, 2
    Y = _signal(Cn, N, M, 3)[:, :, :M // 2 + 1]
    g2 = W.filters(Y[:, :, 1], 1, lowerN, upperN, 2)
    assert np.array_equal(W.filters(Y[:, :, 1], 1, lowerN, upperN, 2, g0=np.zeros_like(g2)), g2)
    g1 = W.filters(Y[:, :, 1], 1, lowerN, upperN, 1)
    np.testing.assert_allclose(W.filters(Y[:, :, 1], 1, lowerN, upperN, 1, g0=g1), g2, rtol=1e-12, atol=1e-14)
