"""CPU tests of the numpy restatement of the scalar feature operators (tests/featops_np.py) and of the shared cases (tests/featops_cases.py).
They exercise the restatement only: they pass with and without the device operators, and pin what the GPU tests of tests/test_gpu_featops.py
rely on -- the frame and hit counts of the YIN case, and that a d(tau) summed in another order is seen in the returned value."""
import numpy as np
import pytest

from tests import featops_cases as Cs
from tests import featops_np as R


def test_yin_case_counts_are_pinned():
    """Headset1, N = 512, shift 160, threshold 0.5: 840 frames, 366 without a pitch, hits in all four chunks of 64 lags (16 / 406 / 30 / 22).
    A later change of the cases cannot silently empty a chunk."""
    x, p, v, tau = Cs.yin_headset()
    hist, misses = Cs.yin_chunk_histogram(tau)
    assert x.shape == (Cs.YIN_FRAMES, Cs.YIN_N)
    assert misses == Cs.YIN_MISSES and hist == Cs.YIN_CHUNK_HITS
    assert ((p[:, 0] == 0) == (tau <= 1)).all() and (p[tau > 1, 0] == (16000.0 / (tau[tau > 1] - 1)).astype(np.float32)).all()


@pytest.mark.parametrize("variant", ["f64", "four"])
def test_a_wrong_summation_order_is_seen_in_the_value(variant):
    """d(tau) accumulated in fp64 and rounded once, or in four fp32 partial sums over j mod 4, leaves every pitch of the Headset1 case as it is
    (0 of 840 differ) but changes the bits of the value at the returning lag: measured 372 of 840 frames for the fp64 accumulator and 374 of 840
    for the four partial sums (which change 38 % of the d(tau) elements).  The pitch alone cannot show the order, the value does."""
    x, p, v, tau = Cs.yin_headset()
    p2, v2 = R.yin_pitch(x, 16000, 0.5, variant=variant)
    nd = Cs.differing(v, v2)
    print("%s: %d of %d pitches and %d values differ" % (variant, Cs.differing(p, p2), len(v), nd))
    assert Cs.differing(p, p2) == 0
    assert nd > len(v) // 10


def test_yin_small_frames_and_sine():
    assert R.yin_pitch(np.ones((2, 3), np.float32))[0].tolist() == [[0.0], [0.0]]                  # W = 1: the loop never runs
    p, v = R.yin_pitch(np.zeros((1, 512), np.float32))                                              # 0/0 fails both comparisons
    assert p[0, 0] == 0 and np.isnan(v[0])
    p, v, tau = R.yin_pitch(Cs.sine_frame(), details=True)
    assert tau[0] == 81 and p[0, 0] == np.float32(16000.0 / 80)


def test_spike_filter_is_the_median_with_a_zero_tail():
    for tapN, n in ((3, 320), (5, 320), (9, 64), (5, 6)):
        q = (tapN - 1) // 2
        for x in (Cs.frames(n, n, 3, 9000), Cs.ties_block(n, tapN)):
            y = R.spike_filter(x, tapN)
            ref = np.stack([np.median(x[:, i - q:i + q + 1], axis=1) for i in range(q, n - 2 * q)], axis=1) if n - 2 * q > q else np.zeros((len(x), 0))
            assert np.array_equal(y[:, q:n - 2 * q], ref.astype(np.float32))
            assert np.array_equal(y[:, :min(q, n - 2 * q)], x[:, :min(q, n - 2 * q)])
            assert not y[:, n - 2 * q:].any()
    for tapN, n in ((2, 10), (4, 10), (5, 4)):
        with pytest.raises(ValueError):
            R.spike_filter(np.zeros((1, n), np.float32), tapN)


def test_spike_filter2_removes_a_spike_and_leaves_a_ramp():
    ramp = (np.arange(4 * 320, dtype=np.float32) * 3.0).reshape(4, 320)
    f = R.SpikeFilter2()
    assert np.array_equal(f.run(ramp), ramp) and f.count == 0
    x = Cs.spike_blocks()
    f = R.SpikeFilter2()
    assert np.array_equal(f.run(x), x) and f.count == 0                                             # speech alone has no such slopes
    for name, where in Cs.SPIKES.items():
        f = R.SpikeFilter2(); y = f.run(Cs.with_spikes(x, where))
        assert f.count > 0, name
    f = R.SpikeFilter2(); y = f.run(Cs.with_spikes(x, Cs.SPIKES["middle"]))
    assert f.count == 2 and np.abs(y - x).max() < 100.0                                             # the line between the neighbours, not the spike


def test_minmax_operators():
    e = Cs.energy_chain()
    a = R.ALog(1.0, 4.0).run(e)
    b = np.float32(e.max() / 1e4)
    assert np.allclose(a[:, 0], np.log10((b + e[:, 0]).astype(np.float64)), rtol=1e-6)
    n = R.Normalize(0.0, 1.0).run(e)
    assert n.min() == 0.0 and abs(n.max() - 1.0) < 1e-6
    ro = R.Normalize(0.0, 1.0, runon=True)
    first = ro.run(e[:10]); again = ro.run(e[:10])
    assert Cs.differing(first, again) > 0                                                          # the bounds of the first pass are kept ...
    ro.nextSpeaker()
    assert Cs.differing(ro.run(e[:10]), first) == 0                                                   # ... until nextSpeaker()
    with np.errstate(all="ignore"):
        c = R.Normalize().run(np.full((3, 2), 5.0, np.float32))
    assert not np.isfinite(c).any()


def test_threshold_resample_and_sphinx_mel():
    x = np.array([[-2.0, -1.0, -0.5, 0.0, 0.5, 1.0, 2.0]], np.float32)
    assert R.threshold(x, 9.0, 1.0, "upper").tolist() == [[-2.0, -1.0, -0.5, 0.0, 0.5, 9.0, 9.0]]
    assert R.threshold(x, 9.0, 1.0, "lower").tolist() == [[9.0] * 6 + [2.0]]
    assert R.threshold(x, 9.0, 1.0, "both").tolist() == [[-9.0, -9.0, -0.5, 0.0, 0.5, 9.0, 9.0]]
    with pytest.raises(KeyError):
        R.threshold(x, 0.0, 1.0, "neither")
    s = np.abs(np.random.default_rng(3).standard_normal((2, 257)))
    assert np.array_equal(R.spectral_resample(s, 1.0, 0), s.astype(np.float32).astype(np.float64))  # weight 1 on the sample itself, 0 past the end
    assert R.spectral_resample(s, R.SAMPLE_RATIO, 0).shape == (2, 257) and R.spectral_resample(s, 0.4, 129).shape == (2, 129)
    with pytest.raises(ValueError):
        R.spectral_resample(s, 1.0, 129)                                                            # effective ratio 1.99
    with pytest.raises(IndexError):
        R.spectral_resample(s[:, :100], 1.0, 200)                                                   # element 100 of 100 with weight 0.5
    assert not R.sphinx_mel_filters().any()                                                         # the defaults lowerF = upperF = 0
    A = R.sphinx_mel_filters(512, 257, 16000.0, 130.0, 6800.0, 40)
    assert A.shape == (40, 257) and (A >= 0).all() and (A.max(axis=1) > 0.5).all() and not A[:, 0].any()
    with pytest.raises(ValueError):
        R.sphinx_mel_filters(512, 257, 16000.0, 130.0, 8001.0, 30)
