"""CPU tests of the sample-rate converter's definition (include/dsr.h section 6d): the numpy restatement tests/src_np.py meets the conditions the
definition was chosen for, and the library's host-only entries (create, ratio, out_samples, the table, the path, the refusals, the operator's
size()) agree with it.  No device is needed.

The signal conditions: unit-amplitude sines of 0.5 s at the source rate, measured on the central half of the output.  Passband tones at 0.25, 0.5
and 0.6 of the output Nyquist come out within 0.01 dB (amplitude from a Hann-windowed DFT at the tone's frequency; worst measured 0.004 dB); a tone
at 1.25 x the output Nyquist is rejected by 78 / 94 / 118 dB for fastest / medium / best (output RMS x sqrt 2 against 1; worst measured 81.5 / 97.1 /
122.0 dB); the image at 5000 Hz of a 3000 Hz tone taken from 8 to 16 kHz lies below -78 / -105 / -125 dB (measured -81.0 / -109.6 / -129.2 dB)."""
import numpy as np
import pytest

from tests import src_np as S

DOWN = [(22050, 16000), (44100, 16000), (48000, 16000), (16000, 8000)]
ALIAS_DB = {"fastest": -78.0, "medium": -94.0, "best": -118.0}
IMAGE_DB = {"fastest": -78.0, "medium": -105.0, "best": -125.0}
COMMON = [8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000, 96000]


def _db(v):
    return 20.0 * np.log10(max(float(v), 1e-300))


@pytest.fixture(scope="module")
def down():
    """{(src, dst, method, tone as a fraction of the output Nyquist): the central half of the converted tone}, each converted once"""
    out = {}
    for src, dst in DOWN:
        for m in S.SINC:
            tab = S.table(src, dst, m)
            for fr in (0.25, 0.5, 0.6, 1.25):
                x = S.tone(fr * dst / 2.0, src)
                out[src, dst, m, fr] = S.central_half(S._outputs(x, 0, src, dst, m, 0, S.out_samples(src, dst, x.size), tab)[0])
    return out


@pytest.mark.parametrize("method", S.SINC)
@pytest.mark.parametrize("src,dst", DOWN)
def test_passband_tones_within_a_hundredth_of_a_decibel(down, src, dst, method):
    for fr in (0.25, 0.5, 0.6):
        dev = _db(S.tone_amplitude(down[src, dst, method, fr], fr * dst / 2.0, dst))
        print("%d -> %d %s, tone at %.2f Nyquist: %+.5f dB" % (src, dst, method, fr, dev))
        assert abs(dev) <= 0.01


@pytest.mark.parametrize("method", S.SINC)
@pytest.mark.parametrize("src,dst", DOWN)
def test_alias_rejection(down, src, dst, method):
    y = down[src, dst, method, 1.25]
    level = _db(np.sqrt(np.mean(y * y)) * np.sqrt(2.0))
    print("%d -> %d %s, tone at 1.25 Nyquist: %.1f dB" % (src, dst, method, level))
    assert level <= ALIAS_DB[method]


@pytest.mark.parametrize("method", S.SINC)
def test_image_rejection_on_interpolation(method):
    y = S.central_half(S.convert(S.tone(3000.0, 8000), 8000, 16000, method))
    level = _db(S.tone_amplitude(y, 5000.0, 16000))
    print("8000 -> 16000 %s: image at 5000 Hz %.1f dB, tone at 3000 Hz %+.5f dB" % (method, level, _db(S.tone_amplitude(y, 3000.0, 16000))))
    assert level <= IMAGE_DB[method]


@pytest.mark.parametrize("method", S.SINC)
@pytest.mark.parametrize("src,dst", DOWN + [(8000, 16000), (44100, 48000)])
def test_constant_comes_out_constant(src, dst, method):
    L, M, K = S.ratio(src, dst, method)
    y = S.convert(np.full(6 * K + 50, 0.75), src, dst, method)
    edge = K * L // M + 2                                                              # outputs whose window reaches a zero outside the input
    mid = y[edge:y.size - edge]
    assert mid.size > 10 and np.abs(mid - 0.75).max() <= 1e-12


@pytest.mark.parametrize("src,dst", DOWN + [(8000, 16000), (44100, 48000), (11025, 16000), (16000, 16000)])
def test_out_samples_is_the_floor(dsr, src, dst):
    c = dsr.SampleRateConverter(src, dst, "fastest")
    assert (c.L, c.M, c.K) == S.ratio(src, dst, "fastest")
    for n in (0, 1, c.M - 1, c.M, 12345):
        assert c.out_samples(n) == S.out_samples(src, dst, n) == (n * c.L) // c.M
        assert S.convert(np.zeros(n), src, dst, "zoh").size == (n * c.L) // c.M
    assert c.out_samples(1 << 40) == ((1 << 40) * c.L) // c.M                          # 64-bit all the way


@pytest.mark.parametrize("method", S.SINC + ("zoh", "linear"))
@pytest.mark.parametrize("src,dst", [(22050, 16000), (48000, 16000), (8000, 16000), (44100, 48000), (16000, 16000)])
def test_blocks_with_a_final_flush_equal_the_one_shot_call(src, dst, method):
    K = S.ratio(src, dst, method)[2]
    x = np.random.default_rng(5).standard_normal(900)
    x = x.astype(np.float32) if method in ("zoh", "linear") else x
    one = S.convert(x, src, dst, method)
    short = max(2 * K - 3, 1)                                                          # a block shorter than 2K
    for lens in ([311, short, 0, 589 - short], [1] * 7 + [893], [900], [450, 449, 1], [899 - short, short, 1]):
        got = S.stream_convert(x, src, dst, method, lens)
        assert got.dtype == one.dtype and np.array_equal(got, one), (lens, got.size, one.size)


def test_zoh_and_linear_are_their_closed_forms():
    x = np.random.default_rng(6).standard_normal(500).astype(np.float32)
    for src, dst in [(22050, 16000), (8000, 16000), (48000, 16000), (44100, 48000)]:
        L, M, _ = S.ratio(src, dst, "zoh"); n = np.arange(500 * L // M); base = n * M // L
        assert np.array_equal(S.convert(x, src, dst, "zoh"), x[base])
        xp = np.concatenate([x, np.zeros(1, np.float32)])
        f = ((n * M % L).astype(np.float32) / np.float32(L)).astype(np.float32)
        lin = S.convert(x, src, dst, "linear")
        assert lin.dtype == np.float32 and np.array_equal(lin, xp[base] + f * (xp[base + 1] - xp[base]))
        exact = xp[base].astype(np.float64) + (n * M % L) / L * (xp[base + 1].astype(np.float64) - xp[base])
        assert np.abs(lin - exact).max() <= 4 * 2.0 ** -24 * np.abs(x).max() * 2
    assert np.array_equal(S.convert(x, 16000, 16000, "best"), x)                       # equal rates: a copy


def test_library_table_is_the_restatement_rounded_to_fp32(dsr):
    for src, dst, m in [(22050, 16000, "fastest"), (44100, 16000, "best"), (48000, 16000, "medium"), (8000, 16000, "best"), (11025, 16000, "best")]:
        c = dsr.SampleRateConverter(src, dst, m); t = c.table(); r = S.table(src, dst, m)
        assert t.shape == r.shape == (c.L, 2 * c.K)
        assert np.all(np.abs(t - r) <= 2.0 ** -24 * np.abs(r) + 1e-14)                 # one rounding of the fp64 value
        assert np.abs(t.astype(np.float64).sum(axis=1) - 1.0).max() <= 2 * c.K * 2.0 ** -24


def test_common_rates_are_all_accepted_and_the_table_cap_refuses(dsr):
    worst = 0
    for a in COMMON:
        for b in COMMON:
            L, M, K = S.ratio(a, b, "best"); worst = max(worst, L)
            assert 2 * K * L <= S.TABLE_CAP
    assert worst == 1280                                                               # 11025 -> 32000 and 11025 -> 96000; 2K L = 81920
    c = dsr.SampleRateConverter(11025, 16000, "best")
    assert (c.L, c.M, c.K) == (640, 441, 32)
    with pytest.raises(ValueError):
        S.ratio(44101, 96000, "best")                                                  # L = 96000, 2K = 64
    with pytest.raises(dsr.DsrError) as e:
        dsr.SampleRateConverter(44101, 96000, "best")
    assert e.value.status == dsr.E_PARAMETER
    assert dsr.SampleRateConverter(44101, 96000, "linear").L == 96000                  # no table, no cap


def test_refusals(dsr):
    with pytest.raises(dsr.DsrError) as e:
        dsr.SampleRateConverter(22050, 16000, "sinc")
    assert e.value.status == dsr.E_CONSISTENCY and "Cannot recognize type (sinc) of sample rate converter." in str(e.value)
    with pytest.raises(KeyError):
        S.ratio(22050, 16000, "sinc")
    for a, b in [(0, 16000), (16000, 0)]:
        with pytest.raises(dsr.DsrError) as e:
            dsr.SampleRateConverter(a, b, "best")
        assert e.value.status == dsr.E_PARAMETER
        with pytest.raises(ValueError):
            S.ratio(a, b, "best")


def test_path_names_the_cell_without_a_device(dsr, monkeypatch):
    from dsr import _src
    monkeypatch.delenv("DSR_SRC_TABLE", raising=False)
    cell = lambda *a: dsr.SampleRateConverter(*a).path()
    assert cell(22050, 16000, "fastest")[:2] == (_src.SRC_TABLE_LDS, _src.SRC_INPUT_LDS)
    t = cell(44100, 16000, "best")                                                     # 160 rows of 2 x 89 + 1 floats: about 112 KB, beside the tile
    assert t[:2] == (_src.SRC_TABLE_LDS, _src.SRC_INPUT_LDS) and 160 * 179 * 4 < t[3] <= 160 * 1024
    assert cell(48000, 16000, "best")[0] == _src.SRC_TABLE_UNIFORM                     # L = 1
    assert cell(8000, 16000, "best")[0] == _src.SRC_TABLE_LDS                          # M = 1
    assert cell(11025, 16000, "best")[0] == _src.SRC_TABLE_MEM                         # 640 rows of 65 floats do not fit
    assert cell(96000, 1, "fastest")[:2] == (_src.SRC_TABLE_UNIFORM, _src.SRC_INPUT_DIRECT)    # 2K = 1 920 000 taps: no tile holds them
    assert cell(22050, 16000, "zoh")[:2] == cell(16000, 16000, "best")[:2] == (_src.SRC_TABLE_NONE, _src.SRC_INPUT_DIRECT)
    monkeypatch.setenv("DSR_SRC_TABLE", "mem")
    assert cell(22050, 16000, "fastest")[0] == cell(48000, 16000, "best")[0] == _src.SRC_TABLE_MEM


@pytest.mark.parametrize("size,src,dst,expect", [(160, 22050, 16000, 116), (441, 44100, 16000, 160), (320, 8000, 16000, 640)])
def test_operator_size_follows_the_float_formula(dsr, size, src, dst, expect):
    from dsr.btk.feature import SampleFeaturePtr, SamplerateConversionFeaturePtr
    assert S.feature_size(size, src, dst) == expect
    samp = SampleFeaturePtr(blockLen=size, shiftLen=size)
    f = SamplerateConversionFeaturePtr(samp, src, dst)
    assert f.size() == expect and f.name() == "SamplerateConversion"
    assert SamplerateConversionFeaturePtr(samp, src, dst, 77, "best", "r").size() == 77
    with pytest.raises(dsr.DsrError) as e:
        SamplerateConversionFeaturePtr(samp, src, dst, 0, "nearest")
    assert e.value.status == dsr.E_CONSISTENCY
