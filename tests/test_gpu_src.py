"""GPU tests of the sample-rate converter (include/dsr.h section 6d, csrc/src_kernels.hip) through the C-ABI binding, the operator and the C++ facade.

Batch: U = 2 utterances of C = 2 channels, 2400 and 1873 samples of seeded noise plus a tone.  The reference is the fp64 restatement tests/src_np.py.
Tolerance of a sinc method -- derived, nothing of it measured: |y - y64| <= (2K + 3) 2^-24 sum_j |h_j x_j|, the sum from the restatement: 2^-24 for
the rounded coefficient, and at most 2K + 2 roundings for the products and any order of summation.  zoh and linear match bit for bit, and so do all
the paths among themselves: table in LDS / in memory, every tile split, one-shot / blocks with carried state, U, C, and a second call.
Run with -s for the cell and the largest observed fraction of the bound of every case."""
import os
import subprocess

import numpy as np
import pytest

from tests import src_np as S
from tests.conftest import PKG

pytestmark = pytest.mark.gpu

U, C, N = 2, 2, 2400
LENS = (2400, 1873)
RATIOS = [(22050, 16000), (48000, 16000), (8000, 16000), (44100, 48000), (11025, 16000)]
SWITCHES = ("DSR_SRC_TABLE", "DSR_SRC_RUN", "DSR_SRC_TILES")
LDS, MEM, UNIFORM, NONE = 0, 1, 2, 3
CELL = {(22050, 16000): LDS, (48000, 16000): UNIFORM, (8000, 16000): LDS, (44100, 48000): LDS}      # 11025 -> 16000: by method, below


def _signal():
    rng = np.random.default_rng(20240611)
    x = rng.standard_normal((U, C, N)) * 0.25 + 0.5 * np.sin(2 * np.pi * 0.031 * np.arange(N) + rng.uniform(0, 6, (U, C, 1)))
    return np.ascontiguousarray(x.astype(np.float32))


X = _signal()
_REF = {}


def _ref(src, dst, method):
    """{(u, c): (y, sum |h x|)} of the one-shot call on every row's own length, computed once"""
    key = (src, dst, method)
    if key not in _REF:
        _REF[key] = {(u, c): S.convert(X[u, c, :LENS[u]], src, dst, method, with_mag=True) for u in range(U) for c in range(C)}
    return _REF[key]


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _one_shot(dsr, cuda, src, dst, method, x=None, lens=LENS):
    """-> (converter, y [U][C][out] with NaN where nothing was written, nout)"""
    import torch
    x = X if x is None else x
    c = dsr.SampleRateConverter(src, dst, method)
    y = torch.full((x.shape[0], x.shape[1], c.out_samples(x.shape[2])), float("nan"), dtype=torch.float32, device=cuda)
    y, nout = c.apply(torch.from_numpy(x).to(cuda), torch.tensor(lens, dtype=torch.int32, device=cuda), y=y)
    return c, y.cpu().numpy(), nout.cpu().numpy()


def _check_counts(c, y, nout, lens=LENS):
    for u, n in enumerate(lens):
        assert nout[u] == (n * c.L) // c.M
        assert np.isfinite(y[u]).all() and np.all(y[u, :, nout[u]:] == 0), "utterance %d: its row is not zero past %d outputs (NaN: never written)" % (u, nout[u])


@pytest.mark.parametrize("method", S.SINC)
@pytest.mark.parametrize("src,dst", RATIOS)
def test_sinc_methods_stay_within_the_derived_bound(dsr, cuda, src, dst, method):
    c, y, nout = _one_shot(dsr, cuda, src, dst, method)
    expect = CELL.get((src, dst), MEM if method == "best" else LDS)                     # 640 rows of 65 floats do not fit in LDS, of 21 or 33 they do
    assert c.path()[0] == expect, "%d -> %d %s takes cell %s, the case is there for table cell %d" % (src, dst, method, c.path(), expect)
    _check_counts(c, y, nout)
    assert (nout > c.path()[2]).any() or c.M > c.L                                      # more than one tile wherever the ratio gives that many outputs
    worst = 0.0
    for (u, ch), (ref, mag) in _ref(src, dst, method).items():
        err = np.abs(y[u, ch, :nout[u]].astype(np.float64) - ref); bound = (2 * c.K + 3) * 2.0 ** -24 * mag
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), "%d -> %d %s row (%d, %d): %.3g of the bound" % (src, dst, method, u, ch, (err / bound).max())
    print("%d -> %d %s: L %d M %d K %d, cell %s, largest error %.4f of the bound" % (src, dst, method, c.L, c.M, c.K, c.path(), worst))


@pytest.mark.parametrize("method", ("zoh", "linear"))
@pytest.mark.parametrize("src,dst", RATIOS + [(16000, 16000)])
def test_zoh_and_linear_match_bit_for_bit(dsr, cuda, src, dst, method):
    c, y, nout = _one_shot(dsr, cuda, src, dst, method)
    assert c.path()[0] == NONE
    _check_counts(c, y, nout)
    for (u, ch), (ref, _) in _ref(src, dst, method).items():
        assert ref.dtype == np.float32 and np.array_equal(y[u, ch, :nout[u]], ref)


@pytest.mark.parametrize("src,dst,method", [(22050, 16000, "fastest"), (48000, 16000, "medium"), (8000, 16000, "best"), (44100, 48000, "fastest"),
                                            (44100, 16000, "best")])
def test_table_in_memory_and_every_tile_split_equal_the_default_path(dsr, cuda, monkeypatch, src, dst, method):
    c, y, nout = _one_shot(dsr, cuda, src, dst, method)
    assert c.path()[0] in (LDS, UNIFORM)
    monkeypatch.setenv("DSR_SRC_TABLE", "mem")
    cm, ym, nm = _one_shot(dsr, cuda, src, dst, method)
    assert cm.path()[0] == MEM and np.array_equal(nm, nout) and np.array_equal(ym, y)
    monkeypatch.delenv("DSR_SRC_TABLE")
    for run, tiles in ((256, 1), (256, 3), (512, 16), (1024, 2)):
        monkeypatch.setenv("DSR_SRC_RUN", str(run)); monkeypatch.setenv("DSR_SRC_TILES", str(tiles))
        ct, yt, nt = _one_shot(dsr, cuda, src, dst, method)
        assert ct.path()[2] == run and ct.path()[0] == c.path()[0]
        assert np.array_equal(nt, nout) and np.array_equal(yt, y), (run, tiles)


def _blocks(K):
    """three ragged blocks per utterance; one of utterance 0 is shorter than 2K, and the utterances' blocks differ in length"""
    short = max(2 * K - 3, 1)
    return [[1000, short, LENS[0] - 1000 - short], [700, 900, LENS[1] - 1600]]


@pytest.mark.parametrize("src,dst,method", [(22050, 16000, "fastest"), (44100, 16000, "best"), (48000, 16000, "medium"), (8000, 16000, "best"),
                                            (11025, 16000, "best"), (22050, 16000, "zoh"), (48000, 16000, "linear"), (8000, 16000, "linear"),
                                            (16000, 16000, "medium")])
def test_three_ragged_blocks_with_a_final_flush_equal_the_one_shot_call(dsr, cuda, src, dst, method):
    import torch
    c, y, nout = _one_shot(dsr, cuda, src, dst, method)
    state = c.state(U, C, cuda); blocks = _blocks(c.K); pos = [0, 0]; got = [[] for _ in range(U)]
    assert any(b < 2 * c.K for b in blocks[0]) or c.K <= 1
    for k in range(3):
        lens = [blocks[u][k] for u in range(U)]; stride = max(lens)
        xb = np.zeros((U, C, stride), np.float32)
        for u in range(U):
            xb[u, :, :lens[u]] = X[u, :, pos[u]:pos[u] + lens[u]]; pos[u] += lens[u]
        yb = torch.full((U, C, c.block_out_bound(stride)), float("nan"), dtype=torch.float32, device=cuda)
        yb, nb = c.block(state, torch.from_numpy(xb).to(cuda), torch.tensor(lens, dtype=torch.int32, device=cuda), flush=(k == 2), y=yb)
        yb, nb = yb.cpu().numpy(), nb.cpu().numpy()
        for u in range(U):
            assert np.all(yb[u, :, nb[u]:] == 0)
            assert nb[u] == S.block_end(src, dst, method, pos[u], k == 2) - S.block_end(src, dst, method, pos[u] - lens[u], False)
            got[u].append(yb[u, :, :nb[u]])
    for u in range(U):
        whole = np.concatenate(got[u], axis=1)
        assert whole.shape[1] == nout[u] and np.array_equal(whole, y[u, :, :nout[u]]), "utterance %d" % u


@pytest.mark.parametrize("src,dst,method", [(22050, 16000, "medium"), (48000, 16000, "best"), (8000, 16000, "fastest"), (11025, 16000, "best"),
                                            (22050, 16000, "linear")])
def test_rows_do_not_depend_on_the_batch_and_a_second_call_repeats(dsr, cuda, src, dst, method):
    c, y, nout = _one_shot(dsr, cuda, src, dst, method)
    _, y2, n2 = _one_shot(dsr, cuda, src, dst, method)
    assert np.array_equal(y2, y) and np.array_equal(n2, nout)                           # a second call, on a new handle
    import torch
    xd = torch.from_numpy(X).to(cuda); ns = torch.tensor(LENS, dtype=torch.int32, device=cuda)
    y3, n3 = c.apply(xd, ns); y4, n4 = c.apply(xd, ns)                                   # and on the same handle
    assert np.array_equal(y3.cpu().numpy(), y) and np.array_equal(y4.cpu().numpy(), y) and np.array_equal(n4.cpu().numpy(), nout)
    for u in range(U):                                                                  # U = 1
        _, yu, nu = _one_shot(dsr, cuda, src, dst, method, x=np.ascontiguousarray(X[u:u + 1]), lens=LENS[u:u + 1])
        assert nu[0] == nout[u] and np.array_equal(yu[0], y[u])
    for ch in range(C):                                                                 # C = 1
        _, yc, nc = _one_shot(dsr, cuda, src, dst, method, x=np.ascontiguousarray(X[:, ch:ch + 1]))
        assert np.array_equal(nc, nout) and np.array_equal(yc[:, 0], y[:, ch])


def test_state_of_another_shape_and_a_short_output_row_are_refused(dsr, cuda):
    import torch
    c = dsr.SampleRateConverter(22050, 16000, "fastest")
    x = torch.from_numpy(X).to(cuda)
    st = c.state(1, C, cuda)                                                            # a state for one utterance
    with pytest.raises(dsr.DsrError) as e:
        c.block(st, x)
    assert e.value.status == dsr.E_CONSISTENCY
    st = c.state(U, C, cuda); c.block(st, x)                                            # the right shape goes through
    with pytest.raises(dsr.DsrError) as e:
        c.apply(x, y=torch.zeros((U, C, c.out_samples(N) - 1), dtype=torch.float32, device=cuda))
    assert e.value.status == dsr.E_DIMENSION


class _Samples:
    """a sample source of 441-sample blocks for PyVectorFloatFeatureStreamPtr"""

    def __init__(self, x, block):
        self.x, self.block = x, block

    def size(self):
        return self.block

    def reset(self):
        pass

    def __iter__(self):
        return iter(self.x[: self.x.size // self.block * self.block].reshape(-1, self.block))


def test_operator_blocks_equal_the_batch_call(dsr, cuda):
    import torch
    from dsr.btk.feature import SamplerateConversionFeaturePtr
    from dsr.btk.stream import PyVectorFloatFeatureStreamPtr
    x = np.ascontiguousarray(np.concatenate([X[0, 0], X[0, 1], X[1, 0]])[:441 * 15 + 200])           # 15 whole blocks and a rest the source drops
    src = PyVectorFloatFeatureStreamPtr(_Samples(x, 441))
    f = SamplerateConversionFeaturePtr(src, 44100, 16000, 0, "medium")
    assert f.size() == 160
    c = dsr.SampleRateConverter(44100, 16000, "medium")
    batch = c.apply(torch.from_numpy(x[:441 * 15]).to(cuda)[None, None])[0].cpu().numpy()[0, 0]
    assert batch.size == 15 * 160

    def walk(op, size):
        rows = []
        for k in range(1000):
            try:
                rows.append(np.array(op.next(k)))
            except StopIteration:                                                       # DSR_E_ITERATOR
                break
        assert op.isEnd() and all(r.size == size for r in rows)
        return np.concatenate(rows)

    first = walk(f, 160)
    assert np.array_equal(first, batch)
    f.reset()
    assert np.array_equal(walk(f, 160), first)                                          # reset(): a second pass equals the first
    f.reset(); f.next(0)
    with pytest.raises(dsr.DsrError) as e:
        f.next(5)                                                                       # out of order: the reference's jindex_error
    assert e.value.status == dsr.E_INDEX
    g = SamplerateConversionFeaturePtr(PyVectorFloatFeatureStreamPtr(_Samples(x, 441)), 44100, 16000, 100, "medium")
    part = walk(g, 100)                                                                 # 2400 outputs in blocks of 100 fill 24 blocks ...
    assert np.array_equal(part, batch[:2400])
    h = SamplerateConversionFeaturePtr(PyVectorFloatFeatureStreamPtr(_Samples(x, 441)), 44100, 16000, 700, "medium")
    assert np.array_equal(walk(h, 700), batch[:2100])                                   # ... and in blocks of 700 three: the last 300 are not delivered


FACADE = r"""
#include "dsr_streams.hpp"
#include <cstdio>
int main() {
  std::vector<float> x(441 * 6);
  for (size_t i = 0; i < x.size(); i++) x[i] = (float) ((int) ((i * 37) % 101) - 50);
  SampleFeaturePtr samp(new SampleFeature("", 441, 441, true));
  samp->setSamples(x.data(), x.size(), 44100);
  try { SamplerateConversionFeaturePtr bad(new SamplerateConversionFeature(samp, 44100, 16000, 0, "nearest")); }
  catch (jconsistency_error& e) { printf("unknown %d %s\n", (int) e.getCode(), e.what()); }
  SamplerateConversionFeaturePtr f(new SamplerateConversionFeature(samp, 44100, 16000, 0, "medium"));
  printf("size %u %s\n", f->size(), f->name().c_str());
  try {
    for (int k = 0; k < 2; k++) { const float* y = f->next(k); printf("block %d", k); for (int i = 0; i < 160; i += 53) printf(" %a", y[i]); printf("\n"); }
  } catch (j_error& e) { printf("err %d %s\n", (int) e.getCode(), e.what()); }
  return 0;
}
"""


def test_cpp_facade_pulls_two_blocks_and_maps_the_unknown_method(dsr, cuda, tmp_path):
    import torch
    src = tmp_path / "f.cpp"; src.write_text(FACADE); exe = tmp_path / "f"
    subprocess.check_call(["g++", "-std=c++11", "-Wall", "-Werror", "-I", os.path.join(PKG, "host"), str(src), "-o", str(exe), "-L", os.path.join(PKG, "lib"),
                           "-ldsr_hip", "-Wl,-rpath," + os.path.join(PKG, "lib"), "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "unknown 3 Cannot recognize type (nearest) of sample rate converter." and lines[1] == "size 160 SamplerateConversion", lines
    x = np.array([(i * 37) % 101 - 50 for i in range(441 * 6)], np.float32)
    y = dsr.SampleRateConverter(44100, 16000, "medium").apply(torch.from_numpy(x).to(cuda)[None, None])[0].cpu().numpy()[0, 0]
    for k in range(2):
        tok = lines[2 + k].split()
        assert tok[:2] == ["block", str(k)] and [float.fromhex(v) for v in tok[2:]] == [float(v) for v in y[160 * k:160 * (k + 1):53]], lines
