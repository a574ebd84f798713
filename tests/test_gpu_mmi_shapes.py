"""SubbandMMI (k_mmi, csrc/k_mmi.hip) at the sizes where a thread owns more than one bin, against the oracle's frame-by-frame restatement
(oracle/orc_mmi.c) with the set-up calls, inputs and tolerance of tests/test_gpu_mmi.py.  The cases are in tests/mmi_cases.py;
tests/test_mmi_cpu.py asserts that their masks strike some of the bins from 256 on and spare others.

k_mmi is one workgroup of 256 threads per utterance.  Branch or template instance of the kernel and its launch, and the case that reaches it:

    branch / instance                                                        case (number as in mmi_cases.CASES, from 1)
    bin loop f = tid, tid + 256, ...: a second bin for thread 0 only         1, 2, 5, 6 (F = 257)
    bin loop: a second bin for every thread                                  3, 4 (F = 512)
    bin loop: up to five bins a thread, F no multiple of 256                 7 (F = 1262)
    k_mmi<16> at its last channel count (C = 16, time-aligned in registers)  1, 3, many utterances
    k_mmi<0> at its first channel count (C = 17, taScr)                      2, 4
    wide mask (fwidth > 1): the ordered pass reads avgOut / outS / maskS
      at indices >= 256, f1 = M / 2 = 256                                    1, 2, 5
      f1 = M - 1 = 511 and 1261 (halfBandShift)                              4, 7
    narrow mask (fwidth 1) on second bins                                    3
    mask type 1: the target's densities updated twice a frame, wup weights   2
    weights of calcWeightsN (NC = 2, three sources)                          2
    APAB with halfBandShift: bin f >= 256 takes the weight of bin M - 1 - f  3
    APAB without halfBandShift: Fout = 512 > F, mirror writes to M - f,
      from mirS / maskS in the wide pass                                     5
    TYPE_ZELINSKI2 (steering with the beamformer's own vector), no mask      6
    dynamic LDS 52 F <= 64 KiB                                               1 - 6 (at most 26 624 bytes)
    dynamic LDS above 64 KiB (65 624 bytes)                                  7
    dynamic LDS above 150 KiB: refused with a dimension error                test_lds_refusal (fftLen 4096, halfBandShift: 212 992 bytes)
    rows past an utterance's end written as zeros, Fout wide                 every case (nframes T, T - 2, 1)
    more utterances than compute units, U = 300                              test_many_utterances"""
import time

import numpy as np
import pytest

from tests import mmi_cases as Mc

pytestmark = pytest.mark.gpu


def _apply(obj, X, nfr, cuda):
    import torch
    return obj.apply(torch.from_numpy(X).to(cuda), torch.from_numpy(nfr).to(cuda)).cpu().numpy()


def _run_case(i, cuda):
    case = Mc.CASES[i]
    X, nfr, refs = Mc.reference(i)
    a = Mc.make("dsr", case)
    assert (a.bins(), a.outBins()) == Mc.bins(case)
    Y = _apply(a, X, nfr, cuda)
    worst = Mc.check(case, Y, X, nfr, refs)
    print("case %s: largest error %.3f TOL" % (Mc.IDS[i], worst))
    return worst


@pytest.mark.parametrize("i", range(len(Mc.CASES)), ids=Mc.IDS)
def test_subband_mmi_shapes(i, cuda):
    _run_case(i, cuda)


def test_lds_refusal(dsr, cuda):
    """fftLen 4096 with halfBandShift needs 52 x 4096 = 212 992 bytes of LDS: apply refuses, every time, and the library goes on working"""
    import torch
    big = Mc.make("dsr", (4096, 4, True, 0, 2, 0x02, 0.7, 1, (0.6, 3, 0), 708))
    X = torch.zeros((1, 4, 1, 4096), dtype=torch.complex64, device=cuda)
    for _ in range(2):
        with pytest.raises(dsr.DsrError) as e:
            big.apply(X)
        assert e.value.status == dsr.E_DIMENSION and "212992 bytes of LDS" in str(e.value)
    torch.cuda.synchronize()
    _run_case(0, cuda)


def test_many_utterances(cuda):
    """U = 300 in case 1's configuration: copies of three inputs, each cut at 1, 2 or 3 frames; the first copy of each (input, frames) pair
    against the oracle, every other copy bit-equal to the first"""
    case = Mc.CASES[0][:10] + (3, 3)
    U = 300
    X3 = Mc.snapshots(case)
    src = np.arange(U) % 3; nfr = (1 + (np.arange(U) // 3 + np.arange(U)) % 3).astype(np.int32)
    assert len({(s, n) for s, n in zip(src, nfr)}) == 9
    full = [Mc.oracle_run(case, X3[k]) for k in range(3)]                       # a prefix of the frames gives a prefix of the output
    t0 = time.time()
    Y = _apply(Mc.make("dsr", case), np.ascontiguousarray(X3[src]), nfr, cuda)
    print("U = 300: apply and copies %.2f s" % (time.time() - t0))
    first = {}
    for u in range(U):
        key = (int(src[u]), int(nfr[u]))
        if key not in first:
            first[key] = u
            worst = Mc.check(case, Y[u:u + 1], X3[src[u]][None], nfr[u:u + 1], [full[src[u]][:nfr[u]]])
            print("input %d, %d frames: largest error %.3f TOL" % (key + (worst,)))
        else:
            assert np.array_equal(Y[u], Y[first[key]]), (u, first[key])
    assert len(first) == 9
