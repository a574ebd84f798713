"""Seeded inputs of the multi-stream tests: score matrices that span 1e-3 .. 1e6 with both signs, index tables, and the near-cancellation set on
which a fused multiply-add in the combination shows (tests/test_ms_np_cpu.py builds and checks it, tests/test_gpu_multistream.py runs the kernel on
the same arrays)."""
from fractions import Fraction
from functools import lru_cache

import numpy as np

WEIGHTS = [(0.95, 0.05), (1.0, 0.0), (0.0, 1.0), (0.3, 1.7)]
FMA_WEIGHTS = [(0.95, 0.05), (0.3, 1.7)]
FMA_ROWS, FMA_COLS = 100, 40                              # the cancellation set as a score matrix [100][40], identity table


def scores(rng, shape):
    """costs of magnitude 1e-3 .. 1e6, both signs"""
    return (rng.choice([-1.0, 1.0], size=shape) * 10.0 ** rng.uniform(-3.0, 6.0, size=shape)).astype(np.float32)


def tables(KA, KV, seed):
    """identity (where the shapes allow it), a permutation-like table and a many-to-one table that leaves some video columns unused (KV > 2) and
    uses column KV - 1"""
    rng = np.random.default_rng(seed)
    out = {}
    if KA == KV:
        out["identity"] = np.arange(KA, dtype=np.int32)
        out["permutation"] = rng.permutation(KA).astype(np.int32)
    else:
        out["wrapped"] = ((np.arange(KA) * 5 + 1) % KV).astype(np.int32)
    used = max(1, KV // 2)
    t = rng.integers(0, used, size=KA).astype(np.int32) if used > 1 else np.zeros(KA, np.int32)
    t[rng.integers(0, KA)] = KV - 1
    out["many_to_one"] = t
    return out


def _rd(x):
    """a Fraction rounded to the nearest double (int / int true division is correctly rounded)"""
    return float(x)


@lru_cache(maxsize=None)
def fma_case(wA, wV, seed=20):
    """a = float32(-(wV v) / wA) for random v: wA a + wV v nearly cancels, so the one rounding a fused multiply-add skips decides the result.
    -> dict(a, v [FMA_ROWS][FMA_COLS] float32, unfused = the reference's bits, fmaA = fma(wA, a, rd(wV v)), fmaV = fma(wV, v, rd(wA a)), each
    rounded to float32, computed in exact rational arithmetic)"""
    rng = np.random.default_rng(seed)
    n = FMA_ROWS * FMA_COLS
    v = scores(rng, n)
    a = (-(np.float64(wV) * v.astype(np.float64)) / np.float64(wA)).astype(np.float32)
    unfused, fmaA, fmaV = np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    FA, FV = Fraction(wA), Fraction(wV)
    for i in range(n):
        xa, xv = Fraction(float(a[i])), Fraction(float(v[i]))
        pa, pv = _rd(FA * xa), _rd(FV * xv)
        unfused[i] = np.float32(_rd(Fraction(pa) + Fraction(pv)))
        fmaA[i] = np.float32(_rd(FA * xa + Fraction(pv)))
        fmaV[i] = np.float32(_rd(FV * xv + Fraction(pa)))
    sh = (FMA_ROWS, FMA_COLS)
    return dict(a=a.reshape(sh), v=v.reshape(sh), unfused=unfused.reshape(sh), fmaA=fmaA.reshape(sh), fmaV=fmaV.reshape(sh))
