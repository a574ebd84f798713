"""The further spherical-array beamformers' host math (dsr_sph kinds HWNC, GSC, HWNCGSC, SPATIALDS, MOEN; csrc/sph.cpp) without a GPU: every
host table through the C-ABI against the restatement tests/sph2_np.py to 1e-12 of the table row's largest entry, properties that do not pass
through the restatement, the error paths and the Python constructors' defaults (read from beamformer.i:651, :680, :709, :764, :997)."""
import ctypes as C
import inspect

import numpy as np
import pytest

from tests import sph_np as S
from tests import sph2_np as S2
from tests.sph2_cases import FS, GEOMS, LOOK, geometry, handle

M = 64
TOL = 1e-12


def _close(got, ref, tol=TOL):
    """row by row (the last axis): |got - ref| <= tol max|ref|"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale = np.abs(ref).max(axis=-1, keepdims=True)
    err = np.abs(got - ref)
    assert np.all(err <= tol * scale), float((err / np.maximum(scale, 1e-300)).max())


def _tables(s):
    return s.modeAmplitudes(), s.harmonics()


@pytest.mark.parametrize("geom,mo", GEOMS)
@pytest.mark.parametrize("ratio,sigma2", [(1.0, 0.0), (0.3, 0.0), (-1.0, 0.0), (0.3, 0.02)])
def test_hwnc_weights(dsr, geom, mo, ratio, sigma2):
    s = handle(dsr, "HWNC", M, geom, mo, ratio=ratio)
    if sigma2:
        s.setSigma2(sigma2)
    s.setLookDirection(*LOOK)
    B, Sh = _tables(s)
    ref = S2.modal_look("HWNC", B, mo, s.C, *LOOK, ratio=ratio, sigma2=sigma2)
    _close(s.lookWeights(), ref)
    _close(s.calcWNG()[None], S2.hwnc_wng(B, s.C, ratio)[None])
    _close(s.beamWeights(1)[0], S2.fold(ref, Sh))
    if ratio > 0:                                                            # independent: ||w|| = 2 sqrt(pi / (C wng)), through a float (2^-23 relative)
        nrm = np.sqrt((np.abs(s.lookWeights()[1:]) ** 2).sum(axis=1))
        want = 2 * np.sqrt(np.pi / (s.C * s.calcWNG()[1:]))
        assert np.all(np.abs(nrm - want) <= 2.0 ** -23 * want)


@pytest.mark.parametrize("geom,mo", [g for g in GEOMS if g[1] > 1])
@pytest.mark.parametrize("kind,NC,normalize", [("GSC", 1, False), ("GSC", 2, True), ("HWNCGSC", 2, False), ("HWNCGSC", 1, True)])
def test_gsc_tables(dsr, oracle, geom, mo, kind, NC, normalize):
    """w_q, w_l, the effective weights and their fold against the restatement.  For B this is a consistency check only: the handle's B
    deviates from the reference's (conj(wq) into _calcBlockingMatrix, then one projection of every column against wq), the restatement
    gsc_blocking_matrix mirrors those two steps, and it is fed the handle's own wq.  What holds B independently: B^H wq = 0
    (test_blocking_matrix_blocks_quiescent), B^H B = I (test_blocking_matrix_columns_orthonormal) and, below, the oracle's
    _calcBlockingMatrix on the same vector, which can be compared for NC = 1 and up to 4 dimensions only."""
    s = handle(dsr, kind, M, geom, mo, normalizeWeight=normalize, NC=NC, ratio=0.3 if kind == "HWNCGSC" else None)
    s.setLookDirection(*LOOK)
    B, Sh = _tables(s)
    D, F = s.dim, M // 2 + 1
    wq = S2.modal_look(kind, B, mo, s.C, *LOOK, ratio=0.3, normalize=normalize)
    _close(s.lookWeights(), wq)
    wqh = s.lookWeights()                                                    # B from the handle's own wq: classical Gram-Schmidt over up to 63 columns
    rng = np.random.default_rng(mo + NC)                                     # turns a last-bit difference of its input into 1e-5 (tests/sph2_np.py)
    wl = np.zeros((F, D), np.complex128)
    assert np.all(s.wl() == 0) and np.all(s.blockingMatrix(0) == 0)
    for f in (1, 7, M // 2):
        Bm = S2.gsc_blocking_matrix(wqh[f], NC)
        _close(s.blockingMatrix(f).T, Bm.T)
        if NC == 1:                                                          # the oracle's _calcBlockingMatrix (NC = 1) on the same vector
            Bo, ok = oracle.blocking_matrix(np.conj(wqh[f]))
            assert ok
            if D <= 4:                                                       # (GSL's BLAS sums in another order, which classical Gram-Schmidt
                _close(s.blockingMatrix(f).T, Bo.T)                          # amplifies column by column: 15 columns already show it)
        packed = rng.standard_normal(2 * (D - NC))
        s.setActiveWeights_f(f, packed)
        wl[f] = S2.sidelobe_wl(Bm, packed)
    _close(s.wl(), wl)
    eff = S2.gsc_effective(wq, wl, normalize)
    _close(s.beamWeights(1)[0], S2.fold(eff, Sh))
    s.setLookDirection(0.4, -1.0)                                            # a new look direction: B anew, wl kept
    _close(s.wl(), wl)
    wq2 = S2.modal_look(kind, B, mo, s.C, 0.4, -1.0, ratio=0.3, normalize=normalize)
    _close(s.lookWeights(), wq2)
    _close(s.blockingMatrix(7).T, S2.gsc_blocking_matrix(s.lookWeights()[7], NC).T)
    _close(s.beamWeights(1)[0], S2.fold(S2.gsc_effective(wq2, wl, normalize), Sh))


@pytest.mark.parametrize("geom,mo", [g for g in GEOMS if g[1] > 1])
@pytest.mark.parametrize("kind,NC", [("GSC", 1), ("GSC", 2), ("HWNCGSC", 1)])
def test_blocking_matrix_blocks_quiescent(dsr, geom, mo, kind, NC):
    """B^H wq = 0 to 1e-10 for every GSC bin (relative to ||wq||; B's columns have unit norm).  _calcBlockingMatrix (beamformer.cc:398-479)
    projects with I - conj(d) d^T / ||d||^2 and so blocks the conjugate of its argument; the handle gives it conj(wq)."""
    s = handle(dsr, kind, M, geom, mo, NC=NC, ratio=1.0 if kind == "HWNCGSC" else None)
    s.setLookDirection(*LOOK)
    wq = s.lookWeights()
    for f in range(1, M // 2 + 1):
        Bm = s.blockingMatrix(f)
        r = np.abs(np.conj(Bm).T @ wq[f]).max() / np.sqrt((np.abs(wq[f]) ** 2).sum())
        print("bin %d: |B^H wq| / ||wq|| = %.3e" % (f, r))
        assert r <= 1e-10, (f, r)


@pytest.mark.parametrize("geom,mo", [("em", 4), ("rnd4", 2)])
def test_blocking_matrix_columns_orthonormal(dsr, geom, mo):
    """B^H B = I to 1e-10 up to 15 columns; classical Gram-Schmidt loses orthogonality with the column count (tests/sph2_np.py), so the
    63 columns of order 8 are not asked for it"""
    s = handle(dsr, "GSC", M, geom, mo, NC=1)
    s.setLookDirection(*LOOK)
    for f in range(1, M // 2 + 1):
        Bm = s.blockingMatrix(f)
        assert np.abs(np.conj(Bm).T @ Bm - np.eye(s.dim - 1)).max() <= 1e-10, f


@pytest.mark.parametrize("geom,mo", GEOMS)
def test_spatial_ds_weights(dsr, geom, mo):
    s = handle(dsr, "SPATIALDS", M, geom, mo, normalizeWeight=True)         # normalizeWeight is not applied (:2159-2161)
    s.setLookDirection(*LOOK)
    B, Sh = _tables(s)
    ref = S2.spatial_ds(B, Sh, mo, *LOOK)
    _close(s.sensorWeights(), ref)
    assert not np.allclose(s.sensorWeights()[0], 1.0)                        # bin 0 computed, not ones
    _close(s.beamWeights(1)[0], ref)
    with pytest.raises(dsr.DsrError):
        s.lookWeights()


def _close_nan(got, ref, tol=TOL):
    """_close on the rows without a NaN, and the same NaN pattern on both sides"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    rows = ~np.isnan(ref).any(axis=-1)
    assert rows.any()
    _close(got[rows], ref[rows], tol)


@pytest.mark.parametrize("geom,mo,lam,normalize", [(g, o, l, n) for g, o in GEOMS for l, n in [(0.0, False), (1e-2, False), (1e-2, True)]])
def test_moen_weights(dsr, geom, mo, lam, normalize):
    """EigenMike order 1 without loading: A is one constant row, so the 32 x 32 normal matrix is a constant, of rank 1 exactly.  On such a
    matrix the reference's single-precision LINPACK SVD takes one of three ways, and which one depends on the constant, that is on the bin:
    it converges to finite (and, the noise singular values above the threshold inverted, meaningless) weights; or a NaN arises in its
    rotations and the bin's weights are all NaN; or its deflation cases alternate without end, where csvdc here stops after a bounded number
    of passes and the bin's weights are all NaN as well (tests/test_sph2_np_cpu.py::test_pseudoinverse_of_exact_rank_one_terminates).  At
    M = 64 some bins go each way.  Library and restatement call the same dsr_pseudoinverse on the same bits: the NaN pattern is held equal
    and the finite bins to the tolerance."""
    s = handle(dsr, "MOEN", M, geom, mo, normalizeWeight=normalize)
    diag = np.zeros(M // 2 + 1, np.float32)
    if lam:
        for f in range(M // 2 + 1):
            s.setLevelOfDiagonalLoading(f, lam)
        diag[:] = lam
    s.setLookDirection(*LOOK)
    B, Sh = _tables(s)
    ref = S2.moen(dsr, B, Sh, mo, *LOOK, diag=diag, normalize=normalize)
    got = s.sensorWeights()                                                  # (it returns: the rank-1 bins end at csvdc's pass bound)
    assert np.array_equal(got[0], np.eye(1, s.C)[0])                         # calcDCWeights into the C-long vector: entries >= dim stay 0
    if (geom, mo, lam) == ("em", 1, 0.0):
        nan = np.isnan(got).any(axis=1)
        assert nan.any() and not nan.all() and np.array_equal(nan, np.isnan(got).all(axis=1))   # a bin is NaN as a whole or not at all
    else:
        assert not np.isnan(ref).any()
    _close_nan(got, ref)
    if not normalize:
        s.fixTerms(True)
        assert np.all(s.sensorWeights()[1:] == 0)                            # the quirk: _fixedW is zeroed before it is used
        s.fixTerms(False)
        _close_nan(s.sensorWeights(), ref)


# c of the constant 32 x 32 matrix, and what the reference's csvdc does with it (run stand-alone without the pass bound): "loops" never returns
RANK_ONE = [(0.5403251539712052, "loops"), (20.865661268574723, "loops"), (3.676791888153566, "loops"), (163.9835165805099, "nan"),
            (0.2882185851410415, "finite"), (22.01313956688178, "finite")]


@pytest.mark.parametrize("c,way", RANK_ONE)
def test_pseudoinverse_of_exact_rank_one_terminates(dsr, c, way):
    """dsr_pseudoinverse on c ones(32, 32), MOEN's normal matrix at EigenMike order 1 without loading.  LINPACK's QR iteration counts only its
    QR steps (case 3) against maxit; on the "loops" constants its two deflation cases alternate for ever.  csvdc here bounds the passes of any
    case (csrc/svd_linpack.cpp) and then reports the singular values left as not converged: the call returns, with status 0, ok = 0 and an
    all-NaN inverse, as on the constants where the unbounded routine itself ends in NaN.  Where it converges nothing changes: finite values
    and ok = 0 still (the noise singular values fall below the threshold 1e-8 of a 1e-7-relative spectrum only in part, the exact zeros do)."""
    n = 32
    A = np.full((n, n), c, np.complex128); P = np.zeros((n, n), np.complex128); ok = C.c_int(7); sv = np.zeros(n, np.float32)
    st = dsr.load().dsr_pseudoinverse(A.ctypes.data_as(C.c_void_p), n, n, C.c_float(1e-8), P.ctypes.data_as(C.c_void_p), C.byref(ok),
                                      sv.ctypes.data_as(C.c_void_p))
    assert st == 0 and ok.value == 0
    if way == "finite":
        assert np.all(np.isfinite(P.view(np.float64)))
        assert abs(sv[0] - n * c) <= 1e-5 * n * c and np.all(sv[1:] <= 1e-5 * sv[0])     # rank 1: one singular value n c, the rest noise
    else:
        assert np.all(np.isnan(P.real))


def test_pseudoinverse_pass_bound_leaves_converging_input_alone(dsr, oracle):
    """the pass bound is far from what a converging input needs: rank-deficient and full-rank matrices up to 40 x 40 give the bits of the
    oracle's csvdc, which has no such bound"""
    rng = np.random.default_rng(8)
    for n, r in [(5, 5), (32, 32), (32, 3), (40, 17), (40, 1)]:
        G = (rng.standard_normal((n, r)) + 1j * rng.standard_normal((n, r)))
        A = G @ np.conj(G.T)
        Po, oko = oracle.pseudoinverse(A)
        P = np.zeros((n, n), np.complex128); ok = C.c_int(7)
        dsr.check(dsr.load().dsr_pseudoinverse(np.ascontiguousarray(A).ctypes.data_as(C.c_void_p), n, n, C.c_float(1e-8),
                                               P.ctypes.data_as(C.c_void_p), C.byref(ok), None))
        assert bool(ok.value) == bool(oko) and np.array_equal(P, Po), (n, r)


@pytest.mark.parametrize("kind,geom,mo", [("HWNC", "em", 4), ("GSC", "em", 8), ("EB", "rnd4", 2), ("DS", "em", 1)])
def test_fold_is_the_transform(dsr, kind, geom, mo):
    """v^H x = w^H (S x) on random x, to 1e-12 of the sum of the products' magnitudes |w|^T |S| |x| (the error bound of either evaluation order)"""
    s = handle(dsr, kind, M, geom, mo, ratio=1.0 if kind == "HWNC" else None)
    s.setLookDirection(*LOOK)
    V, w, Sh = s.beamWeights(1)[0], s.lookWeights(), s.harmonics()
    rng = np.random.default_rng(5)
    x = rng.standard_normal((s.C, 3)) + 1j * rng.standard_normal((s.C, 3))
    a = np.conj(V) @ x
    b = np.conj(w) @ (Sh @ x)
    scale = np.abs(w) @ (np.abs(Sh) @ np.abs(x))
    assert np.all(np.abs(a - b) <= 1e-12 * scale)


def test_beams_table(dsr):
    """beam 0 the look direction with the active weights, beams 1.. their own directions without"""
    s = handle(dsr, "GSC", M, "em", 3, NC=1)
    s.setLookDirection(*LOOK)
    s.setActiveWeights_f(5, np.arange(16.0))
    s.setBeam(1, 2.0, -0.5); s.setBeam(2, 0.7, 1.9)
    V = s.beamWeights(3)
    B, Sh = _tables(s)
    for b, d in enumerate([LOOK, (2.0, -0.5), (0.7, 1.9)]):
        wq = S2.modal_look("GSC", B, 3, s.C, *d)
        wl = np.zeros_like(wq)
        if b == 0:
            wl[5] = S2.sidelobe_wl(S2.gsc_blocking_matrix(s.lookWeights()[5], 1), np.arange(16.0))
        _close(V[b], S2.fold(S2.gsc_effective(wq, wl, False), Sh))
    s.setBeam(0, 2.0, -0.5)                                                  # beam 0 is the look direction
    _close(s.lookWeights(), S2.modal_look("GSC", B, 3, s.C, 2.0, -0.5))


GRID = (0.0, np.pi, -np.pi, np.pi, 0.1, 0.1)


@pytest.mark.parametrize("kind,mode", [("HWNC", "modal"), ("EB", "modal"), ("DS", "modal"), ("GSC", "modal"), ("SPATIALDS", "sensor"), ("MOEN", "moen")])
def test_beam_pattern_matches_restatement(dsr, kind, mode):
    s = handle(dsr, kind, M, "em", 3, ratio=1.0 if kind == "HWNC" else None)
    a, th, ph = geometry("em")
    grid = (0.2, 1.3, -0.4, 0.9, 0.25, 0.3)
    got = s.getBeamPattern(9, 0.9, 0.2, *grid)
    w = (s.sensorWeights() if mode != "modal" else s.lookWeights())[9]       # getBeamPattern set the look direction
    ref = S2.beam_pattern(mode, w, 9, a, FS, M, th, ph, s.harmonics(), grid)
    assert got.shape == ref.shape
    assert np.all(np.abs(got - ref) <= 1e-12 * np.abs(ref).max())


def test_beam_pattern_grid_shape(dsr):
    s = handle(dsr, "HWNC", M, "em", 2, ratio=1.0)
    assert s.getBeamPattern(3).shape == (64, 64)                             # (int)(float)(2 pi / 0.1 + 1.5)
    assert s.getBeamPattern(3, 0.5, 0.5, 0.5, 0.5, 0.5, 0.5, 0.1, 0.1).shape == (1, 1)
    m = handle(dsr, "MOEN", M, "em", 2)
    assert m.getBeamPattern(3).shape == (64, 64)


def _cell(th, ph, look):
    return int(np.argmin(np.abs(th - look[0]))), int(np.argmin(np.abs(ph - look[1])))


@pytest.mark.parametrize("kind", ["HWNC", "SPATIALDS", "MOEN"])
def test_beam_pattern_peaks_at_look_direction(dsr, kind):
    """EigenMike, order 4, bin 16 of 64 (4 kHz, ka = 3.07), 0.1 rad grid: the arg-max lies in the look direction's grid cell; MOEN with the
    loading 1e-2 and its own unconjugated pattern (:2091).  The restatement alone peaks there for this bin (every bin 8..24 does), checked
    first below."""
    look, f = (1.0, 0.3), 16
    a, th_s, ph_s = geometry("em")
    B = S.mode_amplitudes(a, FS, M, 4); Sh = S.sensor_harmonics(4, th_s, ph_s)
    th, ph = S2.pattern_grid(*GRID)
    if kind == "HWNC":
        ref = S2.beam_pattern("modal", S2.modal_look("HWNC", B, 4, 32, *look, ratio=1.0)[f], f, a, FS, M, th_s, ph_s, Sh, GRID)
    elif kind == "MOEN":
        w = S2.moen(dsr, B[:f + 1], Sh, 4, *look, diag=np.full(f + 1, 1e-2, np.float32))[f]
        ref = S2.beam_pattern("moen", w, f, a, FS, M, th_s, ph_s, Sh, GRID)
    else:
        ref = S2.beam_pattern("sensor", S2.spatial_ds(B, Sh, 4, *look)[f], f, a, FS, M, th_s, ph_s, Sh, GRID)
    assert np.unravel_index(np.argmax(ref), ref.shape) == _cell(th, ph, look)
    s = handle(dsr, kind, M, "em", 4, ratio=1.0 if kind == "HWNC" else None)
    if kind == "MOEN":
        s.setLevelOfDiagonalLoading(f, 1e-2)
    got = s.getBeamPattern(f, *look, *GRID)
    assert np.unravel_index(np.argmax(got), got.shape) == _cell(th, ph, look)


def test_errors(dsr):
    L = dsr.load()
    h = C.c_void_p()
    assert L.dsr_sph_create(7, 1, FS, M, 0, 1, 2, 0, 4, C.byref(h)) == dsr.E_PARAMETER        # unknown kind
    assert L.dsr_sph_create(-1, 1, FS, M, 0, 1, 2, 0, 4, C.byref(h)) == dsr.E_PARAMETER
    for k in (2, 3, 4, 5, 6):
        assert L.dsr_sph_create(k, 1, FS, M, 1, 1, 2, 0, 4, C.byref(h)) == dsr.E_PARAMETER    # halfBandShift
    g = handle(dsr, "GSC", M, "em", 3, NC=2)
    with pytest.raises(dsr.DsrError) as e:
        g.setActiveWeights_f(3, np.zeros(14))                                # before setLookDirection
    assert e.value.status == 1
    g.setLookDirection(*LOOK)
    for n in (13, 16, 18):
        with pytest.raises(dsr.DsrError) as e:
            g.setActiveWeights_f(3, np.zeros(n))                             # 2 (dim - NC) = 14
        assert e.value.status == dsr.E_DIMENSION
    with pytest.raises(dsr.DsrError) as e:
        g.setActiveWeights_f(M // 2 + 1, np.zeros(14))
    assert e.value.status == dsr.E_DIMENSION
    g.setActiveWeights_f(M // 2, np.zeros(14))
    for NB in (0, 17, -1):
        with pytest.raises(dsr.DsrError) as e:
            g.beamWeights(NB)
        assert e.value.status == dsr.E_DIMENSION
        dummy = np.zeros(4, np.float32).ctypes.data_as(C.c_void_p)           # checked before anything is read or a device is needed
        assert L.dsr_sph_beams(g.h, dummy, dummy, 1, 1, NB, dummy, None) == dsr.E_DIMENSION
    for b in (-1, 16):
        with pytest.raises(dsr.DsrError):
            g.setBeam(b, 0.1, 0.2)
    with pytest.raises(dsr.DsrError):
        g.beamWeights(2)                                                     # beam 1 has no direction
    with pytest.raises(dsr.DsrError):
        handle(dsr, "GSC", M, "rnd4", 1, NC=1).lookWeights()                 # dim - NC = 0
    with pytest.raises(dsr.DsrError):
        g.setWNG(1.0)
    with pytest.raises(dsr.DsrError):
        g.fixTerms(True)
    with pytest.raises(dsr.DsrError):
        g.getBeamPattern(M // 2 + 1)
    gen = L.dsr_sph_settings_generation(g.h)
    g.setActiveWeights_f(2, np.ones(14))
    assert L.dsr_sph_settings_generation(g.h) == gen + 1
    m = handle(dsr, "MOEN", M, "em", 2)
    gen = L.dsr_sph_settings_generation(m.h)
    m.setLevelOfDiagonalLoading(3, 0.5); m.fixTerms(True)
    assert L.dsr_sph_settings_generation(m.h) == gen + 2
    with pytest.raises(dsr.DsrError):
        m.setLevelOfDiagonalLoading(M // 2 + 1, 0.5)


@pytest.mark.parametrize("kind", ["HWNC", "GSC", "HWNCGSC", "SPATIALDS", "MOEN"])
def test_no_steering_table_for_the_further_kinds(dsr, kind):
    """the SRP search exists over the EB and DS weights only: a handle of another kind refuses the table and what needs it, and the DOA wrapper
    refuses the kind outright"""
    L = dsr.load()
    s = handle(dsr, kind, M, "em", 2)
    assert L.dsr_sph_build_table(s.h) == 1
    assert L.dsr_sph_srp_path(s.h) == -1 and L.dsr_sph_has_table(s.h) == 0
    out = np.zeros((M // 2 + 1) * s.dim * 2)
    assert L.dsr_sph_steering(s.h, 0, out.ctypes.data_as(C.c_void_p), out.size) == 1
    dummy = np.zeros(4, np.float64).ctypes.data_as(C.c_void_p)               # refused before anything is read or a device is needed
    assert L.dsr_sph_srp(s.h, dummy, dummy, 1, 1, dummy, None, dummy, dummy, dummy, None, None, None) == 1
    with pytest.raises(dsr.DsrError) as e:
        handle(dsr, kind, M, "em", 2, nBest=2, cls=dsr.SphDoaSRP)
    assert e.value.status == 1
    for k in ("EB", "DS"):
        assert L.dsr_sph_build_table(handle(dsr, k, M, "em", 2, nBest=2, cls=dsr.SphDoaSRP).h) == 0


def test_stream_class_defaults(dsr):
    """the %extend constructors of beamformer.i: (fftLen, halfBandShift, NC, maxOrder, normalizeWeight[, ratio], nm)"""
    import dsr.btk.beamformer as BF
    want = {
        "SphericalHWNCBeamformerPtr": dict(fftLen=512, halfBandShift=False, NC=1, maxOrder=3, normalizeWeight=False, ratio=0.1, nm="SphericalHWNCBeamformer"),
        "SphericalGSCBeamformerPtr": dict(fftLen=512, halfBandShift=False, NC=1, maxOrder=4, normalizeWeight=False, nm="SphericalGSCBeamformer"),
        "SphericalHWNCGSCBeamformerPtr": dict(fftLen=512, halfBandShift=False, NC=1, maxOrder=4, normalizeWeight=False, ratio=1.0, nm="SphericalHWNCGSCBeamformer"),
        "SphericalMOENBeamformerPtr": dict(fftLen=512, halfBandShift=False, NC=1, maxOrder=4, normalizeWeight=False, nm="SphericalMOENBeamformer"),
        "SphericalSpatialDSBeamformerPtr": dict(fftLen=512, halfBandShift=False, NC=1, maxOrder=3, normalizeWeight=False, nm="SphericalSpatialDSBeamformer"),
    }
    for name, d in want.items():
        p = inspect.signature(getattr(BF, name).__init__).parameters
        assert list(p)[:2] == ["self", "sampleRate"] and p["sampleRate"].default is inspect.Parameter.empty
        assert {k: v.default for k, v in p.items() if k not in ("self", "sampleRate")} == d, name
        with pytest.raises(dsr.DsrError):
            getattr(BF, name)(FS, 64, True)                                  # halfBandShift
    pat = inspect.signature(BF.SphericalMOENBeamformerPtr.getBeamPattern).parameters
    assert [pat[k].default for k in ("theta", "phi", "widthTheta", "widthPhi")] == [0.0, 0.0, 0.1, 0.1]
    assert pat["minTheta"].default == -np.pi and pat["maxPhi"].default == np.pi
    g = BF.SphericalGSCBeamformerPtr(FS, 64)
    with pytest.raises(dsr.DsrError):
        g.setActiveWeights_f(1, np.zeros(30))                                # before setLookDirection
    g.setEigenMikeGeometry()
    assert g.getBeamPattern(4, 1.0, 0.2, 0.0, 1.0, 0.0, 1.0, 0.5, 0.5).shape == (3, 3)
    g.setActiveWeights_f(1, np.zeros(30))                                    # getBeamPattern set the look direction (modalBeamformer.cc:768)
    h = BF.SphericalHWNCBeamformerPtr(FS, 64, maxOrder=2)
    h.setEigenMikeGeometry()
    assert h.getBeamPattern(4, 1.0, 0.0, 0.0, 1.0, 0.0, 1.0, 0.5, 0.5).shape == (3, 3) and h.calcWNG().shape == (33,)
