"""Cases and inputs of the multichannel cross-correlation tests (tests/test_mcc_np_cpu.py, tests/test_gpu_mcc.py).

A block holds a white source that reaches channel c with the integer sample delay tau[c] of one grid point (block_c[m] = s[m - tau[c]], so the
candidate with that tau aligns the channels), on top of independent white noise a channel.  The noise level 0.3 against a unit source keeps
the condition number of every candidate's covariance near C / 0.09 + 1, far below the 1e5 the GPU tolerances assume; L = 2 D cases, where R
is estimated from D samples only, use few channels and a large array so that D stays well above C.

k_mcc_cost<CT> and k_mcc_eig<CT> (csrc/k_mcc.hip) are instantiated for CT = ceil(C / 16) = 1..4 tiles of 16 channels, a matrix row taking
RS = 16 CT + 1 doubles of LDS.  Which C of CASES launches which instantiation, and how full its last tile is:

    CT  RS  C of the cases        last tile
    1   17  2, 4, 8, 13           2, 4, 8, 13 of 16 rows live
    2   33  17                    one live row (the first C past a tile edge)
    2   33  32                    full
    3   49  40                    half full (8 rows)
    3   49  48                    full
    4   65  64                    full"""
import numpy as np

from tests import mcc_np as M

FS = 16000
NOISE = 0.3
KAPPA_MAX = 1e5
EPS = 2.2e-16

# kind, C, geometry (spacing or radius in mm; "pos" = irregular positions through setPositionsOfMicrophones), L (0 = 2 D), maxSource, U, B
CASES = [
    dict(kind="linear", C=2, geom=1500.0, L=0, S=1, U=2, B=3),
    dict(kind="linear", C=4, geom=400.0, L=0, S=3, U=2, B=3),
    dict(kind="linear", C=4, geom=50.0, L=1024, S=3, U=2, B=2),
    dict(kind="linear", C=8, geom=40.0, L=4096, S=1, U=2, B=2),
    dict(kind="linear", C=13, geom="pos", L=1024, S=3, U=3, B=2),
    dict(kind="circular", C=8, geom=1000.0, L=0, S=3, U=2, B=3),
    dict(kind="circular", C=8, geom=100.0, L=1024, S=1, U=2, B=2),
    dict(kind="circular", C=32, geom=150.0, L=1024, S=3, U=2, B=2),
    dict(kind="circular", C=64, geom=210.0, L=4096, S=3, U=2, B=2),
    dict(kind="circular", C=64, geom=210.0, L=1024, S=1, U=3, B=3),
    # batches large enough that a workgroup of k_mcc_cost walks several groups of four candidates (candidates_per_workgroup below), and one
    # with more than 1024 blocks, where a workgroup takes the whole grid
    dict(kind="circular", C=8, geom=1000.0, L=1024, S=3, U=4, B=4),
    dict(kind="circular", C=64, geom=210.0, L=512, S=3, U=6, B=6),
    dict(kind="linear", C=4, geom=50.0, L=64, S=3, U=33, B=33),
    # the instantiation of three channel tiles, and the partial-tile edges (the table in the module docstring)
    dict(kind="circular", C=40, geom=180.0, L=1024, S=3, U=2, B=2),              # CT = 3, last tile half full
    dict(kind="circular", C=48, geom=200.0, L=1024, S=1, U=2, B=2),              # CT = 3, every tile full
    dict(kind="linear", C=17, geom=30.0, L=1024, S=3, U=2, B=2),                 # CT = 2 with one live row in the second tile
]
MULTI_GROUP = (10, 11, 12)


def candidates_per_workgroup(G, UB):
    """how dsr_mcc_run divides the grid (csrc/k_mcc.hip, mcc_launch): the groups of four candidates are split over about 1024 / (U B)
    workgroups a block -> the candidates one workgroup walks"""
    groups = -(-G // 4); split = min(max(1024 // UB, 1), groups)
    return -(-groups // split) * 4


def irregular_positions(C):
    """a line along y with uneven spacing, 30 mm on average"""
    rng = np.random.default_rng(77)
    y = np.concatenate([[0.0], np.cumsum(20.0 + 20.0 * rng.random(C - 1))])
    return np.stack([np.zeros(C), y, np.zeros(C)], axis=1)


def configure(grid, case):
    """the case's geometry on a grid object with the reference's setters (the restatement's Grid or the product's SearchGrid)"""
    if case["kind"] == "circular":
        grid.setRadius(case["geom"], 0.0)
    elif case["geom"] == "pos":
        grid.setPositionsOfMicrophones(irregular_positions(case["C"]))
    else:
        grid.setDistanceBtwMicrophones(case["geom"])
    return grid


def np_grid(case):
    return configure(M.Grid(case["kind"], case["C"], FS), case)


def build(case, tauTab, D, seed=None):
    """-> dict(x [U][C][N] float32, nsamples [U], L, planted [U][B] grid index (-1: the all-zero block), zero (u, b))
    Utterance 0 is complete; the later ones lose their last block and a few samples more (ragged); block (0, B-1) is all zero."""
    C, U, B = case["C"], case["U"], case["B"]; L = case["L"] or 2 * D; N = B * L + 7
    G = tauTab.shape[0]
    rng = np.random.default_rng(1000 + CASES.index(case) if seed is None else seed)
    x = np.zeros((U, C, N), np.float32); planted = np.full((U, B), -1, np.int64)
    for u in range(U):
        for b in range(B):
            near = np.flatnonzero(np.abs(tauTab).max(axis=1) <= (D // 4 if not case["L"] else D))      # L = 2 D: large shifts read mostly wrapped samples
            g = int(near[rng.integers(0, near.size)]); planted[u, b] = g
            s = rng.standard_normal(L + 2 * D + 2)
            for c in range(C):
                m = np.arange(L) - int(tauTab[g, c]) + D + 1
                x[u, c, b * L:(b + 1) * L] = (s[m] + NOISE * rng.standard_normal(L)).astype(np.float32)
        x[u, :, B * L:] = rng.standard_normal((C, N - B * L)).astype(np.float32)
    x[0, :, (B - 1) * L:B * L] = 0.0; planted[0, B - 1] = -1
    nsamples = np.full(U, N, np.int32)
    for u in range(1, U):
        nsamples[u] = B * L - 1 - (3 * u) % (L - 1)                                  # the last block is short: invalid
    return dict(x=x, nsamples=nsamples, L=L, planted=planted, zero=(0, B - 1))


def valid_blocks(case, b):
    """[U][B] bool: (b + 1) L <= nsamples[u]"""
    L = b["L"]
    return np.array([[(k + 1) * L <= b["nsamples"][u] for k in range(case["B"])] for u in range(case["U"])])


def tolerance(C, kappa):
    """the first-order bound on a log-determinant from eigenvalues or pivots with absolute error eps ||R||, both sides having it"""
    return 8.0 * C * kappa * EPS


def reference(case, b, tauTab, D):
    """the restatement over every valid block -> {(u, k): dict of mcc_np.localize}"""
    out = {}; v = valid_blocks(case, b); L = b["L"]
    for u in range(case["U"]):
        for k in range(case["B"]):
            if v[u, k]:
                out[(u, k)] = M.localize(b["x"][u, :, k * L:(k + 1) * L], tauTab, D, case["S"])
    return out


def comparable_entries(ref, tauTab, C):
    """per kept entry: may its grid index be compared?  Yes when every other candidate's cost is further than 2 tol away, or equals it exactly
    with the same tau row (the same arithmetic on both sides: the tie rule decides)."""
    costs, kappa = ref["costs"], ref["kappa"]; out = []
    for c, g in ref["best"]:
        if g < 0:
            out.append(True); continue
        ok = True
        for h in range(costs.size):
            if h == g:
                continue
            tol = max(tolerance(C, kappa[g]), tolerance(C, kappa[h]))
            if abs(costs[h] - c) <= 2 * tol and not (costs[h] == c and np.array_equal(tauTab[h], tauTab[g])):
                ok = False; break
        out.append(ok)
    return out
