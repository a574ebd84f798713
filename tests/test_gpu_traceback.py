"""The best path of a decode comes from k_traceback, a kernel of its own behind k_viterbi: k_viterbi leaves one trace head per utterance (the best token's
back pointer and where the utterance's back-pointer records start), k_traceback follows it and writes arcs, words, their counts and the two statuses a path
can end in.  Where the records do not outlive the utterance (run to completion with more utterances than workgroups: a slot's arena is reused) k_viterbi follows the chain and k_traceback starts
from the hop records; the cases assert which of the two they ran.  Every case here compares the whole result record, the arcs and the words with the oracle's sequential decoder on the same scores."""
import ctypes as C

import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

NDIST = 16
BEAM, LMSCALE = 30.0, 2.0
NFR = [45, 37, 0, 1, 2, 33, 26, 21, 12, 5, 2, 40]          # ragged: no frame at all (JITERATOR), one, two, and lengths that end in different segments
OK, E_ALLOCATION, E_DIMENSION, E_ITERATOR = 0, 2, 5, 9


def eps_graph(seed=61):
    """tests.synth.random_wfst with 200 states and many epsilon arcs (chains inside the graph), few final states of its own, and epsilon chains of
    1, 2, 3 and 4 hops -- some hops with an output symbol -- from twelve states each into final states of their own: the cheapest way to end."""
    arcs, fin = synth.random_wfst(200, NDIST, seed=seed, eps_frac=0.35, nFinal=4, out_frac=0.3)
    rng = np.random.default_rng(1000 + seed); nxt = 200
    for hops in (1, 2, 3, 4):
        for s in rng.choice(np.arange(1, 200), 12, replace=False):
            cur = int(s)
            for _ in range(hops):
                arcs.append((cur, nxt, 0, int(rng.integers(1, 50)) if rng.random() < 0.4 else 0, float(np.float32(rng.uniform(0.0, 0.3))))); cur = nxt; nxt += 1
            fin.append((cur, float(np.float32(rng.uniform(0, 0.2)))))
    return arcs, fin


def both_graphs(dsr, oracle, arcs, fin):
    go, gd = oracle.Wfst(), dsr.Wfst()
    for a in arcs:
        go.add_arc(*a); gd.add_arc(*a)
    for s, c in fin:
        go.add_final(s, c); gd.add_final(s, c)
    return go, gd


@pytest.fixture(scope="module")
def case(dsr, oracle):
    """One graph, one batch of scores, the oracle's decode of every utterance: computed once, shared by the tests below, never changed."""
    arcs, fin = eps_graph()
    go, gd = both_graphs(dsr, oracle, arcs, fin)
    ex = go.export()
    sc = np.random.default_rng(69).uniform(0, 10, (len(NFR), max(NFR), NDIST)).astype(np.float32)
    ref = [go.decode(sc[u, :t], beam=BEAM, lmScale=LMSCALE) if t > 0 else None for u, t in enumerate(NFR)]
    assert all(r is None or r["rc"] == 0 for r in ref)
    return dict(go=go, gd=gd, arcIn=ex["arcIn"], arcOut=ex["arcOut"], sc=sc, ref=ref)


def decode(dsr, cuda, dec, sc, nfr, maxPath, want_paths=True):
    """dsr_decoder_decode_batch with the raw record: nArcs and nWords as the device counted them, the rows of arcs and words whole (what lies behind a path
    in its row is the staging buffer's and says nothing)"""
    import torch
    U, T, nDist = sc.shape
    d_sc = torch.from_numpy(np.ascontiguousarray(sc)).to(cuda); d_n = torch.tensor(nfr, dtype=torch.int32, device=cuda)
    res = (dsr.DecodeResult * U)()
    arcs = np.zeros((U, max(maxPath, 1)), np.int32); words = np.zeros((U, max(maxPath, 1)), np.uint32)
    dsr.check(dsr._lib.dsr_decoder_decode_batch(dec.h, dsr._dev(d_sc), dsr._dev(d_n), U, T, nDist, C.byref(res),
                                                dsr._ptr(arcs) if want_paths else None, dsr._ptr(words) if want_paths else None, maxPath, dsr.cur_stream()))
    out = []
    for u in range(U):
        r = res[u]
        out.append(dict(status=r.status, score=r.score, ac=r.ac, lm=r.lm, frames=r.frames, reachedFinal=bool(r.reachedFinal), nArcs=r.nArcs, nWords=r.nWords,
                        activeHypos=r.activeHypos, finalStatesN=r.finalStatesN, maxActive=r.maxActiveSeen, arcs=arcs[u], words=words[u]))
    return out


def check_ok(ro, rd, maxPath, arcOut, want_paths=True, max_active=True):
    """every field of the record the oracle has a value for, and the path: whole when it fits maxPath, else cut there with the full counts reported
    (max_active=False: the largest list of a frame is not compared)"""
    nA, nW = len(ro["arcs"]), len(ro["words"])
    fits = nA <= maxPath or not want_paths
    assert rd["status"] == (OK if fits else E_DIMENSION)
    assert rd["frames"] == ro["frames"] and rd["reachedFinal"] == ro["reachedFinal"] and rd["finalStatesN"] == ro["finalStatesN"]
    assert np.float32(rd["ac"]).view(np.uint32) == np.float32(ro["ac"]).view(np.uint32)
    assert np.float32(rd["lm"]).view(np.uint32) == np.float32(ro["lm"]).view(np.uint32)
    assert rd["score"] == ro["score"]
    assert rd["activeHypos"] == ro["activeHypos"]
    if max_active:
        assert rd["maxActive"] == int(max(ro["activeCount"]))
    if fits:
        assert rd["nArcs"] == nA and rd["nWords"] == nW
    if not want_paths:
        return
    k = min(nA, maxPath)
    assert np.array_equal(rd["arcs"][:k], ro["arcs"][:k])
    wexp = np.array([arcOut[a] for a in ro["arcs"][:k] if arcOut[a] != 0], np.uint32)      # the words of the arcs that were written
    if fits:
        assert np.array_equal(wexp, ro["words"])
    assert np.array_equal(rd["words"][:len(wexp)], wexp)


def check_failed(rd, status, T):
    assert rd["status"] == status and rd["frames"] == T - 1
    assert rd["nArcs"] == 0 and rd["nWords"] == 0


def check_batch(case, out, idx, nfr, maxPath, want_paths=True):
    for i, u in enumerate(idx):
        if nfr[i] == 0:
            check_failed(out[i], E_ITERATOR, 0)
        else:
            check_ok(case["ref"][u], out[i], maxPath, case["arcOut"], want_paths)


def planned(capfd, what):
    """every launch since the last call ran as the case means it to: the plan line of DSR_VITERBI_SEG_VERBOSE names the mode"""
    lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[dsr viterbi]") and "utterances on" in l]
    assert lines and all(what in l for l in lines), (what, lines)


def eps_runs(arcIn, path):
    """(epsilon arcs at the end of the path, longest run of epsilon arcs before that)"""
    e = [int(arcIn[a] == 0) for a in path]
    tail = 0
    while tail < len(e) and e[len(e) - 1 - tail]:
        tail += 1
    inner = cur = 0
    for v in e[: len(e) - tail]:
        cur = cur + 1 if v else 0; inner = max(inner, cur)
    return tail, inner


def test_ragged_batch_on_three_workgroups(dsr, cuda, case, monkeypatch, capfd):
    """12 utterances on 3 workgroups, each run to its end (no time slicing): every slot decodes several utterances and its arena is reused by each of them, so
    the chain is followed before the slot moves on and k_traceback starts from the hop records; the heads are kept by utterance."""
    monkeypatch.setenv("DSR_VITERBI_SEG", "0"); monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=8192, streams=3); dec.set(case["gd"])
    out = decode(dsr, cuda, dec, case["sc"], NFR, 256)
    check_batch(case, out, range(len(NFR)), NFR, 256)
    planned(capfd, "run to completion")


def test_epsilon_paths(dsr, cuda, case, monkeypatch, capfd):
    """End records (the epsilon path into the final state) of one to four hops and epsilon paths behind emitting arcs are on the decoded best paths, and the
    paths are the oracle's.  As many workgroups as utterances: workgroup u decodes utterance u and nothing else, the records stay in the slots' arenas and
    k_traceback follows them."""
    monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=8192, streams=len(NFR)); dec.set(case["gd"])
    out = decode(dsr, cuda, dec, case["sc"], NFR, 256)
    check_batch(case, out, range(len(NFR)), NFR, 256)
    planned(capfd, "run to completion")
    runs = [eps_runs(case["arcIn"], out[u]["arcs"][:out[u]["nArcs"]]) for u in range(len(NFR)) if NFR[u] > 0]
    assert {1, 2, 3, 4} <= {t for t, _ in runs}, runs                       # end records of every chain length
    assert max(i for _, i in runs) >= 2, runs                               # an expansion record with a path of two hops or more


def test_max_path_shorter_than_some_paths(dsr, cuda, case):
    """maxPath = 20: the long utterances report DSR_E_DIMENSION with their full counts and the first 20 arcs, the short ones between them are whole."""
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=8192, streams=3); dec.set(case["gd"])
    out = decode(dsr, cuda, dec, case["sc"], NFR, 20)
    check_batch(case, out, range(len(NFR)), NFR, 20)
    st = [o["status"] for o in out]
    assert st.count(E_DIMENSION) >= 3 and st.count(OK) >= 3, st
    for u, o in enumerate(out):
        if o["status"] == E_DIMENSION:
            assert o["nArcs"] == len(case["ref"][u]["arcs"]) > 20 and o["nWords"] == len(case["ref"][u]["words"])


def test_counts_without_paths(dsr, cuda, case):
    """want_paths = False: nothing is written, the counts are the whole path's and a short maxPath is no error."""
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=8192, streams=3); dec.set(case["gd"])
    out = decode(dsr, cuda, dec, case["sc"], NFR, 20, want_paths=False)
    check_batch(case, out, range(len(NFR)), NFR, 20, want_paths=False)
    assert max(o["nArcs"] for o in out) > 20


def test_failure_next_to_success(dsr, oracle, cuda):
    """One utterance outgrows maxActive (DSR_E_ALLOCATION: no arcs, no words) between neighbours that do not.  No beam (1e9), so a token is dropped only where
    its distribution costs 1e12: utterance 2 scores every distribution alike and keeps every reachable state; its neighbours have three usable distributions.
    What a frame writes is at most the tokens within the beam of its best (the last frame and the end expansion: all of them) -- counted on the oracle's lists."""
    arcs, fin = synth.random_wfst(200, NDIST, seed=75, eps_frac=0.2, nFinal=20, out_frac=0.3)
    go, gd = both_graphs(dsr, oracle, arcs, fin)
    arcOut = go.export()["arcOut"]
    rng = np.random.default_rng(75)
    nfr = [30, 17, 30, 24, 9]
    sc = rng.uniform(0, 10, (5, 30, NDIST)).astype(np.float32)
    for u in (0, 1, 3, 4):
        dear = np.ones(NDIST, bool); dear[rng.choice(NDIST, 3, replace=False)] = False
        sc[u][:, dear] = 1e12
    maxActive = 128
    ref = [go.decode(sc[u, :nfr[u]], beam=1e9, lmScale=1.0, dump=True) for u in range(5)]

    def written(ro):
        off = ro["dumpOff"]; s = ro["dumpAc"].astype(np.float64) + ro["dumpLm"].astype(np.float64); w = [int(off[-1] - off[-2]), ro["finalStatesN"]]
        for t in range(len(off) - 1):
            x = s[off[t]:off[t + 1]]; w.append(int((x <= x.min() + 1e9).sum()))
        return max(w)
    need = [written(r) for r in ref]
    assert need[2] > maxActive and max(need[u] for u in (0, 1, 3, 4)) <= maxActive, need
    dec = dsr.Decoder(beam=1e9, lmScale=1.0, maxActive=maxActive, maxCandidates=65536, streams=2); dec.set(gd)
    out = decode(dsr, cuda, dec, sc, nfr, 256)
    check_failed(out[2], E_ALLOCATION, nfr[2])
    for u in (0, 1, 3, 4):
        check_ok(ref[u], out[u], 256, arcOut, max_active=False)


@pytest.mark.parametrize("seg,streams,any_,rep", [(7, 3, "1", 1), (5, 9, "2", 1), (16, 4, "1", 1), (7, 64, None, 6)])
def test_time_sliced(dsr, cuda, case, monkeypatch, capfd, seg, streams, any_, rep):
    """Segments of a few frames: an utterance's back-pointer records are pool indices written by several workgroups, the head points into the pool, and
    utterances end in different segments.  One queue on 3-9 workgroups (DSR_VITERBI_SEG_ANY), and the queues bound to the XCDs: 72 utterances on 64 workgroups."""
    monkeypatch.setenv("DSR_VITERBI_SEG", str(seg)); monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    if any_:
        monkeypatch.setenv("DSR_VITERBI_SEG_ANY", any_)
    idx = list(range(len(NFR))) * rep; nfr = NFR * rep
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=8192, streams=streams); dec.set(case["gd"])
    out = decode(dsr, cuda, dec, np.tile(case["sc"], (rep, 1, 1)), nfr, 256)
    check_batch(case, out, idx, nfr, 256)
    planned(capfd, "time-sliced, one queue" if any_ else "time-sliced, XCD-bound queues")


@pytest.mark.parametrize("mode", ["lattice", "topN", "dump"])
def test_other_modes(dsr, oracle, cuda, case, mode):
    """The instantiation with lattice bookkeeping, topN and the token dump compiled in leaves its heads too: lattice mode with an arena per utterance."""
    idx = [0, 8, 3, 5] if mode != "dump" else [7]
    nfr = [NFR[u] for u in idx]
    kw = dict(latticeTokens=400000) if mode == "lattice" else dict(topN=25) if mode == "topN" else {}
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=8192, streams=2, **kw); dec.set(case["gd"])
    if mode == "dump":
        dec.enable_dump(True)
    out = decode(dsr, cuda, dec, case["sc"][idx], nfr, 256)
    if mode == "topN":
        for i, u in enumerate(idx):
            ro = case["go"].decode(case["sc"][u, :nfr[i]], beam=BEAM, lmScale=LMSCALE, topN=25)
            assert ro["rc"] == 0
            check_ok(ro, out[i], 256, case["arcOut"])
    else:
        check_batch(case, out, idx, nfr, 256)
    if mode == "lattice":
        assert dec.lattice(0).data["from"].size > 0                                 # the utterance's own arena is still what the lattice is built from


@pytest.mark.parametrize("seg", [0, 7])
def test_decoder_reused_with_another_batch(dsr, cuda, case, monkeypatch, capfd, seg):
    """The same decoder, 12 utterances and then 5 others: the buffers are reused, and no head of the first run is followed in the second -- utterance 1 of the
    second run has no frame where the first run's had 37.  Run to completion (hop records left by k_viterbi) and time-sliced (k_traceback follows the pool)."""
    monkeypatch.setenv("DSR_VITERBI_SEG", str(seg)); monkeypatch.setenv("DSR_VITERBI_SEG_ANY", "1"); monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=8192, streams=3); dec.set(case["gd"])
    out = decode(dsr, cuda, dec, case["sc"], NFR, 256)
    check_batch(case, out, range(len(NFR)), NFR, 256)
    idx = [11, 2, 0, 9, 3]; nfr = [NFR[u] for u in idx]
    out = decode(dsr, cuda, dec, case["sc"][idx], nfr, 256)
    check_batch(case, out, idx, nfr, 256)
    out = decode(dsr, cuda, dec, case["sc"], NFR, 64)                         # and back, with another maxPath
    check_batch(case, out, range(len(NFR)), NFR, 64)
    planned(capfd, "time-sliced, one queue" if seg else "run to completion")


@pytest.mark.parametrize("how", ["bound", "queue", "sliced"])
def test_hop_capacity(dsr, oracle, cuda, monkeypatch, capfd, how):
    """The chain is cut at 2 x maxCandidates hops and says so (DSR_E_ALLOCATION).  Reachable only with a maxCandidates far below its default of 8 x maxActive: on a
    chain of states every frame places one token, so maxCandidates = 2 is enough to decode, and an utterance of ten frames has ten hops where four are kept;
    its neighbour of three frames is whole.  bound: a workgroup per utterance, k_traceback stops its own walk; queue: three utterances on two workgroups, the walk
    in k_viterbi stops and hands four hops over; sliced: segments of three frames, k_traceback stops its walk through the pool."""
    arcs = [(i, i + 1, 1 + i % NDIST, 1 + i if i % 2 else 0, 0.5) for i in range(20)]
    go, gd = both_graphs(dsr, oracle, arcs, [(20, 0.0)])
    nfr = [10, 3] if how == "bound" else [10, 3, 10]
    sc = np.random.default_rng(3).uniform(0, 10, (len(nfr), 10, NDIST)).astype(np.float32)
    monkeypatch.setenv("DSR_VITERBI_SEG", "3" if how == "sliced" else "0"); monkeypatch.setenv("DSR_VITERBI_SEG_ANY", "1"); monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    dec = dsr.Decoder(beam=BEAM, lmScale=LMSCALE, maxActive=64, maxCandidates=2, streams=2); dec.set(gd)
    out = decode(dsr, cuda, dec, sc, nfr, 64)
    planned(capfd, "time-sliced, one queue" if how == "sliced" else "run to completion")
    for u, t in enumerate(nfr):
        if t == 10:
            assert out[u]["status"] == E_ALLOCATION and out[u]["frames"] == 9
    ro = go.decode(sc[1, :3], beam=BEAM, lmScale=LMSCALE)
    assert ro["rc"] == 0 and len(ro["arcs"]) == 3
    check_ok(ro, out[1], 64, go.export()["arcOut"])
