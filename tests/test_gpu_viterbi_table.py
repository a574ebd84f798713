"""The decoder's LDS state table in its two forms: 32 768 one-word buckets (flag | key or side record | slot; graphs of at most 65 535
states) and the two arrays of 16 384 words (every other graph, and DSR_VITERBI_TABLE=wide).  Every case is decoded with both, the two
results are compared in every field, and both are compared with the oracle's bits -- so the two-array table keeps its coverage now that
small graphs no longer reach it."""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

KEYS = ["status", "score", "ac", "lm", "frames", "reachedFinal", "activeHypos", "maxActive", "placements", "registerFrames", "finalStatesN"]


def _bucket(dst):
    return ((dst * 2654435761) % (1 << 32) >> 7) & 32767        # k_viterbi's table_insert on the narrow table (32 768 buckets)


def _graphs(dsr, oracle, arcs, fin):
    go, gd = oracle.Wfst(), dsr.Wfst()
    for a in arcs:
        go.add_arc(*a); gd.add_arc(*a)
    for s, c in fin:
        go.add_final(s, c); gd.add_final(s, c)
    return go, gd


def _check_decode(ro, rd):
    assert rd["status"] == 0
    assert rd["frames"] == ro["frames"]
    assert rd["reachedFinal"] == ro["reachedFinal"]
    assert np.float32(rd["ac"]).view(np.uint32) == np.float32(ro["ac"]).view(np.uint32)
    assert np.float32(rd["lm"]).view(np.uint32) == np.float32(ro["lm"]).view(np.uint32)
    assert rd["score"] == ro["score"]
    assert np.array_equal(rd["arcs"], ro["arcs"])
    assert np.array_equal(rd["words"], ro["words"])
    assert rd["activeHypos"] == ro["activeHypos"]


def _check_dump(ro, d):
    assert np.array_equal(d["frameOff"], ro["dumpOff"])
    assert np.array_equal(d["node"], ro["dumpNode"])
    assert np.array_equal(d["arc"], ro["dumpArc"])
    assert np.array_equal(d["ac"].view(np.uint32), ro["dumpAc"].view(np.uint32))
    assert np.array_equal(d["lm"].view(np.uint32), ro["dumpLm"].view(np.uint32))


def _same(a, b):
    assert len(a) == len(b)
    for u, (x, y) in enumerate(zip(a, b)):
        assert [x[k] for k in KEYS] == [y[k] for k in KEYS], u
        assert np.array_equal(x["arcs"], y["arcs"]) and np.array_equal(x["words"], y["words"]), u


def _both(monkeypatch, capfd, run):
    """run() with the table the launch picks and with DSR_VITERBI_TABLE=wide -> (default result, wide result, table named by the default launch)"""
    monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    monkeypatch.delenv("DSR_VITERBI_TABLE", raising=False)
    capfd.readouterr()
    a = run()
    err = capfd.readouterr().err
    monkeypatch.setenv("DSR_VITERBI_TABLE", "wide")
    b = run()
    errw = capfd.readouterr().err
    monkeypatch.delenv("DSR_VITERBI_TABLE", raising=False)
    assert "wide state table" in errw and "narrow state table" not in errw
    kinds = set(k for k in ("narrow", "wide") if (k + " state table") in err)
    assert len(kinds) == 1, err
    return a, b, kinds.pop()


def _by_id_graph(nStates, nDist, arcs):
    """Arc list in which node index == state id for states 0 .. nStates-1: a node's index is the order in which its state is first named, so
    the hub's self loop comes first and every other state is named by a self loop of its own, in order, before the arcs of the case
    (the states the case does not use are never reached)."""
    out = [(0, 0, 1, 0, 1.0)]
    out += [(s, s, 1 + s % nDist, 0, 2.0) for s in range(1, nStates)]
    return out + list(arcs)


def _arrivals(eo, ro, f):
    """Frame f + 1 of a graph without epsilon arcs, pruning off: per destination node the arcs that arrive there, in the reference's order
    (token list order x arc order), out of the oracle's dump of frame f."""
    off = ro["dumpOff"]; arr = {}
    for nd in ro["dumpNode"][off[f]:off[f + 1]]:
        for a in range(eo["arcOff"][nd], eo["arcOff"][nd + 1]):
            arr.setdefault(int(eo["arcDst"][a]), []).append(a)
    return arr


def test_frames_that_needed_two_passes(dsr, oracle, cuda, monkeypatch, capfd):
    """~23 k placements a frame: two passes over the two-array table, one over the one-word buckets."""
    import torch
    arcs, fin = synth.random_wfst(4000, 64, seed=11, ties=True)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    T = 14
    sc = np.round(np.random.default_rng(11).uniform(0, 4, (2, T, 64))).astype(np.float32)
    ros = [go.decode(sc[u], beam=1e9, lmScale=2.0, dump=(u == 0)) for u in range(2)]
    assert all(r["rc"] == 0 for r in ros)
    assert all(int(c) >= 3870 for c in ros[0]["activeCount"][T // 2:T]) and int(ros[0]["activeCount"][T - 1]) == 3892      # the lists the second half expands: full

    def run(frames=T):
        dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=2); dec.set(gd)
        return dec.decode_batch(torch.from_numpy(np.ascontiguousarray(sc[:, :frames])).to(cuda))
    a, b, kind = _both(monkeypatch, capfd, run)
    assert kind == "narrow"
    _same(a, b)
    half = run(T // 2)
    for u in range(2):
        _check_decode(ros[u], a[u])
        assert a[u]["registerFrames"] == T
        # frames T/2 .. T-1: both totals also hold one end expansion -- a few dozen placements (50 final states in 4 000), nothing against the margin asked here
        late = (a[u]["placements"] - half[u]["placements"]) / (T - T // 2)
        print("utterance %d: %.0f placements a frame in the second half" % (u, late))
        assert late > 12288 * 1.05

    def run_dump():
        dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=1); dec.set(gd); dec.enable_dump(True)
        out = dec.decode_batch(torch.from_numpy(sc[:1]).to(cuda))
        return out, dec.get_dump()
    for tab in (None, "wide"):
        if tab:
            monkeypatch.setenv("DSR_VITERBI_TABLE", tab)
        out, d = run_dump()
        _check_decode(ros[0], out[0]); _check_dump(ros[0], d)
        assert out[0]["registerFrames"] == T


@pytest.mark.parametrize("nNodes", [65535, 65536])
def test_key_range(dsr, oracle, cuda, monkeypatch, capfd, nNodes):
    """Keys at both ends of the 16-bit field (state + 1 = 2 and 65 535) and either side of bit 15; one state more and the launch takes the wide table."""
    import torch
    nDist, T = 6, 12
    S = [1, 32767, 32768, 65533, 65534]
    rng = np.random.default_rng(3)
    cost = lambda: float(np.float32(rng.uniform(0.1, 1.5)))
    arcs = [(0, s, 1 + int(rng.integers(nDist)), int(rng.integers(0, 3)), cost()) for s in S]
    for i, s in enumerate(S):
        arcs.append((s, 0, 1 + int(rng.integers(nDist)), 0, cost()))
        for t in (S[(i + 1) % 5], S[(i + 2) % 5]):                    # every state is reached from the hub and from two others: 65534 and 1 among them
            arcs.append((s, t, 1 + int(rng.integers(nDist)), int(rng.integers(0, 3)), cost()))
    arcs.append((32768, 65534, 1 + int(rng.integers(nDist)), 0, cost())); arcs.append((65533, 1, 1 + int(rng.integers(nDist)), 0, cost()))
    if nNodes == 65536:
        arcs.append((65534, 65535, 1 + int(rng.integers(nDist)), 0, cost()))
    go, gd = _graphs(dsr, oracle, _by_id_graph(65535, nDist, arcs), [(S[0], 0.0)])     # (a final state that is named already: no node of its own)
    eo = go.export()
    assert eo["nodeState"].size == nNodes and all(int(eo["nodeState"][s]) == s for s in S)
    sc = rng.uniform(0, 3, (1, T, nDist)).astype(np.float32)
    ro = go.decode(sc[0], beam=1e9, lmScale=3.0, dump=True)
    assert ro["rc"] == 0
    # the case is what it is meant to be: some state takes a later arrival that wins, some state one that loses
    won = lost = 0
    off = ro["dumpOff"]
    for f in range(T - 1):
        arr = _arrivals(eo, ro, f)
        nodes = ro["dumpNode"][off[f + 1]:off[f + 2]]; win = ro["dumpArc"][off[f + 1]:off[f + 2]]
        assert sorted(arr) == sorted(int(n) for n in nodes)
        for nd, wa in zip(nodes, win):
            if len(arr[int(nd)]) > 1:
                assert int(wa) in arr[int(nd)]
                won += int(wa) != arr[int(nd)][0]; lost += int(wa) == arr[int(nd)][0]
    assert won > 0 and lost > 0, (won, lost)

    def run():
        dec = dsr.Decoder(beam=1e9, lmScale=3.0, maxActive=8192, streams=1); dec.set(gd); dec.enable_dump(True)
        out = dec.decode_batch(torch.from_numpy(sc).to(cuda))
        return out, dec.get_dump()
    (a, da), (b, db), kind = _both(monkeypatch, capfd, run)
    assert kind == ("narrow" if nNodes == 65535 else "wide")
    _same(a, b)
    for out, d in ((a, da), (b, db)):
        _check_decode(ro, out[0]); _check_dump(ro, d)
        assert out[0]["registerFrames"] == T


def test_probe_chain_wraps(dsr, oracle, cuda, monkeypatch, capfd):
    """States whose buckets are the last eight and the first eight of the narrow table: fourteen of them hash to the last eight buckets, so
    the probe chains run past the table's end into the first buckets and push the states that live there further on."""
    import torch
    nDist, T = 8, 10
    # every state the narrow table's key field can hold whose bucket lies in the window (33 of them; states above 65 534 take the wide table)
    S = [d for d in range(1, 65535) if _bucket(d) >= 32760 or _bucket(d) <= 7]
    assert len(S) == 33 and sum(1 for d in S if _bucket(d) >= 32760) == 14
    rng = np.random.default_rng(8)
    cost = lambda: float(np.float32(rng.uniform(0.1, 1.5)))
    arcs = []
    for i, s in enumerate(S):
        arcs.append((0, s, 1 + int(rng.integers(nDist)), int(rng.integers(0, 3)), cost()))
        arcs.append((s, 0, 1 + int(rng.integers(nDist)), 0, cost()))
        for t in (S[(i + 1) % len(S)], S[(i + 7) % len(S)], S[(i + 16) % len(S)]):
            arcs.append((s, t, 1 + int(rng.integers(nDist)), 0, cost()))
    go, gd = _graphs(dsr, oracle, _by_id_graph(65535, nDist, arcs), [(S[0], 0.0)])     # (a final state that is named already: no node of its own)
    eo = go.export()
    assert eo["nodeState"].size == 65535 and all(int(eo["nodeState"][s]) == s for s in S)
    sc = rng.uniform(0, 3, (1, T, nDist)).astype(np.float32)
    ro = go.decode(sc[0], beam=1e9, lmScale=3.0, dump=True)
    assert ro["rc"] == 0
    off = ro["dumpOff"]
    assert set(S) <= set(int(n) for n in ro["dumpNode"][off[T - 1]:off[T]])        # all of them are in the table together

    def run():
        dec = dsr.Decoder(beam=1e9, lmScale=3.0, maxActive=8192, streams=1); dec.set(gd); dec.enable_dump(True)
        out = dec.decode_batch(torch.from_numpy(sc).to(cuda))
        return out, dec.get_dump()
    (a, da), (b, db), kind = _both(monkeypatch, capfd, run)
    assert kind == "narrow"
    _same(a, b)
    for out, d in ((a, da), (b, db)):
        _check_decode(ro, out[0]); _check_dump(ro, d)
        assert out[0]["registerFrames"] == T


def test_chains_of_later_arrivals(dsr, oracle, cuda, monkeypatch, capfd):
    """Exact ties everywhere: states with several later arrivals -- the push that keeps the slot field, and the replay of multi-record chains."""
    import torch
    arcs, fin = synth.random_wfst(1500, 64, seed=9, ties=True)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    sc = np.round(np.random.default_rng(77).uniform(0, 6, (1, 80, 64))).astype(np.float32)
    ro = go.decode(sc[0], beam=15.0, lmScale=1.0, dump=True)
    assert ro["rc"] == 0

    def run():
        dec = dsr.Decoder(beam=15.0, lmScale=1.0, maxActive=8192, streams=1); dec.set(gd); dec.enable_dump(True)
        out = dec.decode_batch(torch.from_numpy(sc).to(cuda))
        return out, dec.get_dump()
    (a, da), (b, db), kind = _both(monkeypatch, capfd, run)
    assert kind == "narrow"
    _same(a, b)
    for out, d in ((a, da), (b, db)):
        _check_decode(ro, out[0]); _check_dump(ro, d)


def test_time_sliced_narrow(dsr, oracle, cuda, monkeypatch, capfd):
    """Utterances put down and taken up between segments (one queue, 3 workgroups, 7 frames a segment): sliced = unsliced, narrow = wide, oracle's bits."""
    import torch
    seg, streams, U, T = 7, 3, 29, 45
    arcs, fin = synth.random_wfst(1500, 48, seed=31, eps_frac=0.2)
    go, gd = _graphs(dsr, oracle, arcs, fin)
    rng = np.random.default_rng(77)
    monkeypatch.setenv("DSR_VITERBI_SEG_ANY", "1")
    sc = rng.uniform(0, 8, (U, T, 48)).astype(np.float32)
    nfr = [int(v) for v in rng.integers(2, T + 1, U)]
    nfr[0] = T; nfr[3] = 1; nfr[5] = 0; nfr[9] = seg; nfr[10] = seg + 1; nfr[11] = 2 * seg - 1

    def run(segv):
        monkeypatch.setenv("DSR_VITERBI_SEG", str(segv))
        dec = dsr.Decoder(beam=22.0, lmScale=12.0, streams=streams, maxActive=8192); dec.set(gd)
        return dec.decode_batch(torch.from_numpy(sc).to(cuda), torch.tensor(nfr, dtype=torch.int32, device=cuda))
    a, aw, kind = _both(monkeypatch, capfd, lambda: run(seg))
    assert kind == "narrow"
    b, bw, _ = _both(monkeypatch, capfd, lambda: run(0))
    _same(a, aw); _same(b, bw); _same(a, b)
    for u in range(10):
        if nfr[u] == 0:
            assert a[u]["status"] == 9
        else:
            ro = go.decode(sc[u, :nfr[u]], beam=22.0, lmScale=12.0)
            assert ro["rc"] == 0
            _check_decode(ro, a[u])
