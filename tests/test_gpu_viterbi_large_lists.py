"""k_viterbi on frames whose token list is longer than 2 048 tokens: the frame that writes such a list lays out the next frame's placement slots (bitmap of
run starts + group table) for lists of up to 4 096 tokens; longer lists, lists with a token that has no arcs, lists whose placements do not fit the register
path, frames without pruning (dump mode, the last frame) and the first frame of a resumed segment build the layout themselves in P1/P2.

Every case is compared with oracle/orc_wfst.c: per-frame token lists bit for bit in dump mode; score, ac, lm, activeHypos, placements, arcs, words and status
in normal mode.  The beam is 1e9, so every token of a list expands and the oracle's dump gives each frame's list size and placement count exactly: the path
every frame takes is PREDICTED from them (_paths) and compared with the decoder's own counts -- registerFrames, and laidOutFrames, the register-path frames
the frame before had laid out -- so a case that stopped exercising the path it is named for fails."""
import numpy as np
import pytest

from tests import synth

pytestmark = pytest.mark.gpu

LAY_TOKENS = 4096          # longest list a frame lays out for the next one (4 x 1024 threads)
REG_PLACEMENTS = 24576     # most placements of a register-path frame, narrow and wide table alike
REG_TOKENS = 8190          # most expanding tokens of a register-path frame


def _graphs(dsr, oracle, arcs, fin):
    go, gd = oracle.Wfst(), dsr.Wfst()
    for a in arcs:
        go.add_arc(*a); gd.add_arc(*a)
    for s, c in fin:
        go.add_final(s, c); gd.add_final(s, c)
    return go, gd


def _counts(eo):
    """Per node: placements a token there makes in a frame (emitting arcs behind every epsilon path, no recombination: the graph's expansion records) and
    in the end expansion without its own final state (epsilon paths that enter a final state)."""
    off, dst, ain, fin = eo["arcOff"], eo["arcDst"], eo["arcIn"], eo["nodeFinal"]
    n = fin.size
    x = np.zeros(n, np.int64); e = np.zeros(n, np.int64); done = np.zeros(n, bool)
    for root in range(n):                        # iterative depth-first walk (epsilon arcs only go forward: no cycle)
        stack = [root]
        while stack:
            v = stack[-1]
            if done[v]:
                stack.pop(); continue
            todo = [int(dst[a]) for a in range(off[v], off[v + 1]) if ain[a] == 0 and not done[dst[a]]]
            if todo:
                stack.extend(todo); continue
            cx = ce = 0
            for a in range(off[v], off[v + 1]):
                if ain[a] == 0:
                    d = int(dst[a]); cx += x[d]; ce += (1 if fin[d] else 0) + e[d]
                else:
                    cx += 1
            x[v] = cx; e[v] = ce; done[v] = True; stack.pop()
    return x, e


def _frames(eo, x, ro, T, beam=1e9):
    """From the oracle's dump: per frame the tokens it expands (frame f + 1: the tokens of frame f's list within the beam of f's best emitting placement,
    decoder.h:586-588 -- all of them at beam 1e9), those of them without arcs, and its placements."""
    off = ro["dumpOff"]; lists = [np.array([0])]                                                 # (node 0 = the initial state)
    for f in range(T - 1):
        sl = slice(off[f], off[f + 1])
        keep = ~((ro["dumpAc"][sl] + ro["dumpLm"][sl]).astype(np.float64) > ro["topScore"][f] + beam)
        lists.append(ro["dumpNode"][sl][keep])
    n = [len(l) for l in lists]; zero = [int((x[l] == 0).sum()) for l in lists]; C = [int(x[l].sum()) for l in lists]
    return n, zero, C


def _paths(n, zero, C, T, seg=0):
    """-> (register-path frames, those of them laid out by the frame before), as k_viterbi decides them."""
    reg = [C[f] <= REG_PLACEMENTS and n[f] - zero[f] <= REG_TOKENS for f in range(T)]
    laid = [f > 0 and reg[f - 1] and n[f] <= LAY_TOKENS and zero[f] == 0 and C[f] <= REG_PLACEMENTS and not (seg > 0 and f % seg == 0) for f in range(T)]
    return sum(reg), sum(laid)


def _placements(eo, x, e, ro, T, C):
    off = ro["dumpOff"]; last = ro["dumpNode"][off[T - 1]:off[T]]
    return sum(C) + int((eo["nodeFinal"][last] != 0).sum() + e[last].sum())


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


def _dead_end(S):
    """Arcs into a state that has none of its own, from three states the random graph reaches early."""
    return [(s, S, 1 + s % 7, 0, 0.5) for s in (1, 2, 3, 5, 8, 13, 21, 34)]


# name -> states, seed, epsilon share, frames, what the SATURATED list must be: (tokens min, max, placements min, max), and the path the frames behind it take
CASES = {
    "above_2048":       dict(S=2600, seed=51, eps=0.1, T=14, sat=(2049, 4096, 8193, REG_PLACEMENTS), path="laid"),
    "at_4096":          dict(S=4205, seed=61, eps=0.0, T=14, sat=(4096, 4096, 8193, REG_PLACEMENTS), path="laid"),
    "above_4096":       dict(S=4190, seed=61, eps=0.0, T=14, sat=(4097, 4100, 8193, REG_PLACEMENTS), path="p1p2"),
    "below_placements": dict(S=4150, seed=53, eps=0.1, T=14, sat=(2049, 4096, 23000, REG_PLACEMENTS), path="laid"),
    "above_placements": dict(S=4200, seed=53, eps=0.1, T=14, sat=(2049, 4096, REG_PLACEMENTS + 1, 27000), path="memory"),
    "dead_end":         dict(S=2600, seed=51, eps=0.1, T=14, sat=(2049, 4096, 8193, REG_PLACEMENTS), path="p1p2", extra=_dead_end),
}


@pytest.fixture(scope="module")
def built(dsr, oracle):
    """Graphs, scores and oracle results of every case, made once: ragged lengths -- full, shorter, one frame, none."""
    cache = {}

    def get(name):
        if name in cache:
            return cache[name]
        c = CASES[name]; S, T = c["S"], c["T"]
        arcs, fin = synth.random_wfst(S, 64, seed=c["seed"], eps_frac=c["eps"])
        if c.get("extra"):
            arcs = arcs + c["extra"](S)
        go, gd = _graphs(dsr, oracle, arcs, fin)
        eo = go.export(); x, e = _counts(eo)
        nfr = [T, T - 3, 1, 0]
        sc = np.random.default_rng(c["seed"]).uniform(0, 4, (len(nfr), T, 64)).astype(np.float32)
        ros = [go.decode(sc[u, :nfr[u]], beam=1e9, lmScale=2.0, dump=True) if nfr[u] > 0 else None for u in range(len(nfr))]
        assert all(r is None or r["rc"] == 0 for r in ros)
        fr = [_frames(eo, x, ros[u], nfr[u]) if nfr[u] > 0 else None for u in range(len(nfr))]
        # the case is what it is named for: the saturated list (what the last frames expand) lies where it should, on the CPU, before any GPU work
        n, zero, C = fr[0]; lo, hi, clo, chi = c["sat"]
        assert lo <= n[T - 1] <= hi and n[T - 1] == n[T - 2] and clo <= C[T - 1] <= chi, (name, n, C)
        assert (zero[T - 1] > 0) == bool(c.get("extra")), (name, zero)
        cache[name] = dict(go=go, gd=gd, eo=eo, x=x, e=e, sc=sc, nfr=nfr, ros=ros, fr=fr, T=T)
        return cache[name]
    return get


def _run(dsr, cuda, b, streams=2, nfr=None, **kw):
    import torch
    nfr = b["nfr"] if nfr is None else nfr
    dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=streams, **kw); dec.set(b["gd"])
    return dec, dec.decode_batch(torch.from_numpy(b["sc"][:len(nfr)]).to(cuda), torch.tensor(nfr, dtype=torch.int32, device=cuda))


def _check_case(b, out, path, seg=0):
    T = b["T"]
    for u, nf in enumerate(b["nfr"]):
        if nf == 0:
            assert out[u]["status"] == 9
            continue
        ro = b["ros"][u]; n, zero, C = b["fr"][u]
        _check_decode(ro, out[u])
        assert out[u]["placements"] == _placements(b["eo"], b["x"], b["e"], ro, nf, C)
        reg, laid = _paths(n, zero, C, nf, seg)
        print("utterance %d: %d frames, %d on the register path, %d of them laid out by the frame before (expected %d, %d); last list %d tokens, %d placements" %
              (u, nf, out[u]["registerFrames"], out[u]["laidOutFrames"], reg, laid, n[nf - 1], C[nf - 1]))
        assert (out[u]["registerFrames"], out[u]["laidOutFrames"]) == (reg, laid)
    # ... and the frames behind the saturated list of the full-length utterance take the path the case is named for
    n, zero, C = b["fr"][0]; reg, laid = _paths(n, zero, C, T, seg); big = sum(1 for f in range(T) if n[f] > 2048)
    assert big >= 4
    if path == "laid":
        assert laid >= big - 1 - (T // seg if seg else 0) and reg == T
    elif path == "p1p2":
        own = sum(1 for f in range(T) if n[f] > LAY_TOKENS or (n[f] > 2048 and zero[f] > 0))      # large lists that must build their own layout
        assert reg == T and own >= 4 and reg - laid >= own + 1
    else:
        assert T - reg >= 4 and reg - laid >= 1


@pytest.mark.parametrize("table", ["narrow", "wide"])
@pytest.mark.parametrize("name", list(CASES))
def test_large_lists(dsr, cuda, built, monkeypatch, capfd, name, table):
    b = built(name)
    monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    if table == "wide":
        monkeypatch.setenv("DSR_VITERBI_TABLE", "wide")
    else:
        monkeypatch.delenv("DSR_VITERBI_TABLE", raising=False)
    capfd.readouterr()
    _, out = _run(dsr, cuda, b)
    err = capfd.readouterr().err
    assert (table + " state table") in err, err
    assert "laid out by the frame before" in err                                # the same counts, summed over the batch, in the launch's verbose output
    tot = [int(w) for w in err.split("[dsr viterbi] frames:")[1].split("\n")[0].replace(",", " ").split() if w.isdigit()]
    ok = [o for o in out if o["status"] in (0, 5)]
    assert tot == [sum(o["laidOutFrames"] for o in ok), sum(o["registerFrames"] - o["laidOutFrames"] for o in ok), sum(o["frames"] + 1 - o["registerFrames"] for o in ok)]
    _check_case(b, out, CASES[name]["path"])
    # dump mode: the lists themselves, bit for bit (no pruning there, so no frame is laid out by the one before)
    import torch
    dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=1); dec.set(b["gd"]); dec.enable_dump(True)
    outd = dec.decode_batch(torch.from_numpy(b["sc"][:1]).to(cuda))
    _check_decode(b["ros"][0], outd[0]); _check_dump(b["ros"][0], dec.get_dump())
    assert outd[0]["laidOutFrames"] == 0


def test_large_lists_time_sliced(dsr, cuda, built, monkeypatch, capfd):
    """Seven utterances on two workgroups, five frames a segment: a resume falls between frames with lists above 2 048 tokens, and the first frame of a
    resumed segment builds its own layout."""
    import torch
    b = built("above_2048"); T, seg = b["T"], 5
    monkeypatch.setenv("DSR_VITERBI_SEG_ANY", "1"); monkeypatch.setenv("DSR_VITERBI_SEG", str(seg)); monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")
    order = [0, 1, 2, 3, 0, 1, 0]                                                # (utterances of the case, some of them twice)
    nfr = [b["nfr"][i] for i in order]
    sc = np.ascontiguousarray(b["sc"][order])
    dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=2); dec.set(b["gd"])
    capfd.readouterr()
    out = dec.decode_batch(torch.from_numpy(sc).to(cuda), torch.tensor(nfr, dtype=torch.int32, device=cuda))
    assert "time-sliced, one queue" in capfd.readouterr().err
    bb = dict(b); bb["nfr"] = nfr; bb["ros"] = [b["ros"][i] for i in order]; bb["fr"] = [b["fr"][i] for i in order]
    _check_case(bb, out, "laid", seg=seg)
    n, zero, C = b["fr"][0]
    assert n[seg] > 2048 or n[2 * seg] > 2048                                    # a resume in front of a large list


def test_large_lists_pruned(dsr, oracle, cuda, built):
    """A beam that prunes: the list that is written (and laid out) is the part of the reference's list that passes the next frame's beam test."""
    import torch
    b = built("at_4096"); T, beam = b["T"], 17.0
    dec = dsr.Decoder(beam=beam, lmScale=2.0, maxActive=16384, streams=2); dec.set(b["gd"])
    out = dec.decode_batch(torch.from_numpy(b["sc"][:2]).to(cuda), torch.tensor([T, T - 3], dtype=torch.int32, device=cuda))
    for u, nf in enumerate((T, T - 3)):
        ro = b["go"].decode(b["sc"][u, :nf], beam=beam, lmScale=2.0, dump=True)
        assert ro["rc"] == 0
        _check_decode(ro, out[u])
        n, zero, C = _frames(b["eo"], b["x"], ro, nf, beam)
        print("utterance %d: lists kept by the reference %s, expanded %s, %d of %d frames laid out" % (u, list(ro["activeCount"]), n, out[u]["laidOutFrames"], nf))
        assert max(n) > 2048 and max(n) < max(ro["activeCount"])                 # lists above the old limit, and pruning at work
        assert out[u]["placements"] == _placements(b["eo"], b["x"], b["e"], ro, nf, C)
        assert (out[u]["registerFrames"], out[u]["laidOutFrames"]) == _paths(n, zero, C, nf) == (nf, nf - 1)


def test_large_lists_lattice(dsr, oracle, cuda, built):
    """Lattice mode keeps every placement in memory: no frame on the register path, none laid out, results and lattice as the oracle's."""
    import torch
    b = built("above_2048"); nfr = [9, 6]
    dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=2, latticeTokens=400000); dec.set(b["gd"])
    out = dec.decode_batch(torch.from_numpy(b["sc"][:2, :9].copy()).to(cuda), torch.tensor(nfr, dtype=torch.int32, device=cuda))
    for u in range(2):
        ro = b["go"].decode(b["sc"][u, :nfr[u]], beam=1e9, lmScale=2.0, lattice=(u == 1), eosX=7)
        assert ro["rc"] == 0
        _check_decode(ro, out[u])
        assert out[u]["registerFrames"] == 0 and out[u]["laidOutFrames"] == 0
    L = dec.lattice(1, eosX=7)
    for k in ("nodeFinal", "from", "to", "in", "out", "start", "end"):
        assert np.array_equal(ro["lattice"][k], L.data[k]), k
    for k in ("ac", "lm"):
        assert np.array_equal(ro["lattice"][k].view(np.int64), L.data[k].view(np.int64)), k
