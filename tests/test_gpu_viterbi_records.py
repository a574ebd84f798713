"""The expansion records of the register path and the narrow state table's wipe.

Part 1: the hot record carries lmScale x cost and lmScale x eps1, formed on the host when the graph is set; the expansion adds them where it used to
multiply.  A small graph drives every branch of the hop code (epsilon paths of 0, 1, 2, 3, 4 and 15 hops, exits after 5, 7 and 14; outputs on first,
middle and last hops; a silence arc entered from silence and non-silence edges and behind an epsilon hop) with costs 0.1f, 0.0f, 3e30f and -- in the
'tiny' graph -- 1e-30f, whose product with every scale used here is below 2^-60 and turns the penalty-free instantiation off by itself.

Part 2: on the narrow table the first arrival of a state zeroes the state's bucket in the fold; no block-wide wipe in the frame loop.  A word left
behind would change who is first in a later frame, or send a state down another probe chain: colliding buckets, parked first arrivals, a memory-path
frame between register-path frames, a failed utterance before others on the same workgroup, time slicing and the lattice mode.

Every decode is compared with the oracle bit for bit (per-frame lists where the mode dumps them), and runs with both tables, which must agree."""
import numpy as np
import pytest

from tests.test_gpu_viterbi_table import _arrivals, _both, _bucket, _by_id_graph, _check_decode, _check_dump, _graphs, _same

pytestmark = pytest.mark.gpu

SIL = 8          # input symbol of the silence model (distribution 7)
ND = 8


# ------------------------------------------------------------------ part 1
def _hop_graph(tiny):
    """-> arcs (from, to, input, output, cost), final states.  State 0 is the hub; chain j starts at A = 100 (j + 1): an emitting arc 0 -> A, h epsilon
    hops A -> A+1 -> .. -> A+h, an emitting arc A+h -> A+50, and from there back to the hub and on to the next chain's start."""
    E = [0.1, 0.0, 0.7, 1.3, 0.25, 2.5]; P = [0.0, 0.1, 0.45, 1.7]
    ne = [0]; npth = [0]

    def ce():
        ne[0] += 1; return E[ne[0] % len(E)]

    def cp():
        npth[0] += 1; return P[npth[0] % len(P)]
    arcs = [(0, 0, 1, 0, 0.1)]
    hops = [0, 1, 2, 3, 4, 15]
    outs = {1: {0: 3}, 2: {1: 4}, 3: {1: 5}, 4: {0: 6, 2: 7, 3: 8}, 15: {0: 9, 7: 10, 14: 11}}          # chain -> hop -> output symbol
    for j, h in enumerate(hops):
        A = 100 * (j + 1); B = A + 50
        arcs.append((0, A, 1 + j, 0, ce()))
        for k in range(h):
            arcs.append((A + k, A + k + 1, 0, outs.get(h, {}).get(k, 0), cp()))
        # chain 1 ends in a silence arc behind its epsilon hop (the edge before it is an epsilon edge); chains 0 and 3 end in arcs with an output
        arcs.append((A + h, B, SIL if h == 1 else 2 + j, 12 if h in (0, 3) else 0, ce()))
        if h == 15:
            for k in (5, 7, 14):
                arcs.append((A + k, B, 1 + k % 7, 13 if k == 7 else 0, ce()))
        arcs.append((B, 0, 1 + (j + 3) % 7, 0, ce()))
        arcs.append((B, 100 * ((j + 1) % len(hops) + 1), 1 + (j + 5) % 7, 0, ce()))
    # silence state: entered by a silence arc and by another one, with a silence self loop (taken from a silence edge and from a non-silence edge)
    arcs += [(0, 900, SIL, 0, 0.3), (0, 900, 3, 0, 0.4), (900, 900, SIL, 0, 0.2), (900, 0, 2, 14, 0.5), (900, 100, 4, 0, 0.0)]
    # 3e30f on an emitting arc and on a first epsilon hop
    arcs += [(0, 950, 4, 0, 3e30), (950, 0, 5, 2, 0.1), (0, 960, 2, 0, 0.1), (960, 961, 0, 0, 3e30), (961, 0, 6, 0, 0.7)]
    if tiny:       # 1e-30f on an emitting arc, on a first hop and on the second hop of a two-hop path
        arcs += [(0, 970, 3, 0, 1e-30), (970, 971, 0, 1, 1e-30), (971, 972, 0, 0, 1e-30), (972, 0, 7, 0, 0.1), (971, 0, 5, 0, 0.0)]
    return arcs, [(0, 0.0), (150, 0.5)]


T1 = 8
_hop_cache = {}


def _hop_case(dsr, oracle, tiny):
    """graph pair, scores and the oracle's decodes (filled as the cases ask for them), once per graph"""
    if tiny not in _hop_cache:
        arcs, fin = _hop_graph(tiny)
        go, gd = _graphs(dsr, oracle, arcs, fin)
        sc = np.random.default_rng(41 + int(tiny)).uniform(0, 3, (1, T1, ND)).astype(np.float32)
        _hop_cache[tiny] = dict(go=go, gd=gd, sc=sc, ref={})
    return _hop_cache[tiny]


def _hop_ref(b, lmScale, lmPenalty, silPenalty):
    k = (lmScale, lmPenalty, silPenalty)
    if k not in b["ref"]:
        ro = b["go"].decode(b["sc"][0], beam=1e35, lmScale=lmScale, lmPenalty=lmPenalty, silPenalty=silPenalty, silenceX=SIL, dump=True)
        assert ro["rc"] == 0
        b["ref"][k] = ro
    return b["ref"][k]


def test_hop_graph_is_what_it_is_meant_to_be(dsr, oracle):
    """expansion records with 0, 1, 2, 3, 4, 5, 7, 14 and 15 hops, and all of them taken: the last list holds the end of every chain"""
    b = _hop_case(dsr, oracle, True)
    ro = _hop_ref(b, 12.0, 0.0, 0.0)
    eo = b["go"].export()
    eps = {}
    for nd in range(eo["nodeState"].size):
        for a in range(eo["arcOff"][nd], eo["arcOff"][nd + 1]):
            if eo["arcIn"][a] == 0:
                eps.setdefault(nd, []).append(int(eo["arcDst"][a]))

    def depths(nd, d=0):
        out = {d} if any(eo["arcIn"][a] != 0 for a in range(eo["arcOff"][nd], eo["arcOff"][nd + 1])) else set()
        for t in eps.get(nd, []):
            out |= depths(t, d + 1)
        return out
    seen = set()
    for nd in set(int(n) for n in ro["dumpNode"]):
        seen |= depths(nd)
    assert {0, 1, 2, 3, 4, 5, 7, 14, 15} <= seen, seen
    state = eo["nodeState"]; off = ro["dumpOff"]
    last = set(int(state[n]) for n in ro["dumpNode"][off[T1 - 1]:off[T1]])
    assert {150, 250, 350, 450, 550, 650, 900, 950} <= last, last
    assert float(np.max(ro["dumpLm"])) > 1e31 and float(np.min(ro["dumpLm"][ro["dumpLm"] > 0])) < 1e-28          # 3e30f and 1e-30f made it into the scores


@pytest.mark.parametrize("pen", [False, True], ids=["nopen", "pen"])
@pytest.mark.parametrize("tiny", [False, True], ids=["plain", "tiny"])
@pytest.mark.parametrize("lmScale", [12.0, 9.3, 1e-3])
def test_scaled_costs(dsr, oracle, cuda, monkeypatch, capfd, lmScale, tiny, pen):
    """plain + nopen: the penalty-free instantiation (every product at least 2^-60); tiny: a product below 2^-60, the penalty instantiation whatever the
    penalties; pen: both penalties non-zero."""
    import torch
    b = _hop_case(dsr, oracle, tiny)
    lmP, silP = (0.37, -1.9) if pen else (0.0, 0.0)
    ro = _hop_ref(b, lmScale, lmP, silP)
    if tiny:
        assert lmScale * float(np.float32(1e-30)) < 2.0 ** -60
    else:
        assert lmScale * 0.1 >= 2.0 ** -60

    def run():
        dec = dsr.Decoder(beam=1e35, lmScale=lmScale, lmPenalty=lmP, silPenalty=silP, silenceX=SIL, maxActive=8192, streams=1); dec.set(b["gd"]); dec.enable_dump(True)
        out = dec.decode_batch(torch.from_numpy(b["sc"]).to(cuda))
        return out, dec.get_dump()
    (a, da), (w, dw), kind = _both(monkeypatch, capfd, run)
    assert kind == "narrow"
    _same(a, w)
    for out, d in ((a, da), (w, dw)):
        _check_decode(ro, out[0]); _check_dump(ro, d)
        assert out[0]["registerFrames"] == T1


def test_two_decoders_one_graph(dsr, oracle, cuda):
    """two decoders of different lmScale made from one Wfst, used in turn: each has its own scaled records"""
    import torch
    b = _hop_case(dsr, oracle, False)
    decs = []
    for lmScale in (12.0, 9.3):
        dec = dsr.Decoder(beam=1e35, lmScale=lmScale, silenceX=SIL, maxActive=8192, streams=1); dec.set(b["gd"]); dec.enable_dump(True)
        decs.append((lmScale, dec))
    for lmScale, dec in decs + decs[:1]:
        ro = _hop_ref(b, lmScale, 0.0, 0.0)
        out = dec.decode_batch(torch.from_numpy(b["sc"]).to(cuda))
        _check_decode(ro, out[0]); _check_dump(ro, dec.get_dump())
        assert out[0]["registerFrames"] == T1


# ------------------------------------------------------------------ part 2
def _colliding_pair():
    """the first two states above the ones the case uses that share a bucket of the narrow table"""
    seen = {}
    for d in range(20, 65535):
        k = _bucket(d)
        if k in seen:
            return seen[k], d
        seen[k] = d


TA = 6
_coll_cache = {}


def _collide_case(dsr, oracle):
    """(a): X and Y share a bucket (Y probes on).  Frame 1 puts tokens on P1..P6 (and Q1, Q2); from frame 2 on X is reached twice a frame and Y four
    times, and since the list order turns round every frame and X and Y feed the P's in another order than the hub does, the arrival order changes."""
    if not _coll_cache:
        X, Y = _colliding_pair()
        assert _bucket(X) == _bucket(Y) and X != Y
        rng = np.random.default_rng(19)
        cost = lambda: float(np.float32(rng.uniform(0.1, 1.5)))
        inp = lambda: 1 + int(rng.integers(ND))
        Pn = [1, 2, 3, 4, 5, 6]
        arcs = [(0, p, inp(), 0, cost()) for p in Pn]
        arcs += [(1, X, inp(), 1, cost()), (2, X, inp(), 0, cost())]
        arcs += [(p, Y, inp(), 2 if p == 4 else 0, cost()) for p in (3, 4, 5, 6)]
        arcs += [(X, p, inp(), 0, cost()) for p in (6, 3, 1)] + [(Y, p, inp(), 0, cost()) for p in (5, 2, 4)] + [(X, 0, inp(), 0, cost()), (Y, 0, inp(), 3, cost())]
        go, gd = _graphs(dsr, oracle, _by_id_graph(Y + 1, ND, arcs), [(0, 0.0), (X, 0.1)])
        eo = go.export()
        assert all(int(eo["nodeState"][s]) == s for s in Pn + [X, Y])
        sc = rng.uniform(0, 3, (1, TA, ND)).astype(np.float32)
        ro = go.decode(sc[0], beam=1e9, lmScale=3.0, dump=True)
        assert ro["rc"] == 0
        _coll_cache.update(X=X, Y=Y, go=go, gd=gd, eo=eo, sc=sc, ro=ro, plain=go.decode(sc[0], beam=1e9, lmScale=3.0))
    return _coll_cache


def test_collide_case_is_what_it_is_meant_to_be(dsr, oracle):
    b = _collide_case(dsr, oracle)
    X, Y, eo, ro = b["X"], b["Y"], b["eo"], b["ro"]
    firstX, firstY, lens = set(), set(), []
    for f in range(TA - 1):
        arr = _arrivals(eo, ro, f)
        lens.append((len(arr[X]), len(arr[Y])))
        firstX.add(arr[X][0]); firstY.add(arr[Y][0])
    # the first frame that reaches them: one later arrival at X, a chain of three at Y; the four frames behind it add the states' own self loops
    # (_by_id_graph) and bring the arrivals in other orders
    assert lens[0] == (2, 4) and lens[1:] == [(3, 5)] * 4, lens
    assert len(firstX) > 1 and len(firstY) > 2, (firstX, firstY)


def test_colliding_buckets(dsr, oracle, cuda, monkeypatch, capfd):
    import torch
    b = _collide_case(dsr, oracle)

    def run():
        dec = dsr.Decoder(beam=1e9, lmScale=3.0, maxActive=8192, streams=1); dec.set(b["gd"]); dec.enable_dump(True)
        out = dec.decode_batch(torch.from_numpy(b["sc"]).to(cuda))
        return out, dec.get_dump()
    (a, da), (w, dw), kind = _both(monkeypatch, capfd, run)
    assert kind == "narrow"
    _same(a, w)
    for out, d in ((a, da), (w, dw)):
        _check_decode(b["ro"], out[0]); _check_dump(b["ro"], d)
        assert out[0]["registerFrames"] == TA

    def run_plain():          # pruning on, the lists laid out for the next frame: the path a decode takes in use
        dec = dsr.Decoder(beam=1e9, lmScale=3.0, maxActive=8192, streams=1); dec.set(b["gd"])
        return dec.decode_batch(torch.from_numpy(b["sc"]).to(cuda))
    a, w, _ = _both(monkeypatch, capfd, run_plain)
    _same(a, w); _check_decode(b["plain"], a[0])
    assert a[0]["registerFrames"] == TA


def test_colliding_buckets_time_sliced(dsr, oracle, cuda, monkeypatch, capfd):
    """(e): the same decode in segments of three frames, a segment boundary between its halves: sliced = unsliced = the oracle"""
    import torch
    b = _collide_case(dsr, oracle)
    monkeypatch.setenv("DSR_VITERBI_SEG_ANY", "1")
    sc = np.concatenate([b["sc"], b["sc"]])          # (time slicing is for batches with more utterances than workgroups)

    def run(seg):
        monkeypatch.setenv("DSR_VITERBI_SEG", str(seg))
        dec = dsr.Decoder(beam=1e9, lmScale=3.0, maxActive=8192, streams=1); dec.set(b["gd"])
        return dec.decode_batch(torch.from_numpy(sc).to(cuda))
    capfd.readouterr()
    a, w, kind = _both(monkeypatch, capfd, lambda: run(3))
    assert kind == "narrow"
    monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1"); capfd.readouterr()
    run(3)
    assert "time-sliced, one queue" in capfd.readouterr().err
    u, uw, _ = _both(monkeypatch, capfd, lambda: run(0))
    _same(a, w); _same(u, uw); _same(a, u)
    for x in a:
        _check_decode(b["plain"], x)
        assert x["registerFrames"] == TA


def test_colliding_buckets_lattice(dsr, oracle, cuda, monkeypatch, capfd):
    """(f): lattice mode (the instantiation with the bookkeeping compiled in)"""
    import torch
    b = _collide_case(dsr, oracle)

    def run():
        dec = dsr.Decoder(beam=1e9, lmScale=3.0, maxActive=8192, streams=1, latticeTokens=100000); dec.set(b["gd"])
        return dec.decode_batch(torch.from_numpy(b["sc"]).to(cuda))
    a, w, kind = _both(monkeypatch, capfd, run)
    assert kind == "narrow"
    _same(a, w)
    # (the lattice mode does not prune the lists at write time: its counts are the dumping decode's)
    _check_decode(b["ro"], a[0])


def _layers(sizes, deg, stride):
    """Layered graph: layer k has sizes[k] states, every state of it deg[k] arcs into layer k + 1 (to states (stride[k] * j + 7 * i) mod its size),
    so frame k makes sizes[k] x deg[k] placements at most."""
    rng = np.random.default_rng(5)
    base = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
    arcs = []
    for k in range(len(sizes) - 1):
        n1 = sizes[k + 1]
        cs = rng.uniform(0.1, 1.5, (sizes[k], deg[k])).astype(np.float32); ins = rng.integers(1, ND + 1, (sizes[k], deg[k]))
        for j in range(sizes[k]):
            for i in range(deg[k]):
                arcs.append((int(base[k] + j), int(base[k + 1] + (stride[k] * j + 7 * i) % n1), int(ins[j, i]), 0, float(cs[j, i])))
    last = int(base[-2])
    arcs += [(last + j, last + (j + 1) % sizes[-1], 1 + j % ND, 0, 0.5) for j in range(sizes[-1])]          # the last layer goes round
    return arcs, [(last, 0.0)]


def _slots(eo, ro, f):
    """frame f + 1 (no epsilon arcs, pruning off): placements, and the largest slot at which a state is reached for the first time"""
    off = ro["dumpOff"]; slot = 0; first = {}
    for nd in ro["dumpNode"][off[f]:off[f + 1]]:
        for a in range(eo["arcOff"][nd], eo["arcOff"][nd + 1]):
            first.setdefault(int(eo["arcDst"][a]), slot); slot += 1
    return slot, max(first.values())


LAYERS = {
    # (b) frame 1: 64 x 160 = 10 240 placements, two slots a thread parked, first arrivals among them; then small frames
    "parked": dict(sizes=[1, 64, 4000, 300, 50, 10], deg=[64, 160, 2, 2, 2], stride=[1, 61, 3, 3, 3], big=10240, registerFrames=6),
    # (c) frame 1: 64 x 400 = 25 600 placements, the memory path, between register-path frames
    "memory": dict(sizes=[1, 64, 6000, 300, 50, 10], deg=[64, 400, 2, 2, 2], stride=[1, 91, 3, 3, 3], big=25600, registerFrames=5),
}
TL = 6
_layer_cache = {}


def _layer_case(dsr, oracle, name):
    if name not in _layer_cache:
        c = LAYERS[name]
        arcs, fin = _layers(c["sizes"], c["deg"], c["stride"])
        go, gd = _graphs(dsr, oracle, arcs, fin)
        sc = np.random.default_rng(23).uniform(0, 3, (1, TL, ND)).astype(np.float32)
        ro = go.decode(sc[0], beam=1e9, lmScale=2.0, dump=True)
        assert ro["rc"] == 0
        _layer_cache[name] = dict(go=go, gd=gd, sc=sc, ro=ro, plain=go.decode(sc[0], beam=1e9, lmScale=2.0), eo=go.export())
    return _layer_cache[name]


@pytest.mark.parametrize("name", list(LAYERS))
def test_large_frame_then_small_ones(dsr, oracle, cuda, monkeypatch, capfd, name):
    import torch
    b = _layer_case(dsr, oracle, name); c = LAYERS[name]
    n, lastFirst = _slots(b["eo"], b["ro"], 0)          # (the list behind frame 0 is what frame 1 expands)
    assert n == c["big"], n
    if name == "parked":
        assert lastFirst >= 8192 + 1024, lastFirst          # first arrivals in the parked slots (register path: slots from 8 192 on)
    assert all(_slots(b["eo"], b["ro"], f)[0] <= 8192 for f in (1, 2, 3, 4))

    def run(dump):
        dec = dsr.Decoder(beam=1e9, lmScale=2.0, maxActive=16384, streams=1); dec.set(b["gd"]); dec.enable_dump(dump)
        out = dec.decode_batch(torch.from_numpy(b["sc"]).to(cuda))
        return out, (dec.get_dump() if dump else None)
    (a, da), (w, dw), kind = _both(monkeypatch, capfd, lambda: run(True))
    assert kind == "narrow"
    _same(a, w)
    for out, d in ((a, da), (w, dw)):
        _check_decode(b["ro"], out[0]); _check_dump(b["ro"], d)
        assert out[0]["registerFrames"] == c["registerFrames"]
    (a, _), (w, _), _ = _both(monkeypatch, capfd, lambda: run(False))
    _same(a, w); _check_decode(b["plain"], a[0])
    assert a[0]["registerFrames"] == c["registerFrames"]


def test_failed_utterance_then_two_more(dsr, oracle, cuda, monkeypatch, capfd):
    """(d): three utterances on one workgroup, run to completion.  The first outgrows maxActive in the middle of its third frame (some 850 new tokens, 512
    allowed) and ends with DSR_E_ALLOCATION; the two behind it decode as if alone."""
    import torch
    arcs, fin = _layers([1, 30, 300, 2000, 40, 8], [30, 10, 3, 2, 2], [1, 11, 13, 3, 3])
    go, gd = _graphs(dsr, oracle, arcs, fin)
    rng = np.random.default_rng(3)
    sc = rng.uniform(0, 40, (3, TL, ND)).astype(np.float32)
    sc[0] = 1.0          # every token of the first utterance stays within the beam: 30, 268, then some 850 new tokens
    beam, lmScale = 6.0, 0.25
    ros = [go.decode(sc[u], beam=beam, lmScale=lmScale) for u in range(3)]
    assert all(r["rc"] == 0 for r in ros)
    assert int(ros[0]["activeCount"][2]) > 512 and all(int(v) <= 512 for u in (1, 2) for v in ros[u]["activeCount"])
    assert all(int(v) > 1 for u in (1, 2) for v in ros[u]["activeCount"][:4])

    def run(us):
        dec = dsr.Decoder(beam=beam, lmScale=lmScale, maxActive=512, streams=1); dec.set(gd)
        return dec.decode_batch(torch.from_numpy(np.ascontiguousarray(sc[us])).to(cuda))
    a, w, kind = _both(monkeypatch, capfd, lambda: run([0, 1, 2]))
    assert kind == "narrow"
    monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1"); capfd.readouterr()
    run([0, 1, 2])
    assert "run to completion" in capfd.readouterr().err
    _same(a, w)
    assert a[0]["status"] == 2                                   # DSR_E_ALLOCATION
    for u in (1, 2):
        _check_decode(ros[u], a[u])
        _same([a[u]], run([u]))
