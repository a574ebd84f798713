"""The epsilon hops behind the first in the register path's expansion: hops 2 to 4 in straight line for every lane (dropped by select where the path is
shorter), their costs loaded once per pair of placements, the hop loop only for a wave that holds a path of more than four hops, paths above 14 hops
walked through the arc arrays.

State 0 is the start state F, so frame 0 expands F's expansion list alone, from slot 0: the order of its records is the depth-first order of the
graph's arcs, which the cases below shape (a 64-slot group = one wave's placements, slots t and t + 1024 = the two placements of a thread's first
pair, slots from 8 192 on = parked).  Every emitting arc ends in a small pool of states D that lead back to F and to each other, so later frames
expand F again, behind and between other tokens.

Every decode is compared with the oracle bit for bit (per-frame lists where the mode dumps them), and runs with both tables, which must agree."""
import numpy as np
import pytest

from tests.test_gpu_viterbi_table import _both, _check_decode, _check_dump, _graphs, _same

pytestmark = pytest.mark.gpu

SIL = 8          # input symbol of the silence model (distribution 7)
ND = 8
BEAM = 1e35      # nothing is pruned: the slots of a frame are the dumped list's expansion records in order
PEN = (0.37, -1.9)
E_COST = [0.1, 0.0, 0.7, 1.3, 0.25, 2.5]
H_COST = [0.0, 0.1, 0.45, 1.7]


class _Graph:
    """F = state 0, the pool D = states 1 .. nD, chain states from nD + 1 on"""

    def __init__(self, nD, hcost=H_COST):
        self.nD = nD; self.arcs = []; self.fresh = nD + 1; self.ne = 0; self.nh = 0; self.hcost = hcost

    def emit(self, src, sil=False, dst=None):
        """(the k-th emitting arc ends in D number 7 k mod nD: nD is a prime above the length of F's list where every placement of frame 0 is to show in the lists)"""
        k = self.ne; self.ne += 1
        self.arcs.append((src, 1 + (k * 7) % self.nD if dst is None else dst, SIL if sil else 1 + k % 7, 2 + k % 5 if k % 3 == 0 else 0, E_COST[k % len(E_COST)]))

    def hop(self, src, out=0, cost=None):
        k = self.nh; self.nh += 1
        dst = self.fresh; self.fresh += 1
        self.arcs.append((src, dst, 0, out, self.hcost[k % len(self.hcost)] if cost is None else cost))
        return dst

    def spine(self, depths, outs=(), sil=(), costs=None):
        """a chain of max(depths) epsilon hops from F; a state at a depth in `depths` has an emitting arc ahead of its hop and one behind it, so the
        depth-first order of F's records goes down the chain and up again: depths in rising, then in falling order.  outs: hops (1-based) with an output
        symbol; sil: depths whose emitting arcs are silence arcs; costs: hop (1-based) -> cost."""
        chain = [0]; behind = []
        for d in range(max(depths) + 1):
            if d in depths:
                self.emit(chain[d], sil=d in sil)
            if d < max(depths):
                chain.append(self.hop(chain[d], out=20 + d if d + 1 in outs else 0, cost=(costs or {}).get(d + 1)))
            behind.append(chain[d])
        for d in range(max(depths), -1, -1):          # (behind the state's hop)
            if d in depths:
                self.emit(behind[d], sil=d in sil)

    def block(self, h, n, outs=(), dst=None):
        """n emitting arcs behind one shared chain of h hops from F: n consecutive records of h hops"""
        s = 0
        for k in range(h):
            s = self.hop(s, out=20 + k if k + 1 in outs else 0)
        for i in range(n):
            self.emit(s, dst=None if dst is None else dst(i))

    def done(self):
        """the pool: every D leads back to F and to the next D.  (A state's newest arc is its first one: the arcs go in in reverse, so that
        every state's arcs -- and with them F's records -- come in the order they were made above.)"""
        a = self.arcs[::-1]
        assert a[0][0] == 0                                       # the first state named is the start state
        for j in range(1, self.nD + 1):
            a.append((j, 0, 1 + j % 7, 0, E_COST[j % len(E_COST)]))
            a.append((j, 1 + j % self.nD, 1 + (j + 3) % 7, 3 if j % 4 == 0 else 0, E_COST[(j + 2) % len(E_COST)]))
        return a, [(0, 0.0), (3, 0.5)]


ALL9 = (0, 1, 2, 3, 4, 5, 6, 14, 15)


def _g_every():
    g = _Graph(601)
    for s in range(32):
        g.spine(ALL9, outs=(1 + s % 15,), sil=(s % 16,))
    return g.done()


def _g_edge(m):
    g = _Graph(601)
    for s in range(16):
        g.spine(tuple(range(m + 1)), outs=(1 + s % (m + 1),))
    return g.done()


def _g_pair(a, b):
    g = _Graph(2053)
    g.block(a, 1024, outs=(2, 4)); g.block(b, 1024, outs=(3, 5, 15)); g.block(0, 1)
    return g.done()


def _g_parked():
    g = _Graph(2003)
    g.block(0, 8192, dst=lambda i: 301 + (7 * i) % 1703)          # (the parked placements have D 1 .. 300 to themselves)
    s = 0
    for d in range(1, 6):
        s = g.hop(s, out=7 if d == 4 else 0)
        if d >= 3:
            for i in range(100):
                g.emit(s, dst=1 + 100 * (d - 3) + i)
    g.emit(0, dst=301)
    return g.done()


def _g_pen():
    """outputs on hop 2, 3, 4 and 5, each alone, all together, and none; the emitting arcs at one depth of every chain are silence arcs (depth > 0: a silence arc behind an epsilon path)"""
    g = _Graph(601)
    for r in range(3):
        for k, outs in enumerate([(2,), (3,), (4,), (5,), (2, 3, 4, 5), ()]):
            g.spine(tuple(range(7)), outs=outs, sil=((k + r) % 7,))
    return g.done()


def _g_cost(tiny):
    """0.0f, 0.1f, 3e30f and 1e-30f (tiny; 0.7f otherwise) on each of the hops 2 to 5"""
    cs = [0.0, 0.1, 3e30, 1e-30 if tiny else 0.7]
    g = _Graph(601)
    for r in range(4):
        for rot in range(4):
            g.spine(tuple(range(7)), outs=(2 + (r + rot) % 4,), sil=(6,) if rot == r else (), costs={h: cs[(h + rot) % 4] for h in (2, 3, 4, 5)})
    return g.done()


CASES = {
    "every": (_g_every, 6), "edge2": (lambda: _g_edge(2), 6), "edge3": (lambda: _g_edge(3), 6), "edge4": (lambda: _g_edge(4), 6), "edge5": (lambda: _g_edge(5), 6),
    "pair0_4": (lambda: _g_pair(0, 4), 4), "pair3_5": (lambda: _g_pair(3, 5), 4), "pair5_15": (lambda: _g_pair(5, 15), 4), "parked": (_g_parked, 3),
    "pen": (_g_pen, 6), "cost": (lambda: _g_cost(False), 6), "cost_tiny": (lambda: _g_cost(True), 6),
}
_cache = {}


def _case(dsr, oracle, name):
    """graph pair, scores (two utterances; the second one is for the sliced decode), the oracle's decodes as the tests ask for them, once per case"""
    if name not in _cache:
        make, T = CASES[name]
        arcs, fin = make()
        go, gd = _graphs(dsr, oracle, arcs, fin)
        sc = np.random.default_rng(sorted(CASES).index(name) + 50).uniform(0, 3, (2, T, ND)).astype(np.float32)
        _cache[name] = dict(go=go, gd=gd, sc=sc, T=T, ref={}, eo=None, xp={})
    return _cache[name]


def _ref(b, lmScale=12.0, pen=(0.0, 0.0), dump=True, u=0):
    k = (lmScale, pen, dump, u)
    if k not in b["ref"]:
        ro = b["go"].decode(b["sc"][u], beam=BEAM, lmScale=lmScale, lmPenalty=pen[0], silPenalty=pen[1], silenceX=SIL, dump=dump)
        assert ro["rc"] == 0
        b["ref"][k] = ro
    return b["ref"][k]


def _records(b, nd):
    """the expansion records of node nd in order (WfstGraph::tables: depth first, arcs in order) -> [(hops of the path, the path's arcs, the emitting arc)]"""
    if b["eo"] is None:
        b["eo"] = b["go"].export()
    eo = b["eo"]
    if nd not in b["xp"]:
        out = []

        def walk(n, path):
            for a in range(eo["arcOff"][n], eo["arcOff"][n + 1]):
                if eo["arcIn"][a] == 0:
                    walk(int(eo["arcDst"][a]), path + (a,))
                else:
                    out.append((len(path), path, a))
        walk(nd, ())
        b["xp"][nd] = out
    return b["xp"][nd]


def _slots(b, ro, f):
    """the placements of frame f in slot order: frame 0 expands the start node, frame f > 0 the list dumped behind frame f - 1"""
    if f == 0:
        _records(b, 0)
        start = int(np.where(b["eo"]["nodeState"] == 0)[0][0])
        return list(_records(b, start))
    off = ro["dumpOff"]; out = []
    for nd in ro["dumpNode"][off[f - 1]:off[f]]:
        out += _records(b, int(nd))
    return out


def _hops(b, ro, f):
    return np.array([r[0] for r in _slots(b, ro, f)])


def _groups(h):
    return [h[i:i + 64] for i in range(0, len(h) - 63, 64)]          # the full 64-slot groups


# ------------------------------------------------------------------ the cases are what they are meant to be (oracle only)
def test_cases_are_what_they_are_meant_to_be(dsr, oracle):
    b = _case(dsr, oracle, "every"); ro = _ref(b)
    h0 = _hops(b, ro, 0)
    assert len(h0) == 32 * 18 and sum(1 for i in range(len(h0)) if h0[i] == 0 and (i == 0 or h0[i - 1] != 0)) >= 32          # 64 runs through the nine classes
    assert all(set(ALL9) <= set(g) for g in _groups(h0)), [sorted(set(g)) for g in _groups(h0)]       # every class in every wave of frame 0
    for f in (2, 3, 4, 5):                                                                                 # and again behind other tokens, at other lanes
        assert any(set(ALL9) <= set(g) for g in _groups(_hops(b, ro, f)))
    # (the sliced decode: the first frames of its resumed segments)
    for u in (0, 1):
        rp = _ref(b, u=u)
        assert max(_hops(b, rp, 3)) == 15 and sum(_hops(b, rp, 3) > 1) > 64
    for m in (2, 3, 4, 5):
        b = _case(dsr, oracle, "edge%d" % m); ro = _ref(b)
        gs = _groups(_hops(b, ro, 0))
        assert len(gs) >= 1 and all(max(g) == m for g in gs)
        for f in range(b["T"]):
            hf = _hops(b, ro, f)
            assert max(hf) <= m
            assert f in (0, 1) or any(max(g) == m for g in _groups(hf))
    for a, c in ((0, 4), (3, 5), (5, 15)):
        b = _case(dsr, oracle, "pair%d_%d" % (a, c)); ro = _ref(b)
        h0 = _hops(b, ro, 0)
        assert len(h0) == 2049 and all(h0[:1024] == a) and all(h0[1024:2048] == c) and h0[2048] == 0
        assert len(_hops(b, ro, 2)) >= 2049
    b = _case(dsr, oracle, "parked"); ro = _ref(b)
    h0 = _hops(b, ro, 0)
    assert len(h0) == 8493 and all(h0[:8192] == 0) and [int(sum(h0[8192:] == k)) for k in (3, 4, 5)] == [100, 100, 100]
    assert 0 < len(_hops(b, ro, 1)) <= 8192
    b = _case(dsr, oracle, "pen"); ro = _ref(b, pen=PEN)
    eo = b["eo"] if b["eo"] is not None else b["go"].export()
    s0 = _slots(b, ro, 0)
    pats = set()
    for n, path, a in s0:
        pats.add((n, tuple(k + 1 for k, e in enumerate(path) if eo["arcOut"][e] != 0)))
    for k in (2, 3, 4, 5):
        assert (6, (k,)) in pats and (k, (k,)) in pats           # an output on hop k alone, on the last hop of a path and inside a longer one
    assert (6, (2, 3, 4, 5)) in pats and (6, ()) in pats
    assert set(n for n, path, a in s0 if eo["arcIn"][a] == SIL) >= {1, 2, 3, 4, 5, 6}          # silence arcs behind paths of every length
    assert _ref(b, pen=PEN)["lm"] != _ref(b)["lm"]
    for tiny in (False, True):
        b = _case(dsr, oracle, "cost_tiny" if tiny else "cost"); ro = _ref(b)
        eo = b["go"].export()
        want = set(np.array([0.0, 0.1, 3e30, 1e-30 if tiny else 0.7], np.float32).view(np.uint32).tolist())
        for k in (2, 3, 4, 5):
            got = set()
            for n, path, a in _slots(b, ro, 0):
                if n == 6:
                    got.add(int(np.float32(eo["arcCost"][path[k - 1]]).view(np.uint32)))
            assert got == want, (k, got)
        assert float(np.max(ro["dumpLm"])) > 1e31          # 3e30f made it into the lists (1e-30f behind a first hop is absorbed: it is there for the arithmetic and the instantiation)


# ------------------------------------------------------------------ decodes
def _decode_both(dsr, cuda, monkeypatch, capfd, b, lmScale=12.0, pen=(0.0, 0.0), maxActive=8192):
    """dumping (every list against the oracle's) and plain (pruning on, lists laid out for the next frame), each with both tables"""
    import torch
    sc = torch.from_numpy(b["sc"][:1]).to(cuda)

    def run(dump):
        dec = dsr.Decoder(beam=BEAM, lmScale=lmScale, lmPenalty=pen[0], silPenalty=pen[1], silenceX=SIL, maxActive=maxActive, streams=1); dec.set(b["gd"]); dec.enable_dump(dump)
        out = dec.decode_batch(sc)
        return out, (dec.get_dump() if dump else None)
    ro = _ref(b, lmScale, pen)
    (a, da), (w, dw), kind = _both(monkeypatch, capfd, lambda: run(True))
    assert kind == "narrow"
    _same(a, w)
    for out, d in ((a, da), (w, dw)):
        _check_decode(ro, out[0]); _check_dump(ro, d)
        assert out[0]["registerFrames"] == b["T"]
    (a, _), (w, _), _ = _both(monkeypatch, capfd, lambda: run(False))
    _same(a, w); _check_decode(_ref(b, lmScale, pen, dump=False), a[0])
    assert a[0]["registerFrames"] == b["T"]


@pytest.mark.parametrize("pen", [False, True], ids=["nopen", "pen"])
def test_every_class_in_one_wave(dsr, oracle, cuda, monkeypatch, capfd, pen):
    _decode_both(dsr, cuda, monkeypatch, capfd, _case(dsr, oracle, "every"), pen=PEN if pen else (0.0, 0.0))


@pytest.mark.parametrize("m", [2, 3, 4, 5])
def test_largest_path_of_a_wave(dsr, oracle, cuda, monkeypatch, capfd, m):
    """4: the last length in straight line; 5: the first one that takes the loop"""
    b = _case(dsr, oracle, "edge%d" % m)
    _decode_both(dsr, cuda, monkeypatch, capfd, b)
    _decode_both(dsr, cuda, monkeypatch, capfd, b, pen=PEN)


@pytest.mark.parametrize("name", ["pair0_4", "pair3_5", "pair5_15"])
def test_two_placements_of_a_pair(dsr, oracle, cuda, monkeypatch, capfd, name):
    b = _case(dsr, oracle, name)
    _decode_both(dsr, cuda, monkeypatch, capfd, b)
    _decode_both(dsr, cuda, monkeypatch, capfd, b, pen=PEN)


def test_parked_placements(dsr, oracle, cuda, monkeypatch, capfd):
    b = _case(dsr, oracle, "parked")
    _decode_both(dsr, cuda, monkeypatch, capfd, b, maxActive=16384)
    _decode_both(dsr, cuda, monkeypatch, capfd, b, pen=PEN, maxActive=16384)


def test_outputs_on_hops(dsr, oracle, cuda, monkeypatch, capfd):
    """the same graph with both penalties (the penalty instantiation) and with neither (the penalty-free one)"""
    b = _case(dsr, oracle, "pen")
    _decode_both(dsr, cuda, monkeypatch, capfd, b, pen=PEN)
    _decode_both(dsr, cuda, monkeypatch, capfd, b)


@pytest.mark.parametrize("pen", [False, True], ids=["nopen", "pen"])
@pytest.mark.parametrize("tiny", [False, True], ids=["plain", "tiny"])
@pytest.mark.parametrize("lmScale", [12.0, 9.3, 1e-3])
def test_hop_costs_and_scales(dsr, oracle, cuda, monkeypatch, capfd, lmScale, tiny, pen):
    """tiny: a product below 2^-60, which turns the penalty-free instantiation off whatever the penalties"""
    if tiny:
        assert lmScale * float(np.float32(1e-30)) < 2.0 ** -60
    _decode_both(dsr, cuda, monkeypatch, capfd, _case(dsr, oracle, "cost_tiny" if tiny else "cost"), lmScale=lmScale, pen=PEN if pen else (0.0, 0.0))


def test_two_decoders_one_graph(dsr, oracle, cuda):
    """two decoders of different lmScale made from one Wfst, used in turn"""
    import torch
    b = _case(dsr, oracle, "cost")
    decs = []
    for lmScale in (12.0, 9.3):
        dec = dsr.Decoder(beam=BEAM, lmScale=lmScale, silenceX=SIL, maxActive=8192, streams=1); dec.set(b["gd"]); dec.enable_dump(True)
        decs.append((lmScale, dec))
    for lmScale, dec in decs + decs:
        ro = _ref(b, lmScale)
        out = dec.decode_batch(torch.from_numpy(b["sc"][:1]).to(cuda))
        _check_decode(ro, out[0]); _check_dump(ro, dec.get_dump())
        assert out[0]["registerFrames"] == b["T"]


def test_time_sliced(dsr, oracle, cuda, monkeypatch, capfd):
    """segments of three frames: frames 3 of both utterances are the first frames of resumed segments (the general layout path) and hold paths of every length"""
    import torch
    b = _case(dsr, oracle, "every")
    monkeypatch.setenv("DSR_VITERBI_SEG_ANY", "1")

    def run(seg):
        monkeypatch.setenv("DSR_VITERBI_SEG", str(seg))
        dec = dsr.Decoder(beam=BEAM, lmScale=12.0, lmPenalty=PEN[0], silPenalty=PEN[1], silenceX=SIL, maxActive=8192, streams=1); dec.set(b["gd"])
        return dec.decode_batch(torch.from_numpy(b["sc"]).to(cuda))
    capfd.readouterr()
    a, w, kind = _both(monkeypatch, capfd, lambda: run(3))
    assert kind == "narrow"
    monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1"); capfd.readouterr()
    run(3)
    assert "time-sliced, one queue" in capfd.readouterr().err
    u, uw, _ = _both(monkeypatch, capfd, lambda: run(0))
    _same(a, w); _same(u, uw); _same(a, u)
    for i, x in enumerate(a):
        _check_decode(_ref(b, pen=PEN, dump=False, u=i), x)
        assert x["registerFrames"] == b["T"]
