"""The combination bench.py's headline figure comes from, against the oracle: fused analysis + MVDR, gmmMode=2 in its 1024 x 4-Gaussian k_gmm_sp shape,
the time-sliced k_viterbi on XCD-bound queues, two Pipe objects on two streams, collected late into reused host arrays.

The models are bench.build_models' own (the graph at 5 000 states instead of 50 000: the narrow state table either way, the same family of graph, and the
oracle decodes it in milliseconds).  The decode is sliced by DSR_VITERBI_SEG=6 alone, so the XCD-bound queues the bench gets are the ones under test; every
plan is read back from the line DSR_VITERBI_SEG_VERBOSE prints at the launch.

BEAM was chosen once by the bisection of bench.tune_beam with a target of 1 500 active tokens a frame on utterances of these lengths (the oracle's decode
of the oracle's own features: 54 gives 1 465, 56 gives 1 623) and rounded; the tests assert the floor of 1 000 on what the device reports.

Why two sliced persistent grids on two streams cannot wait on each other (k_viterbi.hip, the work loop and the hand-over below it).  A work item is
(utterance, segment); the items of a queue are handed out by one atomic counter per queue and launch, `it` -> segment it / Uq, utterance it mod Uq: every
item of segment s-1 has a smaller number than any item of segment s.  A workgroup spins on segDone[u] only after it has TAKEN item (u, s), s > 0, so item
(u, s-1) was handed out before -- to a workgroup that ran the atomicAdd, i.e. one that is resident and running.  That workgroup either works on (u, s-1),
or waits for (u, s-2) in the same way: the chain of waits strictly descends in item number and ends at a segment-0 item, which waits for nothing.  Items
that find their utterance ended (fr0 > T) or failed (status != 0 behind segDone = 0x7FFFFFFF) return without waiting.  So no workgroup ever waits for a
workgroup that is not yet resident, and none waits for anything of another launch: the counters, segState, segDone, the save area and the pool belong to
one decoder object, and a Pipe owns its decoder.  Two such grids share CUs, never a wait."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BEAM = 55.0
LM_SCALE = 12.0
SEG = 6
MAX_ACTIVE = 16384
MAX_PATH = 192                   # > 2 x 49 frames + 64, bench.py's 2 Tm + 64
NSAMP = 8000                     # samples a row of the input holds; an utterance uses its first lens[u]
ACTIVE_FLOOR = 1000.0
FIELDS = ["status", "score", "ac", "lm", "frames", "reachedFinal", "nArcs", "nWords", "maxActiveSeen", "activeHypos", "placements", "registerFrames",
          "finalStatesN"]


# ------------------------------------------------------------------------------------------- set-up shared by the tests
@pytest.fixture(scope="module")
def shipped(dsr, oracle, cuda):
    import torch
    import bench
    from tests import synth
    mdl = bench.build_models(dsr, synth, 1024, 5000)
    go = oracle.Wfst()
    for a in mdl["arcs"]:
        go.add_arc(*a)
    for s, c in mdl["fin"]:
        go.add_final(s, c)
    gm_m = mdl["gm_m"]
    slots = torch.cuda.get_device_properties(0).multi_processor_count
    assert slots >= 64 and slots % 8 == 0, slots
    return dict(mdl=mdl, go=go, cb=oracle.Codebooks(gm_m["refN"], gm_m["mean"], gm_m["ivar"], gm_m["det"]), val=gm_m["val"],
                cfg=oracle.mfcc_cfg(lda=mdl["lda"]), W=mdl["bf"].get(4), slots=slots, bench=bench)


def _frames(mf, n):
    """MFCC frames of an utterance of n samples, as the pipe counts them: whole synthesis blocks of 128 samples reach the MFCC chain"""
    return mf.frames(((int(n) + 127) // 128) * 128)


def _samples_for(mf, tm):
    """a sample count that gives exactly tm MFCC frames (not a multiple of the block: the last block is ragged)"""
    for nblk in range(1, NSAMP // 128 + 1):
        if mf.frames(nblk * 128) == tm:
            return nblk * 128 - 37
    raise AssertionError("no length with %d frames" % tm)


def _shortest(mf):
    """the shortest utterance that still has an MFCC frame"""
    n = next(n for n in range(1, NSAMP) if _frames(mf, n) >= 1)
    assert _frames(mf, n - 1) == 0 and _frames(mf, n) >= 1
    return n


def _lengths(mf, U, seed, k, lo=5000, hi=8000, longest=None, extra_at=None):
    """Ragged sample counts in [lo, hi] (30-48 frames at 5 000-8 000).  Fixed places: 0 the longest, 3 the shortest with a frame, 9/10/11 the lengths of
    6k, 6k+1 and 6k-1 frames (the end expansion -- "frame" T -- is the first item of a segment, the second, the last); extra_at: the same three again
    from that index on (among the utterances that exist only because of slicing).  -> lens, Tm, the special indices"""
    rng = np.random.default_rng(seed)
    lens = [int(v) for v in rng.integers(lo, hi + 1, U)]
    lens[0] = longest if longest is not None else hi
    lens[3] = _shortest(mf)
    special = [0, 3, 9, 10, 11]
    for base in [9] + ([extra_at] if extra_at is not None else []):
        for j, tm in enumerate((SEG * k, SEG * k + 1, SEG * k - 1)):
            lens[base + j] = _samples_for(mf, tm)
        if base != 9:
            special += [base, base + 1, base + 2]
    Tm = [_frames(mf, n) for n in lens]
    # the preconditions, from the host's frame counts
    assert Tm[9] == SEG * k and Tm[10] == SEG * k + 1 and Tm[11] == SEG * k - 1, Tm[9:12]
    assert Tm[3] >= 1 and Tm[3] == min(Tm) and Tm[0] == max(Tm), (Tm[3], Tm[0])
    assert max(lens) <= NSAMP
    return lens, Tm, special


def _make_pipe(dsr, mdl, beam=BEAM, **dkw):
    """bench.py's make(): an own Mfcc plan and an own Decoder (streams at its default: one workgroup per CU) per pipe"""
    dkw.setdefault("maxActive", MAX_ACTIVE)
    dec = dsr.Decoder(beam=beam, lmScale=LM_SCALE, **dkw); dec.set(mdl["gd"])
    return dsr.Pipe(mdl["ana"], mdl["syn"], mdl["bf"], dsr.Mfcc(lda=mdl["lda"]), mdl["gm"], dec, gmmMode=2, fused=True), dec


def _snap(res, arcs, words):
    """what a collect handed out, copied: the host arrays are the pipe's and the next collect writes them again"""
    return {f: np.array([getattr(q, f) for q in res]) for f in FIELDS}, arcs.copy(), words.copy()


def _same_results(a, b, us, what):
    ra, arcsA, wordsA = a; rb, arcsB, wordsB = b
    for u in us:
        assert [ra[f][u] for f in FIELDS] == [rb[f][u] for f in FIELDS], (what, u, [(f, ra[f][u], rb[f][u]) for f in FIELDS if ra[f][u] != rb[f][u]])
        nA, nW = int(ra["nArcs"][u]), int(ra["nWords"][u])
        assert np.array_equal(arcsA[u, :nA], arcsB[u, :nA]) and np.array_equal(wordsA[u, :nW], wordsB[u, :nW]), (what, u)


def _plan_line(err, U, slots):
    lines = [ln for ln in err.splitlines() if ln.startswith("[dsr viterbi]") and " utterances on " in ln]
    assert len(lines) == 1, err
    assert lines[0].startswith("[dsr viterbi] %d utterances on %d workgroups: " % (U, min(U, slots))), lines[0]
    assert "narrow state table" in lines[0], lines[0]
    return lines[0]


def _env(monkeypatch, seg=SEG):
    for k in ("DSR_VITERBI_SEG_ANY", "DSR_VITERBI_SEG_DROP", "DSR_VITERBI_TABLE", "DSR_VITERBI_NOFAST", "DSR_VITERBI_SLOTS", "DSR_VITERBI_SEG_SAVE_GB"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("DSR_VITERBI_SEG", str(seg))
    monkeypatch.setenv("DSR_VITERBI_SEG_VERBOSE", "1")


def _not_trivial(r, us=None):
    """the floor under the decode: every utterance decoded, ~1 000 tokens alive a frame, the register path in use"""
    us = range(len(r["status"])) if us is None else us
    assert not any(r["status"][u] for u in us), [(u, r["status"][u]) for u in us if r["status"][u]]
    act = float(np.mean([r["activeHypos"][u] / (r["frames"][u] + 1.0) for u in us]))
    assert act >= ACTIVE_FLOOR, act
    assert sum(1 for u in us if r["registerFrames"][u] > 0) > 0.9 * len(us)
    return act


# ------------------------------------------------------------------------------------------- test 1
def test_shipped_combination_against_the_oracle(dsr, oracle, cuda, shipped, monkeypatch, capfd):
    """Six batches over two pipes on two streams in bench.py's rotation (run_steps: a pipe is collected immediately before its next submit), so that each
    pipe object sees three plans and shrinking, then growing, buffers:
      0, 1  pipes 0, 1  slots + 44 utterances  time-sliced, XCD-bound queues
      2     pipe 0      40                     run to completion, one utterance per workgroup (oneEach)
      3     pipe 1      slots + 4              run to completion with more utterances than workgroups (walkHere): DSR_VITERBI_SEG=0 for this submit only
      4, 5  pipes 0, 1  slots + 44, other set  time-sliced, XCD-bound queues
    Per batch, on the rows below Tm[u]: (1) the features of six utterances (shortest and longest among them) against the chained oracle on the device's
    MVDR weights, 2e-3 absolute; (2) the mode-2 scores against oracle.gmm_score_opt of the DEVICE's features, rel 1e-5, and every padding row of the
    features exactly zero; (3) the oracle's decode of the device's own scores: status, score, nArcs, arcs and words bit for bit -- every u >= slots, the
    boundary lengths, the shortest, and eight others over all residues u mod 8; (4) every utterance against the same batch alone on a fresh pipe with
    DSR_VITERBI_SEG=0.  The checks run after the last collect, on copies, so that the two grids really are in flight together."""
    import torch
    mdl, go, slots, bench, mf = shipped["mdl"], shipped["go"], shipped["slots"], shipped["bench"], shipped["mdl"]["mf"]
    _env(monkeypatch)
    Ubig = slots + 44
    lensA, TmA, spA = _lengths(mf, Ubig, seed=301, k=6, extra_at=slots + 9)
    lensB, TmB, spB = _lengths(mf, Ubig, seed=302, k=7, hi=7900, extra_at=slots + 20)
    lens2, Tm2, sp2 = _lengths(mf, 40, seed=303, k=5, hi=7000)
    lens3, Tm3, sp3 = _lengths(mf, slots + 4, seed=304, k=6)
    assert max(lens2) < max(lensA)
    for Tm in (TmA, TmB):
        assert len(set(t // SEG for t in Tm)) >= 3, sorted(set(t // SEG for t in Tm))           # utterances end in at least three different segments
        assert 2 * SEG <= max(Tm) + 1                                                             # (what plan_decode asks before it slices)
    sliced, complete = "time-sliced, XCD-bound queues", "run to completion"
    plan = [  # pipe, lengths, frames, specials, seed of the audio, DSR_VITERBI_SEG at the submit, the plan expected
        (0, lensA, TmA, spA, 11, SEG, sliced), (1, lensA, TmA, spA, 12, SEG, sliced),
        (0, lens2, Tm2, sp2, 13, SEG, complete), (1, lens3, Tm3, sp3, 14, 0, complete),
        (0, lensB, TmB, spB, 15, SEG, sliced), (1, lensB, TmB, spB, 16, SEG, sliced)]
    xs = [bench.make_input(torch, cuda, len(p[1]), mdl["C"], NSAMP, seed=p[4]) for p in plan]
    nds = [torch.tensor(p[1], dtype=torch.int32, device=cuda) for p in plan]
    pipes = [_make_pipe(dsr, mdl)[0] for _ in range(2)]
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    torch.cuda.synchronize()
    got = [None] * len(plan); lines = [None] * len(plan); inflight = [None, None]

    def collect(i):
        k = inflight[i]; U, TmMax = len(plan[k][1]), max(plan[k][2])
        snap = _snap(*pipes[i].collect(reuse=True)); inflight[i] = None
        with torch.cuda.stream(streams[i]):                                   # the intermediates, before this pipe's next submit re-sizes and rewrites them
            feat = pipes[i].intermediate_host(3)[: U * TmMax * 39].reshape(U, TmMax, 39)
            sc = pipes[i].intermediate_host(4)[: U * TmMax * 1024].reshape(U, TmMax, 1024)
        got[k] = (snap, feat, sc)

    capfd.readouterr()
    for k, p in enumerate(plan):
        i = p[0]
        if inflight[i] is not None:
            collect(i)
        capfd.readouterr()
        monkeypatch.setenv("DSR_VITERBI_SEG", str(p[5]))                     # read at the launch
        with torch.cuda.stream(streams[i]):
            pipes[i].submit(xs[k], nds[k], p[1], maxPath=MAX_PATH, want_paths=True)
        monkeypatch.setenv("DSR_VITERBI_SEG", str(SEG))
        lines[k] = _plan_line(capfd.readouterr().err, len(p[1]), slots); inflight[i] = k
    for i in (0, 1):                                                          # drain in submission order
        collect(i)
    torch.cuda.synchronize()
    for k, p in enumerate(plan):
        assert p[6] in lines[k], (k, lines[k])
        with capfd.disabled():
            print("batch %d: %s" % (k, lines[k]))

    h, g, M, m, r, Cn = mdl["h"], mdl["g"], mdl["M"], mdl["m"], mdl["r"], mdl["C"]
    worstF = worstS = 0.0; acts = []
    for k, (i, lens, Tm, special, seed, seg, want) in enumerate(plan):
        U = len(lens); (res, arcs, words), feat, sc = got[k]
        acts.append(_not_trivial(res))
        # (2b) padding rows of the features: exactly zero, whatever a larger batch left there before
        for u in range(U):
            assert not feat[u, Tm[u]:].any(), (k, u)
        # (1) the front end of six utterances
        for u in [0, 3, 9, 10, 11, U - 1]:
            n = lens[u]; xh = xs[k][u].cpu().numpy()
            Xc = np.stack([oracle.analysis_bank(xh[c, :n], h, M, m, r, 0) for c in range(Cn)])
            fo = oracle.mfcc_chain(oracle.synthesis_bank(oracle.beamform_apply(Xc, shipped["W"]), g, M, m, r, 0), shipped["cfg"])
            assert fo.shape[0] == Tm[u], (k, u, fo.shape, Tm[u])
            e = float(np.abs(feat[u, :Tm[u]] - fo).max()); worstF = max(worstF, e)
            assert e < 2e-3, (k, u, e)
        # (2), (3) the checked set: mode 2 on the device's features, then the oracle's decode of the device's scores
        if want == sliced:
            checked = sorted(set(list(range(slots, U)) + special + [24 + 9 * j for j in range(8)]))
            assert set(u % 8 for u in checked if u < slots and u not in special) == set(range(8))
        else:
            checked = sorted(set(list(range(slots, U)) + special + list(range(16, min(U, 36)))))
            assert len(checked) >= 16
        for u in checked:
            T = Tm[u]
            ref, _ = oracle.gmm_score_opt(shipped["cb"], shipped["val"], feat[u, :T])
            e = float((np.abs(sc[u, :T] - ref) / np.maximum(np.abs(ref), 1.0)).max()); worstS = max(worstS, e)
            assert e < 1e-5, (k, u, e)
            ro = go.decode(sc[u, :T], beam=BEAM, lmScale=LM_SCALE)
            assert ro["rc"] == 0, (k, u)
            assert res["status"][u] == 0, (k, u, res["status"][u])
            assert res["score"][u] == ro["score"] and res["nArcs"][u] == len(ro["arcs"]) and res["nWords"][u] == len(ro["words"]), (k, u, T)
            assert np.array_equal(arcs[u, :len(ro["arcs"])], ro["arcs"]), (k, u, T)
            assert np.array_equal(words[u, :len(ro["words"])], ro["words"]), (k, u, T)
            assert res["frames"][u] == ro["frames"] and res["activeHypos"][u] == ro["activeHypos"], (k, u, T)
    with capfd.disabled():
        print("features: max abs error %.3g; mode 2 on pipe features: max rel score error %.3g; mean active tokens a frame, per batch: %s"
              % (worstF, worstS, " ".join("%.0f" % a for a in acts)))

    # (4) every utterance of every batch against the batch alone, unsliced, on a fresh pipe
    monkeypatch.setenv("DSR_VITERBI_SEG", "0")
    for k, p in enumerate(plan):
        capfd.readouterr()
        alone = _snap(*_make_pipe(dsr, mdl)[0].run(xs[k], nds[k], p[1], maxPath=MAX_PATH))
        assert complete in _plan_line(capfd.readouterr().err, len(p[1]), slots)
        assert not alone[0]["status"].any(), k
        _same_results(got[k][0], alone, range(len(p[1])), "batch %d" % k)


# ------------------------------------------------------------------------------------------- test 2
def test_failures_inside_a_sliced_pipe_batch_then_a_clean_one(dsr, cuda, shipped, monkeypatch, capfd):
    """One pipe on one stream, slots + 44 utterances, sliced.
    Batch A: a decoder whose maxActive is the 60th percentile of the maxActiveSeen a roomy run reported.  Some utterances end with status 2
    (DSR_E_ALLOCATION, after a few segments) and some with 0; every status-0 utterance equals its result of the roomy run field for field and path for
    path, and the DSR_VITERBI_SEG=0 run of the same pipe fails exactly the same utterances; a third run, sliced
    again on that pipe, repeats the first.
    Batch B: a clean batch on a pipe object and a decoder that have just carried failures.  A Pipe keeps the decoder it was made with and a decoder's
    maxActive is fixed when it is made, so the roomy decoder is made to fail by its beam instead: maxActive = 1.1 x the largest list the roomy run saw (roomy at
    BEAM: nothing fails), one sliced batch at a beam of 200 (nearly every state alive: the long utterances outgrow it, status 2), then setBeam(BEAM) and
    the same inputs again, collected into the same reused host arrays: bit for bit the roomy run -- the save area, segState / segDone, the pool and the
    host rows ("valid up to nArcs") after failures."""
    import torch
    mdl, slots, bench, mf = shipped["mdl"], shipped["slots"], shipped["bench"], shipped["mdl"]["mf"]
    _env(monkeypatch)
    U = slots + 44
    lens, Tm, special = _lengths(mf, U, seed=311, k=6, extra_at=slots + 9)
    assert len(set(t // SEG for t in Tm)) >= 3
    x = bench.make_input(torch, cuda, U, mdl["C"], NSAMP, seed=21); nd = torch.tensor(lens, dtype=torch.int32, device=cuda)
    stream = torch.cuda.Stream(device=cuda); torch.cuda.synchronize()

    def run(pipe, seg, want):
        monkeypatch.setenv("DSR_VITERBI_SEG", str(seg)); capfd.readouterr()
        with torch.cuda.stream(stream):
            pipe.submit(x, nd, lens, maxPath=MAX_PATH, want_paths=True)
        out = _snap(*pipe.collect(reuse=True))
        assert want in _plan_line(capfd.readouterr().err, U, slots)
        return out
    sliced, complete = "time-sliced, XCD-bound queues", "run to completion"
    roomy = run(_make_pipe(dsr, mdl)[0], SEG, sliced)
    assert not roomy[0]["status"].any()
    _not_trivial(roomy[0])
    seen = roomy[0]["maxActiveSeen"]

    # batch A
    small = max(8, int(np.percentile(seen, 60)))
    pipeS, _ = _make_pipe(dsr, mdl, maxActive=small)
    a = run(pipeS, SEG, sliced); a0 = run(pipeS, 0, complete)
    st = a[0]["status"]
    assert set(st.tolist()) == {0, 2}, sorted(set(st.tolist()))
    assert np.array_equal(st, a0[0]["status"])
    ok = [u for u in range(U) if st[u] == 0]
    with capfd.disabled():
        print("maxActive %d: %d of %d utterances fail" % (small, U - len(ok), U))
    _same_results(a, roomy, ok, "maxActive %d, sliced" % small)
    _same_results(a0, roomy, ok, "maxActive %d, run to completion" % small)
    a2 = run(pipeS, SEG, sliced)                                              # and sliced once more, behind two batches that left failed utterances in every buffer
    assert np.array_equal(a2[0]["status"], st)
    _same_results(a2, roomy, ok, "maxActive %d, sliced again" % small)

    # batch B
    cap = int(1.1 * seen.max())
    pipeR, decR = _make_pipe(dsr, mdl, maxActive=cap, maxCandidates=8 * MAX_ACTIVE)
    decR.setBeam(200.0)
    f = run(pipeR, SEG, sliced)
    assert 2 in f[0]["status"] and set(f[0]["status"].tolist()) <= {0, 2}, sorted(set(f[0]["status"].tolist()))
    with capfd.disabled():
        print("maxActive %d at a beam of 200: %d of %d utterances fail" % (cap, int((f[0]["status"] == 2).sum()), U))
    decR.setBeam(BEAM)
    b = run(pipeR, SEG, sliced)
    _same_results(b, roomy, range(U), "after a batch with failures")
