"""asr/decoder, asr/lattice: the decoding graph, the decoder, its lattices and the decode pipe."""
import ctypes as C

import numpy as np

from . import _core
from ._core import (DsrError, Handle, DecoderCfg, DecodeResult, check, cur_stream, load, vp, i32, i64, f32, _np, _ptr, _dev, _counts)


class Wfst(Handle):
    """WFSTFlyWeight (asr/decoder/wfstFlyWeight.h:47-119)."""

    _destroy = "dsr_wfst_destroy"

    def __init__(self):
        L = load(); self._create(L.dsr_wfst_create)

    def read(self, fileName, binary=False):
        check(_core._lib.dsr_wfst_read(self.h, fileName.encode(), int(binary)))

    def read_dynamic(self, fileName, noSelfLoops=False):
        """WFSTransducer::read (asr/fsm/fsm.cc:901-986)"""
        check(_core._lib.dsr_wfst_read_dynamic(self.h, fileName.encode(), int(noSelfLoops)))

    def write(self, fileName, binary=True):
        check(_core._lib.dsr_wfst_write(self.h, fileName.encode(), int(binary)))

    def add_arc(self, s1, s2, i, o, cost=0.0):
        check(_core._lib.dsr_wfst_add_arc(self.h, s1, s2, i, o, cost))

    def add_final(self, s, cost=0.0):
        check(_core._lib.dsr_wfst_add_final(self.h, s, cost))

    def export(self):
        n = _core._lib.dsr_wfst_num_nodes(self.h); a = _core._lib.dsr_wfst_num_arcs(self.h)
        d = dict(nodeState=np.zeros(n, np.uint32), nodeFinal=np.zeros(n, np.int32), nodeCost=np.zeros(n, np.float32),
                 arcOff=np.zeros(n + 1, np.int32), arcDst=np.zeros(max(a, 1), np.int32), arcIn=np.zeros(max(a, 1), np.uint32),
                 arcOut=np.zeros(max(a, 1), np.uint32), arcCost=np.zeros(max(a, 1), np.float32))
        check(_core._lib.dsr_wfst_export(self.h, *[_ptr(d[k]) for k in ("nodeState", "nodeFinal", "nodeCost", "arcOff", "arcDst", "arcIn", "arcOut", "arcCost")]))
        for k in ("arcDst", "arcIn", "arcOut", "arcCost"):
            d[k] = d[k][:a]
        return d


class Decoder(Handle):
    """DecoderFlyWeight (asr/decoder/decoder.i:147-199) for batches of score matrices."""

    _destroy = "dsr_decoder_destroy"

    def __init__(self, beam=100.0, lmScale=12.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0xFFFFFFFF, maxActive=0,
                 maxCandidates=0, arenaTokens=0, streams=0, latticeTokens=0, topN=0, wordTrace=0, generateLattice=True, propagateN=5, fastHash=False,
                 insertSilence=False, wordTraces=0):
        L = load(); c = DecoderCfg(); L.dsr_decoder_default_cfg(C.byref(c))
        c.wordTrace, c.wordTraceLattice, c.propagateN, c.fastHash, c.insertSilence, c.wordTraces = int(wordTrace), int(generateLattice), propagateN, int(fastHash), int(insertSilence), wordTraces
        c.beam, c.lmScale, c.lmPenalty, c.silPenalty, c.silenceX = beam, lmScale, lmPenalty, silPenalty, silenceX
        c.maxActive, c.maxCandidates, c.arenaTokens, c.streams, c.latticeTokens, c.topN = maxActive, maxCandidates, arenaTokens, streams, latticeTokens, topN
        self._create(L.dsr_decoder_create, C.byref(c)); self._g = None

    def set(self, wfst):
        check(_core._lib.dsr_decoder_set(self.h, wfst.h)); self._g = wfst

    def setBeam(self, beam):
        check(_core._lib.dsr_decoder_set_beam(self.h, beam))

    def enable_dump(self, on=True):
        check(_core._lib.dsr_decoder_enable_dump(self.h, int(on)))

    def decode_batch(self, scores, nframes=None, maxPath=None):
        """scores: cuda float32 [U][T][nDist].  Returns list of dicts."""
        U, T, nDist = scores.shape
        nframes = _counts(nframes, U, T, scores.device)
        if maxPath is None:
            maxPath = 4 * T + 64
        res = (DecodeResult * U)()
        arcs = np.zeros((U, maxPath), np.int32); words = np.zeros((U, maxPath), np.uint32)
        check(_core._lib.dsr_decoder_decode_batch(self.h, _dev(scores), _dev(nframes), U, T, nDist, C.byref(res), _ptr(arcs), _ptr(words), maxPath, cur_stream()))
        out = []
        for u in range(U):
            r = res[u]
            out.append(dict(status=r.status, score=r.score, ac=r.ac, lm=r.lm, frames=r.frames, reachedFinal=bool(r.reachedFinal),
                            arcs=arcs[u, :min(r.nArcs, maxPath)].copy(), words=words[u, :min(r.nWords, maxPath)].copy(),
                            activeHypos=r.activeHypos, maxActive=r.maxActiveSeen, placements=r.placements, registerFrames=r.registerFrames, laidOutFrames=r.laidOutFrames_, finalStatesN=r.finalStatesN))
        return out

    def lattice(self, u=0, eosX=0):
        """_Decoder::lattice() (decoder.h:805-860) of utterance u of the last decode (needs latticeTokens > 0)"""
        h = vp(); check(_core._lib.dsr_decoder_lattice(self.h, int(u), int(eosX), C.byref(h)))
        return Lattice(h)

    def writeGMM(self, u, conv, channel, spk, utt, cfrom, score, fileName="", frameInterval=0.01):
        """_Decoder::writeGMM (decoder.h:1018-1102) of utterance u of the last decode (needs latticeTokens > 0 and set_symbols)"""
        check(_core._lib.dsr_decoder_write_gmm(self.h, int(u), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                         (fileName or "").encode(), float(frameInterval)))

    def get_dump(self):
        n = i64(); fo = C.POINTER(i64)(); nd = C.POINTER(i32)(); ac = C.POINTER(f32)(); lm = C.POINTER(f32)(); arc = C.POINTER(i32)()
        check(_core._lib.dsr_decoder_get_dump(self.h, C.byref(n), C.byref(fo), C.byref(nd), C.byref(ac), C.byref(lm), C.byref(arc)))
        nf = n.value
        off = np.array([fo[i] for i in range(nf + 1)], np.int64) if nf > 0 else np.zeros(1, np.int64)
        N = int(off[-1])
        g = lambda p, dt: np.ctypeslib.as_array(p, (N,)).astype(dt).copy() if N > 0 else np.zeros(0, dt)
        return dict(frameOff=off, node=g(nd, np.int32), ac=g(ac, np.float32), lm=g(lm, np.float32), arc=g(arc, np.int32))


def _lexh(lex):
    """handle of a lexicon object (asr.dictionary.LexiconPtr keeps it in _h) or None"""
    if lex is None:
        return None
    return getattr(lex, "_h", None) or getattr(lex, "h", None)


class Lattice(Handle):
    """asr/lattice Lattice as the decoder builds it: nodes numbered as the reference numbers them (0 = initial), edges in creation order."""

    _destroy = "dsr_lattice_destroy"

    def __init__(self, handle):
        self.h = handle
        n, e = _core._lib.dsr_lattice_num_nodes(self.h), _core._lib.dsr_lattice_num_edges(self.h)
        d = {"nodeFinal": np.zeros(n, np.int32), "from": np.zeros(e, np.int32), "to": np.zeros(e, np.int32), "in": np.zeros(e, np.uint32),
             "out": np.zeros(e, np.uint32), "start": np.zeros(e, np.int32), "end": np.zeros(e, np.int32), "ac": np.zeros(e, np.float64), "lm": np.zeros(e, np.float64)}
        check(_core._lib.dsr_lattice_get(self.h, *[_ptr(d[k]) for k in ("nodeFinal", "from", "to", "in", "out", "start", "end", "ac", "lm")]))
        self.data = d; self.finalStatesN = _core._lib.dsr_lattice_final_states_n(self.h)

    def write(self, fileName, useSymbols=False, writeData=False):
        """Lattice::write (lattice.cc:715-757); useSymbols needs the lexica and is not offered here"""
        if useSymbols:
            raise DsrError(13, "useSymbols: write the numeric form and map the symbols with the lexica")
        check(_core._lib.dsr_lattice_write(self.h, fileName.encode(), int(writeData)))

    # ---- asr/lattice operations (lattice.i:79-123); symbols cross the boundary as indices, asr/lattice.py joins them with the lexica
    @staticmethod
    def read(fileName, noSelfLoops=False, readData=False, inlex=None, outlex=None):
        """WFST::read(fileName, noSelfLoops, readData) (fsm.h:3787-3873); inlex/outlex: Lexicon objects (or None) for symbolic files"""
        load(); h = vp()
        check(_core._lib.dsr_lattice_read(fileName.encode(), int(noSelfLoops), int(readData), _lexh(inlex), _lexh(outlex), C.byref(h)))
        return Lattice(h)

    def rescore(self, lmScale=30.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0):
        sc = C.c_float(0.0)
        check(_core._lib.dsr_lattice_rescore(self.h, float(lmScale), float(lmPenalty), float(silPenalty), int(silenceX), C.byref(sc)))
        return np.float32(sc.value)

    def bestHypo(self, useInputSymbols=False):
        n = C.c_int(0); check(_core._lib.dsr_lattice_best_hypo(self.h, int(useInputSymbols), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), np.uint32)
        check(_core._lib.dsr_lattice_best_hypo(self.h, int(useInputSymbols), _ptr(out), out.size, C.byref(n)))
        return out[:n.value].copy()

    def gammaProbs(self, acScale=1.0, lmScale=12.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0):
        p = C.c_double(0.0)
        check(_core._lib.dsr_lattice_gamma_probs(self.h, float(acScale), float(lmScale), float(lmPenalty), float(silPenalty), int(silenceX), C.byref(p)))
        return p.value

    def gammaProbsDist(self, distribset, acScale=1.0, lmScale=12.0, lmPenalty=0.0, silPenalty=0.0, silenceX=0):
        """Lattice::gammaProbsDist (lattice.cc:331-341): distribset = a dsr_distribset handle (asr.gaussian.DistribSetBasicPtr keeps it in _ds)"""
        p = C.c_double(0.0)
        check(_core._lib.dsr_lattice_gamma_probs_dist(self.h, distribset, float(acScale), float(lmScale), float(lmPenalty), float(silPenalty), int(silenceX), C.byref(p)))
        return p.value

    def prune(self, threshold=100.0):
        check(_core._lib.dsr_lattice_prune(self.h, float(threshold)))

    def pruneEdges(self, edgesN=0):
        check(_core._lib.dsr_lattice_prune_edges(self.h, int(edgesN)))

    def purge(self):
        check(_core._lib.dsr_lattice_purge(self.h))

    def state(self):
        """per link (creation order): gamma, still on its node's list; per node (creation order): printed index, still held, forward, backward"""
        n, e = _core._lib.dsr_lattice_num_nodes(self.h), _core._lib.dsr_lattice_num_edges(self.h)
        d = dict(gamma=np.zeros(e, np.float64), edgeLive=np.zeros(e, np.int32), nodeIndex=np.zeros(n, np.int32), nodeLive=np.zeros(n, np.int32),
                 fwd=np.zeros(n, np.float64), bwd=np.zeros(n, np.float64))
        check(_core._lib.dsr_lattice_get_state(self.h, *[_ptr(d[k]) for k in ("gamma", "edgeLive", "nodeIndex", "nodeLive", "fwd", "bwd")]))
        return d

    def writeCTM(self, outlex, conv, channel, spk, utt, cfrom, score, fileName="", frameInterval=0.01, endMarker="</s>"):
        check(_core._lib.dsr_lattice_write_ctm(self.h, _lexh(outlex), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                         fileName.encode(), float(frameInterval), endMarker.encode()))

    def writePhoneCTM(self, inlex, conv, channel, spk, utt, cfrom, score, fileName="", frameInterval=0.01, endMarker="</s>"):
        check(_core._lib.dsr_lattice_write_phone_ctm(self.h, _lexh(inlex), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                               fileName.encode(), float(frameInterval), endMarker.encode()))

    def writeHypoHTK(self, outlex, conv, channel, spk, utt, cfrom, score, fileName="", flag=0, frameInterval=0.01, endMarker="</s>"):
        check(_core._lib.dsr_lattice_write_hypo_htk(self.h, _lexh(outlex), conv.encode(), channel.encode(), spk.encode(), utt.encode(), float(cfrom), float(score),
                                              fileName.encode(), int(flag), float(frameInterval), endMarker.encode()))

    def writeWordConfs(self, outlex, fileName, uttId, endMarker="</s>"):
        check(_core._lib.dsr_lattice_write_word_confs(self.h, _lexh(outlex), fileName.encode(), uttId.encode(), endMarker.encode()))

    def pack(self):
        n = _core._lib.dsr_lattice_pack_size(self.h); b = np.zeros(n, np.uint8)
        check(_core._lib.dsr_lattice_pack(self.h, _ptr(b), n)); return b

    @staticmethod
    def unpack(buf):
        load(); b = np.ascontiguousarray(buf, np.uint8); h = vp()
        check(_core._lib.dsr_lattice_unpack(_ptr(b), b.size, C.byref(h))); return Lattice(h)


class Pipe(Handle):
    _destroy = "dsr_pipe_destroy"

    def __init__(self, ana, syn, bf, mfcc, gmm, dec, gmmMode=0, fused=False):
        """fused: analysis bank and fixed-weight beamformer as one kernel where supported (the channel snapshots are then never written)"""
        L = load(); self._keep = (ana, syn, bf, mfcc, gmm, dec)
        self._create(L.dsr_pipe_create, ana.h, syn.h, bf.h, mfcc.h, gmm.h, dec.h, gmmMode)
        if fused:
            check(L.dsr_pipe_set_fused(self.h, 1))

    def run(self, x, nsamp_dev, nsamp_host, maxPath=4096, want_paths=True):
        U, Cn, N = x.shape
        res = (DecodeResult * U)()
        ns = _np(nsamp_host, np.int32)
        arcs = np.zeros((U, maxPath), np.int32) if want_paths else None
        words = np.zeros((U, maxPath), np.uint32) if want_paths else None
        check(_core._lib.dsr_pipe_run(self.h, _dev(x), _dev(nsamp_dev), _ptr(ns), U, Cn, N, C.byref(res),
                                _ptr(arcs) if want_paths else None, _ptr(words) if want_paths else None, maxPath, cur_stream()))
        return res, arcs, words

    def submit(self, x, nsamp_dev, nsamp_host, maxPath=4096, want_paths=True):
        """Enqueue one batch on the current stream and return; collect() waits for it.  One batch in flight per Pipe."""
        U, Cn, N = x.shape
        ns = _np(nsamp_host, np.int32)
        self._inflight = (U, maxPath, want_paths, x, nsamp_dev, ns)              # keep the inputs alive until collected
        check(_core._lib.dsr_pipe_submit(self.h, _dev(x), _dev(nsamp_dev), _ptr(ns), U, Cn, N, maxPath, 1 if want_paths else 0, cur_stream()))

    def collect(self, reuse=False):
        """reuse: hand out the same host arrays call after call (rows are valid up to nArcs / nWords, the rest is whatever the call before left):
        a fresh zero-filled pair is 16 MB of page faults per 1000-utterance batch"""
        U, maxPath, want_paths = self._inflight[:3]
        res = (DecodeResult * U)()
        if reuse and want_paths:
            h = getattr(self, "_host", None)
            if h is None or h[0].shape != (U, maxPath):
                h = self._host = (np.zeros((U, maxPath), np.int32), np.zeros((U, maxPath), np.uint32))
            arcs, words = h
        else:
            arcs = np.zeros((U, maxPath), np.int32) if want_paths else None
            words = np.zeros((U, maxPath), np.uint32) if want_paths else None
        check(_core._lib.dsr_pipe_collect(self.h, C.byref(res), _ptr(arcs) if want_paths else None, _ptr(words) if want_paths else None))
        self._inflight = None
        return res, arcs, words

    def stage_ms(self):
        ms = (f32 * 6)(); check(_core._lib.dsr_pipe_stage_ms(self.h, ms)); return list(ms)

    def intermediate(self, which):
        p = vp(); n = i64(); check(_core._lib.dsr_pipe_intermediate(self.h, which, C.byref(p), C.byref(n))); return p.value, n.value

    def intermediate_host(self, which, dtype=np.float32):
        p, n = self.intermediate(which)
        out = np.zeros(n // np.dtype(dtype).itemsize, dtype)
        check(_core._lib.dsr_memcpy_dtoh(_ptr(out), vp(p), n, cur_stream()))
        return out
