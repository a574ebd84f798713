// csrc/viterbi.h -- what the decoder object (decoder.cpp) and the Viterbi kernel (k_viterbi.hip) share: the records both sides size and fill,
// the kernel's argument block, and the host entry points of the kernel's translation unit
#pragma once
#include "common.h"
#include "wfst_graph.h"

namespace dsr {

struct Tok { int32_t node; float ac; float lm; uint32_t bp; };        // register view; node bit31: edge input == silenceX
// token lists in memory: what a frame's beam test and expansion need (TokA) apart from what only the end phase needs (TokB)
struct TokA { float ac; float lm; uint32_t bp; uint32_t xs; };        // xs: first expansion record of the node | bit31: edge input == silenceX
struct TokB { int32_t node; int32_t cnt; };                           // cnt: number of expansion records of the node
// expansion record as the register path reads it, in two parts.  The hot record is what the expansion (P3) loads: 16 bytes of fields and the record's two language-model
// costs ALREADY SCALED -- lmCost = lmScale * (double) cost and lmEps1 = lmScale * (double) eps1, formed once on the host when the graph is set (dsr_decoder_set; lmScale is
// fixed when the decoder is created).  Exactness: decoder.cpp is built with -ffp-contract=off, and an IEEE-754 double product of the same two operands, rounded to nearest,
// is the device's __dmul_rn(lmScale, (double) cost) bit for bit -- the expansion adds the very double it used to compute per placement.
// eps1: cost of the first epsilon hop (meta bit17: it has an output).  Further hops (meta bits 18..30: hop h = 1..13 has an output):
// a two-hop path carries the second cost in p2 (float bits, scaled on the device), longer ones the offset of their hop costs in GraphDev::pathCost
// (floats, hops 2.. in order; entry 0 belongs to no path).  The expansion loads the costs of hops 2 to 4 for both placements of a pair as soon as the records
// are there and applies them in straight line, dropped by select where the path is shorter; only a wave that holds a path of more than four hops loops over the rest;
// meta bit31: more than 14 hops, walked through the path/arc arrays instead.
// The cold record is what the new token needs (P6 gathers it by record): the destination and its own expansion range.
struct XRecD { int32_t dist; uint32_t meta; int32_t dst; int32_t p2; double lmCost; double lmEps1; };
struct XRecC { int32_t dst; int32_t dstXoff; int32_t dstCnt; int32_t pad; };
struct Side { double ttl; float ac; float lm; int32_t rec; uint32_t prevBp; int32_t c; uint32_t next; };   // a later arrival at an occupied state
struct CandA { double ttl; float ac; float lm; };
struct CandB { int32_t dst; int32_t next; int32_t rec; uint32_t prevBp; };   // rec bit30: the emitting arc's input is the silence symbol
struct Bp { uint32_t prev; uint32_t rec; };
// what k_viterbi leaves of an utterance for k_traceback: the best token's back pointer (0xFFFFFFFF: nothing to trace -- no best token, or the utterance failed)
// and where the utterance's back-pointer records start in DecDev::arena, in records (its own arena in lattice mode, 0 = the pool of a time-sliced batch; its slot's arena otherwise, where the chain is followed at once: hops)
// hops: 0xFFFFFFFF = the chain is k_traceback's to follow (time-sliced batches, lattice mode, a workgroup bound to each utterance).  Where the records do not outlive the utterance --
// run to completion with more utterances than workgroups: a workgroup takes utterances from a queue and its slot's arena is its next utterance's too -- k_viterbi follows the chain itself before it moves on, into the utterance's hop scratch, and
// leaves the number of hops here.
struct TraceHead { unsigned long long arenaOff; uint32_t bp; uint32_t hops; };
// (the LDS budget of decode_plan.h counts 32 bytes per side record; the 32-bit byte offsets of the register path rest on the other sizes)
static_assert(sizeof(TokA) == 16 && sizeof(TokB) == 8 && sizeof(XRecD) == 32 && sizeof(XRecC) == 16 && sizeof(Side) == 32 && sizeof(CandA) == 16 && sizeof(CandB) == 16 && sizeof(Bp) == 8 && sizeof(TraceHead) == 16,
              "record layouts shared by the host and k_viterbi");

static constexpr int kThreads = 1024;             // 16 waves per CU at 128 VGPRs (measured in round 2: 512 x 256 VGPRs 22 % slower, 768 x 168 VGPRs 4 % slower; two 512-thread workgroups per CU 1.2x slower)
static constexpr int kFastC = 24576;               // most placements per frame on the register path (those beyond kFastK per thread are parked in memory)
static constexpr int kProfN = 56;                  // profiling words per slot: 32 phase ticks + 12 of the size-class histogram + 4 frame counts (laid out / through P1 and P2, memory-path frames below two sizes) + 8 hop counters (k_viterbi: s_hop)
static constexpr int kSideLds = 496;               // later arrivals kept in LDS (the rest go to memory)

struct GraphDev {
  int nNodes, initial;
  const int* xoff; const XRec* xrec; const XRecD* xrecD; const XRecC* xrecC; const int* xarc; const int* xpathOff;
  const int* eoff; const ERec* erec; const int* path; const float* pathCost;
  const float* arcCost; const uint32_t* arcOut; const uint32_t* arcIn;
  const int* nodeFinal; const float* nodeCost;
};

// Time slicing (segFrames > 0): a work item is one SEGMENT of an utterance -- segFrames frames -- and the items are taken in the order segment-major, utterance-minor,
// so all utterances of a batch advance together and end together.  (Run to completion, a workgroup per utterance, the workgroups end over a span of one utterance's
// duration once the queue is empty: 11 % of the launch at 1000 utterances on 256 CUs.)  Between its segments an utterance is its token list + these scalars.
struct SegState { int n, status, maxActive, pad; long arenaOff, chunkEnd, arenaUsed; double thresh; long long stat[3]; };

struct DecDev {
  double beam, lmScale, lmPenalty, silPenalty; uint32_t silenceX; int noPen;
  // time slicing: frames per segment (0: off), segments per utterance, queues (8: one per XCD, 1: one for all), the pool of back-pointer records and how many of
  // them an utterance takes at a time (a barrier pair and a device atomic each time: 9 us)
  int segFrames, segCount, segQueues, segDrop; long poolCap, poolChunk;   /* segDrop (tests): bit x set = the workgroups on XCD x do not serve their own queue */ unsigned long long* poolNext; SegState* segState; int* segDone; TokA* saveA; TokB* saveB;
  int maxTok, maxCand; long arenaCap;
  // per-slot scratch (slot s at base + s*stride)
  TokA* tokA; TokB* tokB; TokA* ctok; Side* side; int fastOK; int* tokOff; int* tokCnt; int* owner; int* rank; int* chead; CandA* cA; CandB* cB; unsigned* first; unsigned* tags; Bp* arena;
  int* queue; long long* prof;          // prof: optional per-phase wall-clock ticks (DSR_VITERBI_PROF), 16 per slot
  // dump (slot 0 only)
  int dumpOn; long dumpCap; long* dumpFrameOff; int* dumpNode; float* dumpAc; float* dumpLm; int* dumpArc; long* dumpCount;
  // lattice bookkeeping (generateLattice, decoder.h:531-541,805-953): EVERY placement of every frame is kept, per utterance, in arrival order --
  // {ac, lm, record, parent back pointer} + its unrounded total (the reference's 'worse' chains are an order-dependent function of exactly
  // these; the host replays them, lattice.cpp) -- plus, per back-pointer record, the placement that won its state, and the final token list.
  int latOn; long latCap; uint4* lat; double* latTtl; long* latFrameOff; int* arenaLat; int4* latFinal; int* latInfo;
  // topN > 0 (decoder.h:571-581): a frame expands the topN best tokens of the list in order of their scores and applies no beam; third token buffer
  int topN; TokA* tokA3; TokB* tokB3;
};

// every argument of the kernel, one struct in the kernarg segment (read through KP, see k_viterbi)
struct VitArgs {
  GraphDev G; DecDev D;
  const float* scores; const int* nframesArr; int U, Tmax, nDist;
  dsr_decode_result* res; int* arcsOut; unsigned* wordsOut; int maxPath, useLdsRow, hashN, regionB, cntCap;
  TraceHead* heads;                      // [U] written at the end of every utterance, read by k_traceback
  int* hopRec; int hopStride, walkHere;  // walkHere: the back-pointer records of an utterance are overwritten by the next one of its slot (TraceHead::hops); hopRec: TraceArgs
  int oneEach;                           // as many workgroups as utterances, run to completion: workgroup u decodes utterance u and nothing else (no queue)
};

// k_traceback (k_traceback.hip): the best path of every utterance of a launch, from the heads k_viterbi left -- arcs, words, their counts and the two statuses a path can end in
struct TraceArgs {
  const TraceHead* heads; const Bp* arena; unsigned long long arenaN;       // arenaN: records in arena (the walk stops at its end whatever a record says)
  const XRec* xrec; const ERec* erec; const int* xarc; const int* xpathOff; const int* path; const uint32_t* arcOut;
  int* hopRec; int* hopOff; int hopStride, hopCap;       // hop scratch, hopStride entries per utterance; hopCap: the capacity the status is judged by (2 x maxCand)
  dsr_decode_result* res; int* arcsOut; unsigned* wordsOut; int maxPath, U;
};

// modes: bit 0 per-phase ticks (DSR_VITERBI_PROF), bit 1 lattice bookkeeping / topN / token dump compiled in, bit 2 narrow state table
size_t viterbi_static_lds(int modes);                                                     // static LDS of k_viterbi<modes>
void viterbi_launch(int modes, const VitArgs& A, int slots, size_t ldsBytes, hipStream_t st);
void traceback_launch(const TraceArgs& A, hipStream_t st);                                // k_traceback: one wave per utterance, directly behind k_viterbi on its stream
void xcc_probe_launch(int* out64, hipStream_t st);                                        // k_xcc_probe: the XCD of each workgroup of a 64-workgroup grid

}  // namespace dsr
