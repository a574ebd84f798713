// csrc/decoder.cpp -- the decoder object of the C-ABI (dsr_decoder_*): the graph's tables on the device, the scratch memory of a decode, the launch of
// the Viterbi kernel (k_viterbi.hip, through viterbi.h) or the DecoderWordTrace kernel (k_wordtrace.hip, through wordtrace.h) as decode_plan.h decides it,
// the results of the last decode, and the hand-over of its placement log to the lattice builder (lattice.cpp).
// Built with -ffp-contract=off: the double arithmetic in here (noPen, the lattice scores) is compared bit for bit.
#include "common.h"
#include "wfst_graph.h"
#include "lattice.h"
#include "lexicon.h"
#include "wordtrace.h"
#include "viterbi.h"
#include "decode_plan.h"
#include <algorithm>
#include <cmath>

namespace dsr {

static_assert(kPlanSideBytes == (size_t) kSideLds * sizeof(Side), "decode_plan.h budgets the side records of viterbi.h");

struct DecoderState {
  dsr_decoder_cfg cfg; bool haveGraph = false; int nSlots = 0; int nNodes = 0;
  WfstGraph::Csr csr; WfstGraph::Tables tab;
  DevBuf<int> d_xoff, d_xarc, d_xpathOff, d_eoff, d_path, d_nodeFinal, d_queue; DevBuf<float> d_pathCost;
  DevBuf<XRec> d_xrec; DevBuf<ERec> d_erec; DevBuf<float> d_arcCost, d_nodeCost; DevBuf<uint32_t> d_arcOut, d_arcIn;
  DevBuf<TokA> d_tokA, d_ctok; DevBuf<TokB> d_tokB; DevBuf<Side> d_side; DevBuf<XRecD> d_xrecD; DevBuf<XRecC> d_xrecC; double recLmScale = 0.0; /* the lmScale the records' costs were scaled with */ int fastOK = 0; int maxCnt = 0; DevBuf<int> d_tokOff, d_tokCnt, d_owner, d_rank, d_chead; DevBuf<unsigned> d_tags; DevBuf<CandA> d_cA; DevBuf<CandB> d_cB; DevBuf<unsigned> d_first; DevBuf<Bp> d_arena;
  DevBuf<long long> d_prof; DevBuf<dsr_decode_result> d_res; DevBuf<int> d_arcs; DevBuf<unsigned> d_words;
  long arenaCap = 0; int initial = 0; unsigned tokenMemoryLimit = 0;
  long lastPoolCap = 0;
  hipEvent_t evTrace = nullptr;                                              // recorded behind this decoder's k_traceback (order_behind_last_traceback)
  DevBuf<TraceHead> d_heads; DevBuf<int> d_hopRec, d_hopOff;                 // k_traceback: the head of every utterance's best path; its hop scratch, per utterance
  DevBuf<SegState> d_segState; DevBuf<int> d_segDone; DevBuf<unsigned long long> d_poolNext; DevBuf<TokA> d_saveA; DevBuf<TokB> d_saveB;   // time slicing (DecDev::segFrames)
  // DecoderWordTrace mode (cfg.wordTrace): scratch of k_wordtrace.hip
  DevBuf<WTok> w_tok; DevBuf<WCand> w_cand; DevBuf<int> w_tokOff, w_rank; DevBuf<unsigned long long> w_best; DevBuf<unsigned> w_first; DevBuf<int4> w_traces; size_t w_tablesFor = 0;
  bool costNegZero = false; double costMinAbs = HUGE_VAL;      // over the arcs of the transducer set last: a cost of -0.0; the smallest non-zero |cost|
  // lattice bookkeeping of the last decode (cfg.latticeTokens > 0), per utterance
  DevBuf<uint4> d_lat; DevBuf<double> d_latTtl; DevBuf<long> d_latFrameOff; DevBuf<int> d_arenaLat; DevBuf<int4> d_latFinal; DevBuf<int> d_latInfo;
  int latU = 0, latTmax = 0; long latArenaCap = 0; WfstGraph graphCopy; DevBuf<TokA> d_tokA3; DevBuf<TokB> d_tokB3;
  // symbol tables of the transducer set last (borrowed) and the resolved silSymbol / eosSymbol (decoder.h:740-745)
  const dsr_lexicon* lexIn = nullptr; const dsr_lexicon* lexOut = nullptr; uint32_t eosX = 0; std::string eosSymbol;
  // what the last collected decode left: per-utterance results and best paths (pinned staging memory), for bestHypo / bestPath / finalStatesN
  int lastU = 0; size_t lastMaxPath = 0; bool lastPaths = false;
  PinBuf<dsr_decode_result> h_res; PinBuf<int> h_arcs; PinBuf<unsigned> h_words; hipEvent_t evDone = nullptr;
  int pendingU = 0; size_t pendingPath = 0; int pendingSlots = 0; long long* pendingProf = nullptr;
  // dump
  int dumpOn = 0; long dumpCap = 0; DevBuf<long> d_dumpFrameOff, d_dumpCount; DevBuf<int> d_dumpNode, d_dumpArc; DevBuf<float> d_dumpAc, d_dumpLm;
  std::vector<int64_t> h_dumpFrameOff; std::vector<int32_t> h_dumpNode, h_dumpArc; std::vector<float> h_dumpAc, h_dumpLm; int64_t h_dumpFrames = 0;
};

}  // namespace dsr

using namespace dsr;
struct dsr_decoder : DecoderState {};

extern "C" {

void dsr_decoder_default_cfg(dsr_decoder_cfg* c)
{ memset(c, 0, sizeof(*c)); c->beam = 100.0; c->lmScale = 12.0; c->lmPenalty = 0.0; c->silPenalty = 0.0; c->silenceX = 0xFFFFFFFFu;
  c->propagateN = 5; c->wordTraceLattice = 1; }                            // DecoderWordTrace's defaults (decoder.i:201-260; only read when wordTrace != 0)

dsr_status dsr_decoder_create(const dsr_decoder_cfg* cfg, dsr_decoder** out)
{
  return guard([&] {
    if (!cfg || !out) throw Error(DSR_E_PARAMETER, "null argument");
    require_device();
    dsr_decoder* d = new dsr_decoder(); d->cfg = *cfg;
    if (d->cfg.maxActive <= 0) d->cfg.maxActive = 65536;
    if (d->cfg.maxCandidates <= 0) d->cfg.maxCandidates = 8 * d->cfg.maxActive;
    if (d->cfg.maxCandidates >= (1 << 24)) throw Error(DSR_E_PARAMETER, "maxCandidates must be < 2^24");
    if (d->cfg.streams <= 0) {
      hipDeviceProp_t prop; int dev = 0; DSR_HIP(hipGetDevice(&dev)); DSR_HIP(hipGetDeviceProperties(&prop, dev));
      d->cfg.streams = prop.multiProcessorCount;
      const int t = read_vit_env().slots; if (t > 0) d->cfg.streams = t;
    }
    *out = d;
  });
}
// A decode's workgroups take their CUs whole (registers and LDS), and a decode queued on another stream moves in as the one before frees them: by the time that
// one has ended and its k_traceback may start, a grid of one workgroup per CU has left no room for even one small wave, and the finished decode's paths would wait
// for the whole next decode (measured with two pipes: results 87 ms late on every other step).  So a decode kernel whose grid fills the device on its own -- at least
// as many workgroups as the device has CUs -- is ordered behind the traceback launched last on the device, whichever decoder and stream it came from: it gives up the
// start in the other decode's ragged end (decodes of that size on one device do not overlap any more), the traceback runs on an empty device for half a millisecond.
// A smaller grid leaves CUs free, the traceback's waves find room there, and such decodes run side by side as before.  (The event may be this decoder's own, from a
// launch on another stream: that decode has been collected, the event is complete, the wait is none.)
namespace {
std::mutex g_traceMu; std::map<int, std::pair<const dsr_decoder*, hipEvent_t>> g_lastTrace; std::map<int, int> g_cuCount;     // by device id
void order_behind_last_traceback(int slots, hipStream_t st)
{
  std::lock_guard<std::mutex> lock(g_traceMu);
  int dev = 0; DSR_HIP(hipGetDevice(&dev));
  auto cu = g_cuCount.find(dev);
  if (cu == g_cuCount.end()) { int n = 0; DSR_HIP(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev)); cu = g_cuCount.emplace(dev, n).first; }
  if (slots < cu->second) return;
  const auto it = g_lastTrace.find(dev);
  if (it != g_lastTrace.end()) DSR_HIP(hipStreamWaitEvent(st, it->second.second, 0));
}
void publish_traceback(dsr_decoder* d, hipStream_t st)
{
  std::lock_guard<std::mutex> lock(g_traceMu);
  if (!d->evTrace) DSR_HIP(hipEventCreateWithFlags(&d->evTrace, hipEventDisableTiming));
  DSR_HIP(hipEventRecord(d->evTrace, st));
  int dev = 0; DSR_HIP(hipGetDevice(&dev));
  g_lastTrace[dev] = std::make_pair((const dsr_decoder*) d, d->evTrace);
}
void forget_traceback(const dsr_decoder* d)
{
  std::lock_guard<std::mutex> lock(g_traceMu);
  for (auto it = g_lastTrace.begin(); it != g_lastTrace.end(); ) { if (it->second.first == d) it = g_lastTrace.erase(it); else ++it; }
}
}  // namespace

void dsr_decoder_destroy(dsr_decoder* d)
{
  if (!d) return;
  forget_traceback(d);
  if (d->evDone) (void) hipEventDestroy(d->evDone);
  if (d->evTrace) (void) hipEventDestroy(d->evTrace);
  delete d;
}

dsr_status dsr_decoder_set(dsr_decoder* d, const dsr_wfst* g)
{
  return guard([&] {
    if (!d || !g) throw Error(DSR_E_PARAMETER, "null argument");
    if (g->initial < 0) throw Error(DSR_E_CONSISTENCY, "the transducer has no arcs");
    d->csr = g->csr(); d->tab = g->tables(d->csr, (size_t) 1 << 28);
    d->nNodes = (int) g->nodes.size(); d->initial = g->initial; d->graphCopy = *g;
    std::vector<int> nf(d->nNodes); std::vector<float> nc(d->nNodes);
    for (int i = 0; i < d->nNodes; i++) { nf[i] = g->nodes[i].final_; nc[i] = g->nodes[i].cost; }
    d->d_xoff.upload(d->tab.xoff); d->d_eoff.upload(d->tab.eoff); d->d_path.upload(d->tab.path);
    if (d->tab.xrec.empty()) throw Error(DSR_E_CONSISTENCY, "the transducer has no emitting arcs");
    d->d_xrec.upload(d->tab.xrec); d->d_xarc.upload(d->tab.xarc); d->d_xpathOff.upload(d->tab.xpathOff);
    {
      // expansion records of the register path (viterbi.h): the hot record with the two costs scaled by this decoder's lmScale -- the products the expansion formed
      // for every placement are constants of (decoder, graph) -- and the cold record with the destination's own expansion range folded in (the register path
      // never reads xoff).  Both are this decoder's own: two decoders of different lmScale made from one transducer share nothing.
      const size_t nx = d->tab.xrec.size(); std::vector<XRecD> xd(nx); std::vector<XRecC> xc(nx); int maxCnt = 0; std::vector<float> pc(1, 0.0f);
      const double lmS = d->cfg.lmScale; d->recLmScale = lmS;
      for (size_t r = 0; r < nx; r++) {
        const XRec& x = d->tab.xrec[r]; XRecD& o = xd[r]; XRecC& oc = xc[r];
        o.dst = x.dst; o.dist = x.dist; o.lmCost = lmS * (double) x.cost; o.meta = x.meta;
        oc.dst = x.dst; oc.dstXoff = d->tab.xoff[x.dst]; oc.dstCnt = d->tab.xoff[x.dst + 1] - d->tab.xoff[x.dst]; oc.pad = 0;
        const int po = d->tab.xpathOff[r], plen = (int) (x.meta & 0xFFFFu); o.p2 = 0; float eps1 = 0.0f;
        if (x.meta >> 18) throw Error(DSR_E_CONSISTENCY, "expansion record %zu: meta bits above 17 are in use", r);
        if (plen) { const int a0 = d->tab.path[po]; eps1 = d->csr.cost[a0]; if (d->csr.out[a0] != 0) o.meta |= 0x20000u; }
        o.lmEps1 = lmS * (double) eps1;
        if (plen > 14) o.meta |= 0x80000000u;
        else if (plen > 1) {
          if (plen == 2) { const float c1 = d->csr.cost[d->tab.path[po + 1]]; memcpy(&o.p2, &c1, 4); }
          else { o.p2 = (int) pc.size(); for (int h = 1; h < plen; h++) pc.push_back(d->csr.cost[d->tab.path[po + h]]); }
          for (int h = 1; h < plen; h++) if (d->csr.out[d->tab.path[po + h]] != 0) o.meta |= 1u << (17 + h);
        }
        if (oc.dstCnt > maxCnt) maxCnt = oc.dstCnt;
      }
      d->d_xrecD.upload(xd); d->d_xrecC.upload(xc); d->d_pathCost.upload(pc);
      // (the register path addresses both record arrays with 32-bit byte offsets: 2^27 records x 32 bytes of the hot record is the bound, the 16-byte cold records end below 2^31)
      d->fastOK = (maxCnt < (1 << 19) && nx < ((size_t) 1 << 27)) ? 1 : 0; d->maxCnt = maxCnt;
      if (read_vit_env().noFast) d->fastOK = 0;
    }
    { std::vector<ERec> e = d->tab.erec; if (e.empty()) e.push_back(ERec{0, 0, 0, 0}); d->d_erec.upload(e); }
    d->d_arcCost.upload(d->csr.cost); d->d_arcOut.upload(d->csr.out); d->d_arcIn.upload(d->csr.in);
    d->costNegZero = false; d->costMinAbs = HUGE_VAL;
    for (size_t a = 0; a < d->csr.cost.size(); a++) {
      const float c = d->csr.cost[a]; uint32_t bits; memcpy(&bits, &c, 4);
      if (bits == 0x80000000u) d->costNegZero = true;
      if (c != 0.0f && std::fabs((double) c) < d->costMinAbs) d->costMinAbs = std::fabs((double) c);
    }
    d->d_nodeFinal.upload(nf); d->d_nodeCost.upload(nc);
    d->haveGraph = true; d->nSlots = 0;    // scratch is (re)allocated by the first decode
  });
}
// DecoderFlyWeight::set(wfst) = _Decoder::_set (decoder.h:740-745): the network and, through its lexica, the indices of silSymbol (input
// lexicon) and eosSymbol (output lexicon); a missing symbol is the reference's jkey_error (mlist.h:109-114).  Symbols may be NULL when the
// transducer carries no lexica (then cfg.silenceX stays as configured).
dsr_status dsr_decoder_set_symbols(dsr_decoder* d, const dsr_wfst* g, const char* silSymbol, const char* eosSymbol)
{
  return guard([&] {
    if (!d || !g) throw Error(DSR_E_PARAMETER, "null argument");
    uint32_t silX = d->cfg.silenceX, eosX = 0;
    if (silSymbol) { if (!g->lexIn) throw Error(DSR_E_KEY, "the transducer has no input lexicon to look '%s' up in", silSymbol); silX = g->lexIn->index(silSymbol); }
    if (eosSymbol) { if (!g->lexOut) throw Error(DSR_E_KEY, "the transducer has no output lexicon to look '%s' up in", eosSymbol); eosX = g->lexOut->index(eosSymbol); }
    const dsr_status s = dsr_decoder_set(d, g);
    if (s != DSR_OK) throw Error(s, "%s", dsr_last_error());
    d->cfg.silenceX = silX; d->eosX = eosX; d->lexIn = g->lexIn; d->lexOut = g->lexOut; d->eosSymbol = eosSymbol ? eosSymbol : "";
  });
}
uint32_t dsr_decoder_eos_index(const dsr_decoder* d) { return d ? d->eosX : 0; }

// Results of the last collected decode, utterance u.  bestHypo(useInputSymbols) (decoder.h:748-773): the output symbols != 0 along the best path, or
// the input symbols != 0 with immediate repetitions dropped ("inX != 0 && inX != lastX", walking the path from its END, so a repetition is judged
// against the symbol after it), each followed by a blank.  bestPath() (:775-797): the names of the distributions along the path = the input
// symbols != 0, one per line.  Strings need the lexica (DSR_E_KEY without); the id variants do not.
static void need_last(const dsr_decoder* d, int u, bool paths)
{
  if (!d) throw Error(DSR_E_PARAMETER, "null argument");
  if (d->lastU <= 0) throw Error(DSR_E_CONSISTENCY, "no decode has been collected yet");
  if (u < 0 || u >= d->lastU) throw Error(DSR_E_INDEX, "utterance %d of %d", u, d->lastU);
  if (paths && !d->lastPaths) throw Error(DSR_E_CONSISTENCY, "the last decode was collected without its paths");
  if (d->h_res.p[u].status != DSR_OK) throw Error(d->h_res.p[u].status, "utterance %d was not decoded (status %d)", u, d->h_res.p[u].status);
}
// ids: the path's symbol ids in time order (which: 0 outputs != 0; 1 inputs != 0 with repetitions dropped as bestHypo(true); 2 inputs != 0 as bestPath)
static std::vector<uint32_t> path_ids(const dsr_decoder* d, int u, int which)
{
  need_last(d, u, true);
  const dsr_decode_result& r = d->h_res.p[u];
  const int n = r.nArcs < (int) d->lastMaxPath ? r.nArcs : (int) d->lastMaxPath;
  const int* arcs = d->h_arcs.p + (size_t) u * d->lastMaxPath;
  std::vector<uint32_t> ids;
  if (which == 1) {                                              // from the end, as the reference walks prev(): keep inX when it differs from the LAST KEPT one
    uint32_t lastX = 0;
    for (int i = n - 1; i >= 0; i--) { const uint32_t inX = d->csr.in[arcs[i]]; if (inX != 0 && inX != lastX) { ids.push_back(inX); lastX = inX; } }
    std::reverse(ids.begin(), ids.end());
  } else for (int i = 0; i < n; i++) { const uint32_t v = which == 0 ? d->csr.out[arcs[i]] : d->csr.in[arcs[i]]; if (v != 0) ids.push_back(v); }
  return ids;
}
dsr_status dsr_decoder_path_ids(const dsr_decoder* d, int u, int which, uint32_t* ids, int cap, int* n)
{
  return guard([&] {
    if (!n || which < 0 || which > 2) throw Error(DSR_E_PARAMETER, "bad argument");
    const std::vector<uint32_t> v = path_ids(d, u, which);
    *n = (int) v.size();
    if (ids) { if ((int) v.size() > cap) throw Error(DSR_E_DIMENSION, "buffer holds %d ids, the path has %zu", cap, v.size()); if (!v.empty()) memcpy(ids, v.data(), 4 * v.size()); }
  });
}
static void put_string(const std::string& s, char* buf, size_t cap, size_t* need)
{
  if (need) *need = s.size() + 1;
  if (buf) { if (s.size() + 1 > cap) throw Error(DSR_E_DIMENSION, "buffer holds %zu bytes, the string needs %zu", cap, s.size() + 1); memcpy(buf, s.c_str(), s.size() + 1); }
}
dsr_status dsr_decoder_best_hypo(const dsr_decoder* d, int u, int useInputSymbols, char* buf, size_t cap, size_t* need)
{
  return guard([&] {
    const std::vector<uint32_t> v = path_ids(d, u, useInputSymbols ? 1 : 0);
    const dsr_lexicon* lex = useInputSymbols ? d->lexIn : d->lexOut;
    if (!lex) throw Error(DSR_E_KEY, "the transducer set on this decoder has no %s lexicon", useInputSymbols ? "input" : "output");
    std::string s; for (size_t i = 0; i < v.size(); i++) { s += lex->symbol(v[i]); s += " "; }
    put_string(s, buf, cap, need);
  });
}
dsr_status dsr_decoder_best_path(const dsr_decoder* d, int u, char* buf, size_t cap, size_t* need, int* count)
{
  return guard([&] {
    const std::vector<uint32_t> v = path_ids(d, u, 2);
    if (!d->lexIn) throw Error(DSR_E_KEY, "the transducer set on this decoder has no input lexicon");
    std::string s; for (size_t i = 0; i < v.size(); i++) { s += d->lexIn->symbol(v[i]); s += "\n"; }
    if (count) *count = (int) v.size();
    put_string(s, buf, cap, need);
  });
}
dsr_status dsr_decoder_final_states_n(const dsr_decoder* d, int u, int* n)
{ return guard([&] { if (!n) throw Error(DSR_E_PARAMETER, "null argument"); need_last(d, u, false); *n = d->h_res.p[u].finalStatesN; }); }
dsr_status dsr_decoder_trace_back_succeeded(const dsr_decoder* d, int u, int* ok)
{ return guard([&] { if (!ok) throw Error(DSR_E_PARAMETER, "null argument"); need_last(d, u, false); *ok = d->h_res.p[u].reachedFinal; }); }

// _Decoder::setTokenMemoryLimit(limit) (decoder.h:396) caps the reference's Token memory pool (MemoryManager).  Tokens here live in per-slot
// arrays sized by cfg.maxActive / maxCandidates / arenaTokens (a decode that outgrows them returns DSR_E_ALLOCATION for that utterance): there
// is no pool to limit.  The value is accepted and kept so that drivers that set it run unchanged.
dsr_status dsr_decoder_set_token_memory_limit(dsr_decoder* d, unsigned limit)
{ return guard([&] { if (!d) throw Error(DSR_E_PARAMETER, "null argument"); d->tokenMemoryLimit = limit; }); }
unsigned dsr_decoder_token_memory_limit(const dsr_decoder* d) { return d ? d->tokenMemoryLimit : 0u; }

dsr_status dsr_decoder_set_beam(dsr_decoder* d, double beam) { return guard([&] { if (!d) throw Error(DSR_E_PARAMETER, "null argument"); d->cfg.beam = beam; }); }

dsr_status dsr_decoder_enable_dump(dsr_decoder* d, int en) { return guard([&] { if (!d) throw Error(DSR_E_PARAMETER, "null argument"); d->dumpOn = en; }); }

// Which XCD a workgroup lands on (k_xcc_probe, k_viterbi.hip).  The XCD-bound queues of the time-sliced decode rest on two properties of the dispatcher that are
// checked here once per device instead of assumed: eight XCDs numbered 0..7, and workgroup i of a grid on XCD (i mod 8) -- so that a grid of 8 k workgroups
// serves every queue.
static bool xcd_round_robin(hipStream_t st)
{
  static std::mutex mu; static std::map<int, bool> known;                 // by device id
  std::lock_guard<std::mutex> lock(mu);
  int dev = 0; DSR_HIP(hipGetDevice(&dev));
  const auto it = known.find(dev); if (it != known.end()) return it->second;
  DevBuf<int> o; o.reserve(64); int h[64];
  xcc_probe_launch(o.p, st);
  DSR_HIP(hipMemcpyAsync(h, o.p, sizeof(h), hipMemcpyDeviceToHost, st)); DSR_HIP(hipStreamSynchronize(st));
  bool ok = true; unsigned seen = 0;
  for (int i = 0; i < 64; i++) { if (h[i] < 0 || h[i] > 7 || h[i] != h[i & 7]) ok = false; }
  for (int i = 0; i < 8 && ok; i++) seen |= 1u << h[i];
  return known[dev] = ok && seen == 0xFFu;
}

static void ensure_scratch(dsr_decoder* d, int slots, int Tmax, int arenas)
{
  const dsr_decoder_cfg& c = d->cfg;
  long arena = c.arenaTokens > 0 ? (long) c.arenaTokens : (long) 8192 * (long) (Tmax + 2);
  if (arena > 0x7FFFFFF0L) arena = 0x7FFFFFF0L;
  // (the kernel strides the arenas, and sizes a sliced batch's pool, by d->arenaCap -- the largest arena so far, not this batch's: that is what has to fit)
  if (slots <= d->nSlots && arena <= d->arenaCap && (size_t) (arenas > slots ? arenas : slots) * (size_t) d->arenaCap <= d->d_arena.n) return;
  if (slots < d->nSlots) slots = d->nSlots;
  if (arena < d->arenaCap) arena = d->arenaCap;
  const size_t S = (size_t) slots;
  d->d_tokA.reserve(S * 2 * c.maxActive); d->d_tokB.reserve(S * 2 * c.maxActive); d->d_ctok.reserve(S * 8192); d->d_side.reserve(S * kFastC);
  d->d_tokOff.reserve(S * (c.maxActive + 1));
  d->d_owner.reserve(S * c.maxCandidates); d->d_rank.reserve(S * c.maxCandidates);
  d->d_cA.reserve(S * c.maxCandidates); d->d_cB.reserve(S * c.maxCandidates);
  d->d_first.reserve(S * d->nNodes); d->d_tokCnt.reserve(S * (c.maxActive + 1)); d->d_chead.reserve(S * c.maxCandidates);
  d->d_tags.reserve(S); DSR_HIP(hipMemset(d->d_tags.p, 0, S * sizeof(unsigned)));          // tag 0 = wipe the table on first use
  d->d_arena.reserve((size_t) (arenas > slots ? arenas : slots) * (size_t) arena);
  d->d_queue.reserve(8);
  d->nSlots = slots; d->arenaCap = arena;
}

// every input symbol must name a distribution (decoder.h:985: _dist->find(distX-1))
static void check_arc_inputs(const dsr_decoder* d, int nDist)
{ for (size_t a = 0; a < d->csr.in.size(); a++) if (d->csr.in[a] > (uint32_t) nDist) throw Error(DSR_E_INDEX, "arc input %u has no distribution (nDist=%d)", d->csr.in[a], nDist); }

// the copies of the results into pinned staging memory, the event collect waits for, and what collect needs to know of the launch
static void enqueue_result_copies(dsr_decoder* d, int U, size_t nPath, hipStream_t st)
{
  d->h_res.reserve(U); d->h_arcs.reserve(nPath ? nPath : 1); d->h_words.reserve(nPath ? nPath : 1);
  DSR_HIP(hipMemcpyAsync(d->h_res.p, d->d_res.p, sizeof(dsr_decode_result) * U, hipMemcpyDeviceToHost, st));
  if (nPath) DSR_HIP(hipMemcpyAsync(d->h_arcs.p, d->d_arcs.p, sizeof(int) * nPath, hipMemcpyDeviceToHost, st));
  if (nPath) DSR_HIP(hipMemcpyAsync(d->h_words.p, d->d_words.p, sizeof(unsigned) * nPath, hipMemcpyDeviceToHost, st));
  if (!d->evDone) DSR_HIP(hipEventCreateWithFlags(&d->evDone, hipEventDisableTiming));
  DSR_HIP(hipEventRecord(d->evDone, st));
  d->pendingU = U; d->pendingPath = nPath;
}

// DecoderWordTrace (decoder.h:1146-1304).  With generateLattice -- the reference's default -- _placeOnList merges the worse chains of two tokens and reads
// wordTrace()->wordSequenceX() of each (decoder.cc:239); a token that has not crossed a word boundary has a null word trace: undefined behaviour in the
// reference on any transducer whose first arcs carry no output symbol.  That search is not built; the 1-best search (generateLattice = false) is.
static void launch_wordtrace(dsr_decoder* d, const float* score, const int32_t* nframes, int U, int Tmax, int nDist, int maxPath, int want_paths, hipStream_t st)
{
  if (d->cfg.wordTraceLattice) throw Error(DSR_E_CONSISTENCY, "DecoderWordTrace with generateLattice: not built (the shipped _placeOnList dereferences the null word trace of "
                                           "every token that has not crossed a word boundary, decoder.cc:239); construct it with generateLattice = false");
  if (d->cfg.topN > 0 || d->cfg.latticeTokens > 0 || d->dumpOn) throw Error(DSR_E_PARAMETER, "DecoderWordTrace: no topN (its frame loop has no such branch, decoder.cc:147-183), lattice bookkeeping or dump");
  check_arc_inputs(d, nDist);
  int slots = d->cfg.streams; if (slots > U) slots = U;
  const dsr_decoder_cfg& c = d->cfg; const size_t S = (size_t) slots;
  const long maxTraces = c.wordTraces > 0 ? (long) c.wordTraces : (long) 1 << 20;
  d->w_tok.reserve(S * 2 * c.maxActive); d->w_cand.reserve(S * c.maxCandidates); d->w_tokOff.reserve(S * (c.maxActive + 1)); d->w_rank.reserve(S * c.maxCandidates);
  d->w_traces.reserve((size_t) U * maxTraces); d->d_queue.reserve(8); d->d_res.reserve(U);
  if (d->w_tablesFor != S * d->nNodes) {                               // the per-state tables are all ones between frames: set once, the kernel restores them
    d->w_best.reserve(S * d->nNodes); d->w_first.reserve(S * d->nNodes); d->w_tablesFor = S * d->nNodes;
    DSR_HIP(hipMemsetAsync(d->w_best.p, 0xFF, sizeof(unsigned long long) * S * d->nNodes, st)); DSR_HIP(hipMemsetAsync(d->w_first.p, 0xFF, sizeof(unsigned) * S * d->nNodes, st));
  }
  if (maxPath < 1) maxPath = 1;
  d->d_arcs.reserve((size_t) U * maxPath); d->d_words.reserve((size_t) U * maxPath);
  DSR_HIP(hipMemsetAsync(d->d_queue.p, 0, 8 * sizeof(int), st));
  WtArgs A; A.nNodes = d->nNodes; A.initial = d->initial; A.xoff = d->d_xoff.p; A.xrec = d->d_xrec.p; A.xarc = d->d_xarc.p; A.xpathOff = d->d_xpathOff.p; A.eoff = d->d_eoff.p;
  A.erec = d->d_erec.p; A.path = d->d_path.p; A.arcCost = d->d_arcCost.p; A.arcOut = d->d_arcOut.p; A.arcIn = d->d_arcIn.p; A.nodeFinal = d->d_nodeFinal.p; A.nodeCost = d->d_nodeCost.p;
  A.beam = c.beam; A.lmScale = c.lmScale; A.lmPenalty = c.lmPenalty; A.silPenalty = c.silPenalty; A.silenceX = c.silenceX; A.insertSilence = c.insertSilence;
  A.maxTok = c.maxActive; A.maxCand = c.maxCandidates; A.maxTraces = maxTraces;
  A.tok = d->w_tok.p; A.cand = d->w_cand.p; A.tokOff = d->w_tokOff.p; A.rank = d->w_rank.p; A.bestKey = d->w_best.p; A.firstSlot = d->w_first.p; A.traces = d->w_traces.p; A.queue = d->d_queue.p;
  A.scores = score; A.nframes = nframes; A.U = U; A.Tmax = Tmax; A.nDist = nDist; A.res = d->d_res.p; A.arcsOut = d->d_arcs.p; A.wordsOut = d->d_words.p; A.maxPath = maxPath;
  wordtrace_launch(A, slots, st);
  enqueue_result_copies(d, U, want_paths ? (size_t) U * maxPath : 0, st);
  d->pendingSlots = slots; d->pendingProf = nullptr; d->latU = 0;
}

// The kernel's argument block from the decoder's state and the plan; reserves and clears the buffers that depend on the batch (ensure_scratch has run).
static VitArgs fill_vit_args(dsr_decoder* d, const DecodePlan& P, const VitEnv& env, const float* score, const int32_t* nframes, int U, int Tmax, int nDist,
                             int maxPath, bool wantPaths, hipStream_t st)
{
  const int slots = P.slots; const bool latOn = d->cfg.latticeTokens > 0;
  d->d_res.reserve(U);
  if (wantPaths) { d->d_arcs.reserve((size_t) U * (maxPath > 0 ? maxPath : 1)); d->d_words.reserve((size_t) U * (maxPath > 0 ? maxPath : 1)); }
  DSR_HIP(hipMemsetAsync(d->d_queue.p, 0, 8 * sizeof(int), st));
  d->d_heads.reserve(U); DSR_HIP(hipMemsetAsync(d->d_heads.p, 0xFF, sizeof(TraceHead) * (size_t) U, st));      // every head empty: one the kernel does not write is not followed
  if (d->dumpOn) {
    d->dumpCap = (long) d->cfg.maxActive * 64 < (long) 1 << 26 ? (long) 1 << 24 : (long) 1 << 26;
    d->d_dumpFrameOff.reserve(Tmax + 2); d->d_dumpCount.reserve(2);
    d->d_dumpNode.reserve(d->dumpCap); d->d_dumpArc.reserve(d->dumpCap); d->d_dumpAc.reserve(d->dumpCap); d->d_dumpLm.reserve(d->dumpCap);
    DSR_HIP(hipMemsetAsync(d->d_dumpCount.p, 0, 2 * sizeof(long), st));
  }
  VitArgs A; GraphDev& G = A.G; DecDev& D = A.D;
  G.nNodes = d->nNodes; G.initial = d->initial; G.xoff = d->d_xoff.p; G.xrec = d->d_xrec.p; G.xrecD = d->d_xrecD.p; G.xrecC = d->d_xrecC.p; G.xarc = d->d_xarc.p;
  G.xpathOff = d->d_xpathOff.p; G.eoff = d->d_eoff.p; G.erec = d->d_erec.p; G.path = d->d_path.p; G.pathCost = d->d_pathCost.p; G.arcCost = d->d_arcCost.p;
  G.arcOut = d->d_arcOut.p; G.arcIn = d->d_arcIn.p; G.nodeFinal = d->d_nodeFinal.p; G.nodeCost = d->d_nodeCost.p;
  // (the records carry lmScale x cost: nothing changes the scale after dsr_decoder_set today; should that ever be added, the records have to be rebuilt with it)
  if (memcmp(&d->recLmScale, &d->cfg.lmScale, sizeof(double)) != 0) throw Error(DSR_E_CONSISTENCY, "lmScale changed after the transducer was set");
  D.beam = d->cfg.beam; D.lmScale = d->cfg.lmScale; D.lmPenalty = d->cfg.lmPenalty; D.silPenalty = d->cfg.silPenalty;
  // penalty-free expansion (k_viterbi, expandR): both penalty products zero, and no placement's lm can be -0.0 -- lmScale > 0, no arc cost of -0.0, and every
  // non-zero lmScale x cost at least 2^-60 in magnitude (a sum float + double of that size is 0 or at least 2^-112: it cannot round to -0.0f)
  D.noPen = (d->cfg.lmScale > 0.0 && std::isfinite(d->cfg.lmScale) && d->cfg.lmScale * d->cfg.lmPenalty == 0.0 && d->cfg.lmScale * d->cfg.silPenalty == 0.0 &&
             !d->costNegZero && (d->costMinAbs == HUGE_VAL || d->cfg.lmScale * d->costMinAbs >= 0x1p-60) && !env.pen) ? 1 : 0;
  D.silenceX = d->cfg.silenceX; D.maxTok = d->cfg.maxActive; D.maxCand = d->cfg.maxCandidates; D.arenaCap = d->arenaCap;
  D.tokA = d->d_tokA.p; D.tokB = d->d_tokB.p; D.ctok = d->d_ctok.p; D.side = d->d_side.p; D.fastOK = d->fastOK; D.tokOff = d->d_tokOff.p; D.owner = d->d_owner.p; D.rank = d->d_rank.p; D.cA = d->d_cA.p; D.cB = d->d_cB.p;
  D.first = d->d_first.p; D.tags = d->d_tags.p; D.tokCnt = d->d_tokCnt.p; D.chead = d->d_chead.p; D.arena = d->d_arena.p; D.queue = d->d_queue.p;
  D.segDrop = env.segDrop; D.segQueues = P.segQueues; D.segFrames = P.segFrames; D.segCount = P.segCount;
  D.poolCap = 0; D.poolChunk = 0; D.poolNext = nullptr; D.segState = nullptr; D.segDone = nullptr; D.saveA = nullptr; D.saveB = nullptr;
  if (P.segFrames > 0) {
    d->d_segState.reserve(U); d->d_segDone.reserve(U); d->d_poolNext.reserve(1);
    d->d_saveA.reserve((size_t) U * d->cfg.maxActive); d->d_saveB.reserve((size_t) U * d->cfg.maxActive);
    DSR_HIP(hipMemsetAsync(d->d_segDone.p, 0, sizeof(int) * (size_t) U, st)); DSR_HIP(hipMemsetAsync(d->d_poolNext.p, 0, sizeof(unsigned long long), st));
    D.poolCap = (long) ((size_t) std::max(P.poolArenas, slots) * (size_t) d->arenaCap); if (D.poolCap > (long) 0xFFFFFFF0L) D.poolCap = (long) 0xFFFFFFF0L;
    D.poolChunk = std::min<long>(262144, std::max<long>(4096, D.poolCap / (4 * (long) U)));      // (what an utterance leaves unused of its last run: at most a quarter of the pool in all)
    D.poolNext = d->d_poolNext.p; D.segState = d->d_segState.p; D.segDone = d->d_segDone.p; D.saveA = d->d_saveA.p; D.saveB = d->d_saveB.p;
  }
  d->lastPoolCap = D.poolCap;
  D.prof = nullptr;
  if (env.prof) { d->d_prof.reserve((size_t) slots * kProfN); D.prof = d->d_prof.p; }
  D.dumpOn = d->dumpOn; D.dumpCap = d->dumpCap; D.dumpFrameOff = d->d_dumpFrameOff.p; D.dumpNode = d->d_dumpNode.p; D.dumpAc = d->d_dumpAc.p;
  D.dumpLm = d->d_dumpLm.p; D.dumpArc = d->d_dumpArc.p; D.dumpCount = d->d_dumpCount.p;
  D.topN = d->cfg.topN > 0 ? d->cfg.topN : 0; D.tokA3 = nullptr; D.tokB3 = nullptr;
  if (D.topN > 0) { d->d_tokA3.reserve((size_t) slots * d->cfg.maxActive); d->d_tokB3.reserve((size_t) slots * d->cfg.maxActive); D.tokA3 = d->d_tokA3.p; D.tokB3 = d->d_tokB3.p; }
  D.latOn = latOn ? 1 : 0; D.latCap = 0; D.lat = nullptr; D.latTtl = nullptr; D.latFrameOff = nullptr; D.arenaLat = nullptr; D.latFinal = nullptr; D.latInfo = nullptr;
  if (latOn) {
    const size_t cap = (size_t) d->cfg.latticeTokens;
    d->d_lat.reserve((size_t) U * cap); d->d_latTtl.reserve((size_t) U * cap); d->d_latFrameOff.reserve((size_t) U * (Tmax + 3));
    d->d_arenaLat.reserve((size_t) U * (size_t) d->arenaCap); d->d_latFinal.reserve((size_t) U * d->cfg.maxActive); d->d_latInfo.reserve((size_t) 4 * U);
    DSR_HIP(hipMemsetAsync(d->d_latInfo.p, 0, sizeof(int) * 4 * (size_t) U, st));
    D.latCap = (long) cap; D.lat = d->d_lat.p; D.latTtl = d->d_latTtl.p; D.latFrameOff = d->d_latFrameOff.p; D.arenaLat = d->d_arenaLat.p; D.latFinal = d->d_latFinal.p; D.latInfo = d->d_latInfo.p;
    d->latU = U; d->latTmax = Tmax; d->latArenaCap = d->arenaCap;
  } else d->latU = 0;
  A.scores = score; A.nframesArr = nframes; A.U = U; A.Tmax = Tmax; A.nDist = nDist; A.res = d->d_res.p;
  A.arcsOut = wantPaths ? d->d_arcs.p : nullptr; A.wordsOut = wantPaths ? d->d_words.p : nullptr; A.maxPath = maxPath;
  A.useLdsRow = P.useLdsRow; A.hashN = P.hashN; A.regionB = (int) (kSideLds * sizeof(Side)); A.cntCap = P.cntCap;
  A.heads = d->d_heads.p;
  // hop scratch of the traceback, per utterance.  A chain has at most one record per frame and the end expansion's, so min(2 x maxCand, Tmax + 2) entries hold it.
  A.hopStride = std::max(1, std::min(2 * D.maxCand, Tmax + 2));
  d->d_hopRec.reserve((size_t) U * A.hopStride); d->d_hopOff.reserve((size_t) U * A.hopStride); A.hopRec = d->d_hopRec.p;
  // back-pointer records outlive their utterance in the pool of a time-sliced batch, in lattice mode (an arena per utterance), and where every workgroup decodes
  // exactly one utterance: with as many workgroups as utterances the kernel binds utterance u to workgroup u instead of dealing them out from the queue (oneEach; from
  // the queue, a workgroup that ends a short utterance before the whole grid is resident would take another into its arena).  Everywhere else -- run to completion
  // with more utterances than workgroups -- a slot's arena is its next utterance's too, and the kernel follows the chain before it moves on.
  A.oneEach = (P.segFrames == 0 && slots == U) ? 1 : 0;
  A.walkHere = (P.segFrames == 0 && !latOn && !A.oneEach) ? 1 : 0;
  return A;
}

// k_traceback's arguments from the decode's: the graph tables a path is spelled out with, the heads, the results, and the hop scratch (the status is judged by
// 2 x maxCand hops as it always was).
static TraceArgs fill_trace_args(dsr_decoder* d, const VitArgs& V)
{
  TraceArgs A; A.hopCap = 2 * V.D.maxCand; A.hopStride = V.hopStride;
  A.heads = V.heads; A.arena = V.D.arena; A.arenaN = (unsigned long long) d->d_arena.n;
  A.xrec = V.G.xrec; A.erec = V.G.erec; A.xarc = V.G.xarc; A.xpathOff = V.G.xpathOff; A.path = V.G.path; A.arcOut = V.G.arcOut;
  A.hopRec = d->d_hopRec.p; A.hopOff = d->d_hopOff.p;
  A.res = V.res; A.arcsOut = V.arcsOut; A.wordsOut = V.wordsOut; A.maxPath = V.maxPath; A.U = V.U;
  return A;
}

// Asynchronous halves of decode_batch: launch enqueues the kernel and the copies of the results into pinned staging
// memory on `stream` and returns; collect waits for that work and hands the results out.  One launch may be in flight
// per decoder object (its scratch memory belongs to the launch).
dsr_status dsr_decoder_decode_launch(dsr_decoder* d, const float* score, const int32_t* nframes, int U, int Tmax, int nDist,
                                     int maxPath, int want_paths, void* stream)
{
  return guard([&] {
    if (!d || !score || !nframes) throw Error(DSR_E_PARAMETER, "null argument");
    if (!d->haveGraph) throw Error(DSR_E_INITIALIZATION, "call set() with a transducer first");
    if (d->pendingU > 0) throw Error(DSR_E_CONSISTENCY, "a decode is already in flight on this decoder: collect it first");
    if (U <= 0) return;
    hipStream_t st = (hipStream_t) stream;
    if (d->cfg.wordTrace) { launch_wordtrace(d, score, nframes, U, Tmax, nDist, maxPath, want_paths, st); return; }
    check_arc_inputs(d, nDist);
    const bool latOn = d->cfg.latticeTokens > 0;
    if (latOn && d->dumpOn) throw Error(DSR_E_PARAMETER, "lattice bookkeeping and the token dump are separate debugging aids: enable one");
    const VitEnv env = read_vit_env();
    PlanIn in; in.streams = d->cfg.streams; in.maxActive = d->cfg.maxActive; in.arenaTokens = d->cfg.arenaTokens; in.latticeTokens = d->cfg.latticeTokens;
    in.topN = d->cfg.topN; in.dumpOn = d->dumpOn != 0; in.nNodes = d->nNodes; in.maxCnt = d->maxCnt; in.U = U; in.Tmax = Tmax; in.nDist = nDist;
    in.staticLds = viterbi_static_lds(plan_base_modes(in, env));
    const DecodePlan P = plan_decode(in, env, [&] { return xcd_round_robin(st); });
    ensure_scratch(d, P.slots, Tmax, latOn ? U : (P.segFrames > 0 ? P.poolArenas : 0));
    if (maxPath < 0) maxPath = 0;
    const VitArgs A = fill_vit_args(d, P, env, score, nframes, U, Tmax, nDist, maxPath, want_paths != 0, st);
    if (env.segVerbose) fprintf(stderr, "[dsr viterbi] %d utterances on %d workgroups: %s, %s state table\n", U, P.slots, P.segFrames > 0 ? (P.segQueues == 8 ? "time-sliced, XCD-bound queues" : "time-sliced, one queue") : "run to completion", P.narrow ? "narrow" : "wide");
    const TraceArgs TA = fill_trace_args(d, A);
    order_behind_last_traceback(P.slots, st);
    viterbi_launch(P.modes, A, P.slots, P.ldsBytes, st);
    traceback_launch(TA, st);                                             // the best paths, from the heads the decode leaves: directly behind it, before the copies
    publish_traceback(d, st);
    enqueue_result_copies(d, U, want_paths ? (size_t) U * maxPath : 0, st);
    d->pendingSlots = P.slots; d->pendingProf = A.D.prof;
  });
}

// DSR_VITERBI_PROF: the per-phase ticks of the last launch, summed over its slots
static void report_profile(const long long* prof, int slots)
{
  std::vector<long long> hp((size_t) slots * kProfN); DSR_HIP(hipMemcpy(hp.data(), prof, hp.size() * sizeof(long long), hipMemcpyDeviceToHost));
  double acc[32] = {0}; for (int s2 = 0; s2 < slots; s2++) for (int i = 0; i < 32; i++) acc[i] += (double) hp[(size_t) s2 * kProfN + i];
  fprintf(stderr, "[dsr viterbi prof] mean us per slot:");
  for (int i = 0; i < 32; i++) if (i != 15) fprintf(stderr, " p%d=%.0f", i, acc[i] / slots / 100.0);
  fprintf(stderr, "\n");
  double tmin = 1e30, tmax = 0.0, tsum = 0.0;                   // busy time per slot: how even the slots' shares of the batch were
  for (int s2 = 0; s2 < slots; s2++) { double t = 0.0; for (int i = 0; i < 32; i++) if (i != 15) t += (double) hp[(size_t) s2 * kProfN + i]; t /= 100.0; tsum += t; if (t < tmin) tmin = t; if (t > tmax) tmax = t; }
  {                                                             // frames by size class: share of the frames, share of their time, us per frame, ns per placement
    double h[12] = {0}; for (int s2 = 0; s2 < slots; s2++) for (int i = 0; i < 12; i++) h[i] += (double) hp[(size_t) s2 * kProfN + 32 + i];
    const double nf = h[0] + h[1] + h[2] + h[3], tk = h[4] + h[5] + h[6] + h[7];
    static const char* const cn[4] = {"<=8192", "<=12288", ">12288", "memory path"};
    for (int c = 0; c < 4; c++) if (h[c] > 0) fprintf(stderr, "[dsr viterbi prof] frames with %s placements: %.1f %% of the frames, %.1f %% of the frame time, %.1f us per frame, %.2f ns per placement\n",
                                                      cn[c], 100.0 * h[c] / nf, 100.0 * h[4 + c] / tk, h[4 + c] / 100.0 / h[c], h[4 + c] * 10.0 / h[8 + c]);
  }
  {                                                             // register-path frames: laid out by the frame before, or through P1 and P2
    double a = 0, b = 0; for (int s2 = 0; s2 < slots; s2++) { a += (double) hp[(size_t) s2 * kProfN + 44]; b += (double) hp[(size_t) s2 * kProfN + 45]; }
    if (a + b > 0) fprintf(stderr, "[dsr viterbi prof] register-path frames: %.1f %% start laid out, %.1f %% run P1/P2\n", 100.0 * a / (a + b), 100.0 * b / (a + b));
    double m1 = 0, m2 = 0, mAll = 0; for (int s2 = 0; s2 < slots; s2++) { m1 += (double) hp[(size_t) s2 * kProfN + 46]; m2 += (double) hp[(size_t) s2 * kProfN + 47]; mAll += (double) hp[(size_t) s2 * kProfN + 32 + 3]; }
    if (mAll > 0) fprintf(stderr, "[dsr viterbi prof] memory-path frames: %.0f, of them %.1f %% with at most 28672 placements, %.1f %% with at most 32767\n", mAll, 100.0 * m1 / mAll, 100.0 * m2 / mAll);
  }
  {                                                             // the epsilon hops behind the first (tick p31), per wave and placement of P3 (k_viterbi: s_hop)
    double h[6] = {0}; for (int s2 = 0; s2 < slots; s2++) for (int i = 0; i < 6; i++) h[i] += (double) hp[(size_t) s2 * kProfN + 48 + i];
    if (h[0] > 0) fprintf(stderr, "[dsr viterbi prof] hops behind the first: %.0f wave-placements, %.1f %% with a path of two or more hops, %.1f %% load hop costs, %.1f %% run the hop loop; "
                                  "%.3f hop iterations per wave-placement for %.3f hops per lane (x 64: %.2f)\n",
                          h[0], 100.0 * h[1] / h[0], 100.0 * h[2] / h[0], 100.0 * h[3] / h[0], h[4] / h[0], h[5] / h[0] / 64.0, h[5] / h[0]);
  }
  fprintf(stderr, "[dsr viterbi prof] busy us per slot: mean %.0f min %.0f max %.0f\n", tsum / slots, tmin, tmax);
  if (slots >= 64 && slots % 8 == 0) {                       // by XCD (workgroup i runs on XCD i mod 8): how even the eight queues of the time-sliced decode come out
    double bx[8] = {0}; for (int s2 = 0; s2 < slots; s2++) { double t = 0.0; for (int i = 0; i < 32; i++) if (i != 15) t += (double) hp[(size_t) s2 * kProfN + i]; bx[s2 & 7] += t / 100.0; }
    fprintf(stderr, "[dsr viterbi prof] busy us per slot, by XCD:"); for (int q = 0; q < 8; q++) fprintf(stderr, " %.0f", bx[q] / (slots / 8)); fprintf(stderr, "\n");
  }
}

dsr_status dsr_decoder_decode_collect(dsr_decoder* d, dsr_decode_result* res, int32_t* arcs_out, uint32_t* words_out)
{
  return guard([&] {
    if (!d || !res) throw Error(DSR_E_PARAMETER, "null argument");
    if (d->pendingU <= 0) throw Error(DSR_E_CONSISTENCY, "no decode in flight");
    const int U = d->pendingU; const size_t nPath = d->pendingPath; const int slots = d->pendingSlots; long long* prof = d->pendingProf;
    d->pendingU = 0; d->lastU = U; d->lastPaths = nPath > 0; d->lastMaxPath = nPath > 0 ? nPath / (size_t) U : 0;
    DSR_HIP(hipEventSynchronize(d->evDone));
    memcpy(res, d->h_res.p, sizeof(dsr_decode_result) * U);
    if (arcs_out && nPath) memcpy(arcs_out, d->h_arcs.p, sizeof(int) * nPath);
    if (words_out && nPath) memcpy(words_out, d->h_words.p, sizeof(unsigned) * nPath);
    if (read_vit_env().segVerbose && d->d_poolNext.p && d->lastPoolCap > 0) {
      unsigned long long used = 0; DSR_HIP(hipMemcpy(&used, d->d_poolNext.p, sizeof(used), hipMemcpyDeviceToHost));
      fprintf(stderr, "[dsr viterbi] pool of back-pointer records: %.1f M of %.1f M taken\n", used / 1e6, d->lastPoolCap / 1e6);
    }
    if (read_vit_env().segVerbose) {                            // which path the frames of the batch took (utterances decoded to their end; DSR_E_DIMENSION: only the path did not fit)
      long long laid = 0, reg = 0, all = 0;
      for (int u = 0; u < U; u++) if (res[u].status == DSR_OK || res[u].status == DSR_E_DIMENSION) { laid += res[u].laidOutFrames_; reg += res[u].registerFrames; all += res[u].frames + 1; }
      fprintf(stderr, "[dsr viterbi] frames: %lld laid out by the frame before, %lld through P1/P2, %lld on the memory path\n", laid, reg - laid, all - reg);
    }
    if (prof) report_profile(prof, slots);
    if (d->dumpOn) {
      long cnt[2]; DSR_HIP(hipMemcpy(cnt, d->d_dumpCount.p, sizeof(cnt), hipMemcpyDeviceToHost));
      const long N = cnt[0] < d->dumpCap ? cnt[0] : d->dumpCap; d->h_dumpFrames = cnt[1];
      std::vector<long> fo(cnt[1] + 1); if (cnt[1] > 0) DSR_HIP(hipMemcpy(fo.data(), d->d_dumpFrameOff.p, sizeof(long) * (cnt[1] + 1), hipMemcpyDeviceToHost));
      d->h_dumpFrameOff.assign(fo.begin(), fo.end());
      d->h_dumpNode.resize(N); d->h_dumpArc.resize(N); d->h_dumpAc.resize(N); d->h_dumpLm.resize(N);
      if (N > 0) {
        DSR_HIP(hipMemcpy(d->h_dumpNode.data(), d->d_dumpNode.p, sizeof(int) * N, hipMemcpyDeviceToHost));
        DSR_HIP(hipMemcpy(d->h_dumpArc.data(), d->d_dumpArc.p, sizeof(int) * N, hipMemcpyDeviceToHost));
        DSR_HIP(hipMemcpy(d->h_dumpAc.data(), d->d_dumpAc.p, sizeof(float) * N, hipMemcpyDeviceToHost));
        DSR_HIP(hipMemcpy(d->h_dumpLm.data(), d->d_dumpLm.p, sizeof(float) * N, hipMemcpyDeviceToHost));
      }
    }
  });
}

dsr_status dsr_decoder_decode_batch(dsr_decoder* d, const float* score, const int32_t* nframes, int U, int Tmax, int nDist,
                                    dsr_decode_result* res, int32_t* arcs_out, uint32_t* words_out, int maxPath, void* stream)
{
  if (!res) return guard([&] { throw Error(DSR_E_PARAMETER, "null argument"); });
  if (U <= 0) return DSR_OK;
  const dsr_status s1 = dsr_decoder_decode_launch(d, score, nframes, U, Tmax, nDist, maxPath, (arcs_out || words_out) ? 1 : 0, stream);
  if (s1 != DSR_OK) return s1;
  return dsr_decoder_decode_collect(d, res, arcs_out, words_out);
}

// _Decoder::lattice() (decoder.h:805-860) for utterance u of the last decode (cfg.latticeTokens > 0)
// the placement log of utterance u of the last lattice-mode decode, copied to the host
namespace {
struct LatHost {
  std::vector<long> frameOff; std::vector<dsr::LatPlace> place; std::vector<double> ttl; std::vector<dsr::LatBp> arena; std::vector<int> arenaLat; std::vector<dsr::LatFinalTok> fin;
  dsr::LatInput in;
};
void load_lat(dsr_decoder* d, int u, uint32_t eosX, LatHost& H)
{
  if (d->latU <= 0) throw Error(DSR_E_CONSISTENCY, "Must enable lattice generation during decoding.");                 // decoder.h:807-808
  if (d->pendingU > 0) throw Error(DSR_E_CONSISTENCY, "a decode is in flight: collect it first");
  if (u < 0 || u >= d->latU) throw Error(DSR_E_INDEX, "utterance %d of %d", u, d->latU);
  int info[4]; DSR_HIP(hipMemcpy(info, d->d_latInfo.p + 4 * (size_t) u, sizeof(info), hipMemcpyDeviceToHost));
  const int finN = info[0], haveNext = info[1], T = info[3]; const long arenaN = info[2];
  if (T <= 0) throw Error(DSR_E_CONSISTENCY, "utterance %d was not decoded to its end (status of its decode result)", u);
  H.frameOff.assign((size_t) T + 2, 0);
  DSR_HIP(hipMemcpy(H.frameOff.data(), d->d_latFrameOff.p + (size_t) u * (d->latTmax + 3), sizeof(long) * ((size_t) T + 2), hipMemcpyDeviceToHost));
  const long nP = H.frameOff[(size_t) T + 1];
  H.place.resize((size_t) (nP > 0 ? nP : 1)); H.ttl.resize((size_t) (nP > 0 ? nP : 1));
  H.arena.resize((size_t) (arenaN > 0 ? arenaN : 1)); H.arenaLat.resize((size_t) (arenaN > 0 ? arenaN : 1)); H.fin.resize((size_t) (finN > 0 ? finN : 1));
  const size_t cap = (size_t) d->cfg.latticeTokens;
  if (nP > 0) { DSR_HIP(hipMemcpy(H.place.data(), d->d_lat.p + (size_t) u * cap, sizeof(LatPlace) * (size_t) nP, hipMemcpyDeviceToHost));
                DSR_HIP(hipMemcpy(H.ttl.data(), d->d_latTtl.p + (size_t) u * cap, sizeof(double) * (size_t) nP, hipMemcpyDeviceToHost)); }
  if (arenaN > 0) { DSR_HIP(hipMemcpy(H.arena.data(), d->d_arena.p + (size_t) u * (size_t) d->latArenaCap, sizeof(LatBp) * (size_t) arenaN, hipMemcpyDeviceToHost));
                    DSR_HIP(hipMemcpy(H.arenaLat.data(), d->d_arenaLat.p + (size_t) u * (size_t) d->latArenaCap, sizeof(int) * (size_t) arenaN, hipMemcpyDeviceToHost)); }
  if (finN > 0) DSR_HIP(hipMemcpy(H.fin.data(), d->d_latFinal.p + (size_t) u * d->cfg.maxActive, sizeof(LatFinalTok) * (size_t) finN, hipMemcpyDeviceToHost));
  LatInput& in = H.in; in.graph = &d->graphCopy; in.csr = &d->csr; in.tab = &d->tab; in.lmScale = d->cfg.lmScale; in.lmPenalty = d->cfg.lmPenalty; in.silPenalty = d->cfg.silPenalty;
  in.silenceX = d->cfg.silenceX; in.eosX = eosX; in.T = T; in.place = H.place.data(); in.ttl = H.ttl.data(); in.frameOff = H.frameOff.data();
  in.arena = H.arena.data(); in.arenaLat = H.arenaLat.data(); in.arenaN = arenaN; in.fin = H.fin.data(); in.finN = finN; in.haveNext = haveNext;
}
}  // namespace

dsr_status dsr_decoder_lattice(dsr_decoder* d, int u, uint32_t eosX, dsr_lattice** out)
{
  return guard([&] {
    if (!d || !out) throw Error(DSR_E_PARAMETER, "null argument");
    LatHost H; load_lat(d, u, eosX, H);
    dsr_lattice* L = new dsr_lattice();
    try { build_lattice(H.in, *L); } catch (...) { delete L; throw; }
    *out = L;
  });
}

// _Decoder::writeGMM(conv, channel, spk, utt, cfrom, score, fileName, frameInterval) (decoder.h:1018-1102; decoder.i:177-178): the 1-best path as
// runs of equal input symbols -- "# utt cfrom score", then per run "conv channel start duration label score", first run first, the end-of-sentence
// label skipped.  The walk needs every token of the best path with its frame and scores: the decoder must have run with lattice bookkeeping
// (latticeTokens > 0, the reference's generateLattice) and symbols set (dsr_decoder_set_symbols: labels come from the input lexicon, :1066).
// fileName "" or NULL: stdout; files are appended to (:1023).  (spk is accepted and unused, as in the reference.)
dsr_status dsr_decoder_write_gmm(dsr_decoder* d, int u, const char* conv, const char* channel, const char* spk, const char* utt, double cfrom, double score,
                                 const char* fileName, double frameInterval)
{
  return guard([&] {
    (void) spk;
    if (!d || !conv || !channel || !utt) throw Error(DSR_E_PARAMETER, "null argument");
    if (!d->lexIn) throw Error(DSR_E_KEY, "the transducer set on this decoder has no input lexicon");
    LatHost H; load_lat(d, u, 0u, H);
    std::vector<GmmRow> rows;
    if (!best_path_gmm(H.in, rows)) throw Error(DSR_E_CONSISTENCY, "no best token");       // (the reference dereferences a null token here)
    FILE* fp = (!fileName || !*fileName) ? stdout : fopen(fileName, "a");
    if (!fp) throw Error(DSR_E_IO, "could not open %s", fileName);
    fprintf(fp, "# %s %10.4f %10.4f\n", utt, cfrom, score);
    for (int i = (int) rows.size() - 1; i >= 0; i--) {
      if (rows[i].inX >= d->lexIn->syms.size()) { if (fp != stdout) fclose(fp); throw Error(DSR_E_INDEX, "input symbol %u is not in the lexicon", rows[i].inX); }
      const std::string& lab = d->lexIn->symbol(rows[i].inX); const char* label = lab.c_str();
      if (lab == d->eosSymbol) continue;
      const double beg = cfrom + rows[i].startX * frameInterval, len = (rows[i].endX - rows[i].startX + 1) * frameInterval;
      fprintf(fp, "%s %s %7.2f %7.2f %-20s %7.2f\n", conv, channel, beg, len, label, rows[i].score);
    }
    if (fp != stdout) fclose(fp); else fflush(stdout);
  });
}
void dsr_lattice_destroy(dsr_lattice* L) { delete L; }
int dsr_lattice_num_nodes(const dsr_lattice* L) { return L ? (int) L->nodeFinal.size() : 0; }
int dsr_lattice_num_edges(const dsr_lattice* L) { return L ? (int) L->from.size() : 0; }
int dsr_lattice_final_states_n(const dsr_lattice* L) { return L ? L->finalStatesN : 0; }
dsr_status dsr_lattice_get(const dsr_lattice* L, int32_t* nodeFinal, int32_t* from, int32_t* to, uint32_t* in, uint32_t* out, int32_t* start, int32_t* end, double* ac, double* lm)
{
  return guard([&] {
    if (!L) throw Error(DSR_E_PARAMETER, "null argument");
    const size_t nE = L->from.size();
    if (nodeFinal) memcpy(nodeFinal, L->nodeFinal.data(), 4 * L->nodeFinal.size());
    if (from && nE) memcpy(from, L->from.data(), 4 * nE); if (to && nE) memcpy(to, L->to.data(), 4 * nE);
    if (in && nE) memcpy(in, L->in.data(), 4 * nE); if (out && nE) memcpy(out, L->out.data(), 4 * nE);
    if (start && nE) memcpy(start, L->start.data(), 4 * nE); if (end && nE) memcpy(end, L->end.data(), 4 * nE);
    if (ac && nE) memcpy(ac, L->ac.data(), 8 * nE); if (lm && nE) memcpy(lm, L->lm.data(), 8 * nE);
  });
}
dsr_status dsr_lattice_write(dsr_lattice* L, const char* fileName, int writeData)
{ return guard([&] { if (!L || !fileName) throw Error(DSR_E_PARAMETER, "null argument"); L->write(fileName, writeData != 0); }); }
size_t dsr_lattice_pack_size(const dsr_lattice* L) { return L ? 16 + 4 * L->nodeFinal.size() + 40 * L->from.size() : 0; }
dsr_status dsr_lattice_pack(const dsr_lattice* L, void* buf, size_t bufBytes)
{
  return guard([&] {
    if (!L || !buf) throw Error(DSR_E_PARAMETER, "null argument");
    const std::vector<unsigned char> b = L->pack();
    if (b.size() > bufBytes) throw Error(DSR_E_DIMENSION, "buffer holds %zu bytes, the lattice needs %zu", bufBytes, b.size());
    memcpy(buf, b.data(), b.size());
  });
}
dsr_status dsr_lattice_unpack(const void* buf, size_t bytes, dsr_lattice** out)
{
  return guard([&] {
    if (!buf || !out) throw Error(DSR_E_PARAMETER, "null argument");
    dsr_lattice* L = new dsr_lattice();
    try { static_cast<LatticeData&>(*L) = LatticeData::unpack((const unsigned char*) buf, bytes); } catch (...) { delete L; throw; }
    *out = L;
  });
}

dsr_status dsr_decoder_get_dump(dsr_decoder* d, int64_t* nFrames, const int64_t** frameOff, const int32_t** node,
                                const float** ac, const float** lm, const int32_t** arc)
{
  return guard([&] {
    if (!d) throw Error(DSR_E_PARAMETER, "null argument");
    if (nFrames) *nFrames = d->h_dumpFrames;
    if (frameOff) *frameOff = d->h_dumpFrameOff.data();
    if (node) *node = d->h_dumpNode.data(); if (arc) *arc = d->h_dumpArc.data();
    if (ac) *ac = d->h_dumpAc.data(); if (lm) *lm = d->h_dumpLm.data();
  });
}

}  // extern "C"
