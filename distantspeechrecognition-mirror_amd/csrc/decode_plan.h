// csrc/decode_plan.h -- every launch decision of the Viterbi decode (decoder.cpp, dsr_decoder_decode_launch), taken in one pure function that can be
// asked without a device, and the decoder's environment switches.  Plain C++17: nothing of HIP in here.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>

namespace dsr {

// The decoder's switches (DSR_VITERBI_<NAME>), read by read_vit_env() and nowhere else.
struct VitEnv {
  int slots = 0;             // SLOTS: workgroups of a decoder created with cfg.streams <= 0 (default: one per CU)
  bool noFast = false;       // NOFAST: every frame takes the memory path
  int seg = 125;             // SEG: frames per segment of the time-sliced decode (0: run every utterance to completion)
  double segSaveGB = 16.0;   // SEG_SAVE_GB: largest save area (token lists of utterances between their segments) time slicing may take
  int segAny = 0;            // SEG_ANY: set = slice on one queue where the XCD-bound queues cannot be used; 2 = one queue always
  int segDrop = 0;           // SEG_DROP (tests): bit x set = the workgroups on XCD x do not serve their own queue
  bool segVerbose = false;   // SEG_VERBOSE: print the launch's plan and the use of the back-pointer pool to stderr
  bool pen = false;          // PEN: keep the penalty arithmetic of the expansion even where it is provably a no-op
  bool prof = false;         // PROF: per-phase ticks (the profiling instantiations) and their report at collect
  bool noHash = false;       // NOHASH: no LDS state table (recombination through memory)
  bool noCnt = false;        // NOCNT: no expansion counts in LDS
  bool tableWide = false;    // TABLE=wide: the two-array state table whatever the graph
};

inline VitEnv read_vit_env()
{
  VitEnv e; const char* v;
  if ((v = getenv("DSR_VITERBI_SLOTS"))) e.slots = atoi(v);
  e.noFast = getenv("DSR_VITERBI_NOFAST") != nullptr;
  if ((v = getenv("DSR_VITERBI_SEG"))) e.seg = atoi(v);
  if ((v = getenv("DSR_VITERBI_SEG_SAVE_GB"))) e.segSaveGB = atof(v);
  if ((v = getenv("DSR_VITERBI_SEG_ANY"))) e.segAny = atoi(v) == 2 ? 2 : 1;
  if ((v = getenv("DSR_VITERBI_SEG_DROP"))) e.segDrop = (int) strtol(v, nullptr, 0);
  e.segVerbose = getenv("DSR_VITERBI_SEG_VERBOSE") != nullptr;
  e.pen = getenv("DSR_VITERBI_PEN") != nullptr;
  e.prof = getenv("DSR_VITERBI_PROF") != nullptr;
  e.noHash = getenv("DSR_VITERBI_NOHASH") != nullptr;
  e.noCnt = getenv("DSR_VITERBI_NOCNT") != nullptr;
  e.tableWide = (v = getenv("DSR_VITERBI_TABLE")) && !strcmp(v, "wide");
  return e;
}

// what the plan is decided from: the configuration, the graph, the batch, and the static LDS of the instantiation plan_base_modes() names
struct PlanIn {
  int streams, maxActive; long long arenaTokens, latticeTokens; int topN; bool dumpOn;
  int nNodes, maxCnt;                 // states of the graph; its largest number of expansion records per state
  int U, Tmax, nDist;
  size_t staticLds;
};

struct DecodePlan {
  int slots, segFrames, segQueues, segCount, poolArenas; long arenaPer; int useLdsRow, hashN, cntCap, modes; size_t ldsBytes; bool narrow;
};

static constexpr size_t kPlanSideBytes = (size_t) 496 * 32;      // kSideLds side records (viterbi.h)

// instantiation without the table bit: bit 0 per-phase ticks, bit 1 lattice bookkeeping / topN / token dump compiled in (the static LDS does not depend on bit 2)
inline int plan_base_modes(const PlanIn& in, const VitEnv& env) { return (env.prof ? 1 : 0) | ((in.latticeTokens > 0 || in.topN > 0 || in.dumpOn) ? 2 : 0); }

// roundRobin(): does this device deal the workgroups of a grid out round robin over 8 XCDs -- asked only when the answer decides something
template <class RoundRobin> DecodePlan plan_decode(const PlanIn& in, const VitEnv& env, RoundRobin&& roundRobin)
{
  DecodePlan p;
  const int U = in.U, Tmax = in.Tmax, nDist = in.nDist;
  int slots = in.streams; if (slots > U) slots = U; if (in.dumpOn) slots = 1;
  const bool latOn = in.latticeTokens > 0;
  // Time slicing (DecDev): when there are more utterances than workgroups, in the plain decode mode.
  int segFrames = 0;
  if (!latOn && !in.dumpOn && in.topN <= 0 && U > slots) {
    segFrames = env.seg;
    if (segFrames < 0 || 2 * segFrames > Tmax + 1) segFrames = 0;
    // between its segments an utterance's token list waits in a save area of maxActive tokens: with very large lists and very many utterances that is more memory
    // than the scheduling is worth
    const double saveGB = (double) U * (double) in.maxActive * 24.0 / 1e9;
    if (saveGB > env.segSaveGB) segFrames = 0;
  }
  // XCD-bound queues (the cheap hand-over) need workgroups on every XCD: grids of 8 k >= 64 workgroups on a device that deals workgroups out round robin.
  // Anything else decodes every utterance in one go -- unless SEG_ANY asks for the one-queue form (device-scope fences at every hand-over: the tests).
  int segQueues = 8;
  if (segFrames > 0 && !(slots >= 64 && slots % 8 == 0 && roundRobin())) { if (env.segAny) segQueues = 1; else segFrames = 0; }
  if (segFrames > 0 && env.segAny == 2) segQueues = 1;
  // (sliced: one pool of back-pointer records for the batch instead of an arena per slot -- 1536 records per utterance and frame on average, at least what the slots had)
  const long arenaPer = in.arenaTokens > 0 ? (long) in.arenaTokens : (long) 8192 * (long) (Tmax + 2);
  int poolArenas = 0;
  if (segFrames > 0) {
    const double want = (double) U * 1536.0 * (double) (Tmax + 2) / (double) arenaPer;
    poolArenas = (int) std::min<double>(std::ceil(want), (double) (0xFFFFFFF0u / (unsigned long long) arenaPer));
    if ((unsigned long long) std::max(poolArenas, slots) * (unsigned long long) arenaPer > 0xFFFFFFF0ull) segFrames = 0;      // back pointers are 32-bit pool indices
  }
  p.slots = slots; p.segFrames = segFrames; p.segQueues = segQueues; p.poolArenas = poolArenas; p.arenaPer = arenaPer;
  p.segCount = segFrames > 0 ? (Tmax + segFrames) / segFrames : 1;            // segments cover frames 0 .. Tmax (the end expansion is "frame" T)
  // LDS: [score row][state table: 2 x hashN words][later arrivals' side records][expansion counts]; the row stays in global memory
  // when it would push the state table below the size the register path needs.  One 1024-thread workgroup per CU.  The table's 2 x hashN words are
  // hashN = 16 384 two-word buckets (wide: key array + first-arrival array) or, for graphs of at most 65 535 states, 32 768 one-word buckets
  // (narrow: flag | key or side record | slot) -- the formula below gives the same number of bytes for both, 128 KB at hashN = 16 384.
  int modes = plan_base_modes(in, env);
  const size_t eoffB = kPlanSideBytes; const size_t ldsCap = (size_t) 160 * 1024 - in.staticLds;      // what the kernel's static LDS leaves of a CU's 160 KB
  const int hashMax = 16384;
  int useLds = (size_t) nDist * sizeof(float) <= 64 * 1024;
  if (useLds && (size_t) ((nDist + 3) & ~3) * sizeof(float) + (size_t) hashMax * 8 + eoffB > ldsCap) useLds = 0;
  const size_t rowB = useLds ? (size_t) ((nDist + 3) & ~3) * sizeof(float) : 16;
  int hashN = hashMax; while (hashN > 0 && rowB + (size_t) hashN * 8 + eoffB > ldsCap) hashN >>= 1;
  if (env.noHash) hashN = 0;
  // + the expansion counts of up to 2048 tokens (u16) when the budget and the graph's largest fan-out allow
  int cntCap = (hashN > 0 && in.maxCnt < 65536 && rowB + (size_t) hashN * 8 + eoffB + 4096 <= ldsCap) ? 2048 : 0;
  if (env.noCnt) cntCap = 0;
  p.ldsBytes = rowB + (size_t) hashN * 8 + eoffB + 2 * (size_t) cntCap;
  // narrow table: the key field holds state + 1 in 16 bits, the slot field 15 bits = the 24 576 placements 32 768 buckets take at a load of 0.75
  // (TABLE=wide: the two-array table whatever the graph -- A/B runs and the tests)
  p.narrow = in.nNodes <= 65535 && hashN == hashMax && !env.tableWide;
  if (p.narrow) modes |= 4;
  p.useLdsRow = useLds; p.hashN = hashN; p.cntCap = cntCap; p.modes = modes;
  return p;
}

}  // namespace dsr
