// csrc/k_traceback.hip -- the best path of every utterance of a decode (bestHypo, asr/decoder/decoder.h:748-773), from the trace heads k_viterbi leaves.
//
// Following the back pointers is one dependent 8-byte load per frame of the path: a thousand memory latencies in a row that need no LDS table, no barrier
// of 1024 threads and a handful of registers.  Inside k_viterbi that wait held a whole CU (a decode workgroup fills one); here it is one wave per utterance,
// grid = U, with no LDS at all, and the chains of a batch are followed side by side.
//
// The kernel is launched directly behind k_viterbi on its stream.  The kernel boundary is the only synchronisation there is: every back-pointer record,
// result record and head was written by a kernel that has ended, so all loads are plain ones -- also for the pool of a time-sliced batch, whose records
// were written on several CUs of an XCD.  It does NOT fit beside a decode: k_viterbi's workgroups take the registers and the LDS of their CUs whole, so a
// decode that another stream has queued must not move in before this kernel has run (decoder.cpp, order_behind_last_traceback).
//
// Where the records do not outlive their utterance (a decode run to completion: its workgroups take utterances from a queue, and a slot's arena is its next
// utterance's too) k_viterbi has followed the chain already and the head says how many hops wait in the hop scratch.
//
// Per utterance: lane 0 follows `prev` from the head and stores the hop records (newest first); the wave then counts the arcs of every hop -- an end record
// (kEndBit) stands for its epsilon path into the final state, an expansion record for its emitting arc and the epsilon path behind it --, places them with a
// prefix sum (arcsOut is in time order, cut at maxPath), counts the arcs with an output symbol, and writes the word sequence of the arc list with a second
// prefix sum.  Utterances whose head is empty (no best token, or a failed decode) are left as k_viterbi wrote them.
#include "launch.h"
#include "viterbi.h"

namespace dsr {

static constexpr uint32_t kNone = 0xFFFFFFFFu;
static constexpr uint32_t kEndBit = 0x80000000u;
static constexpr int kTraceThreads = 64;

// inclusive prefix sum over the wave (DPP row shifts and row broadcasts, as in k_viterbi)
__device__ __forceinline__ int trace_incl_scan(int v)
{
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);      // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);      // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);      // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);      // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);     // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);     // row_bcast:31 -> rows 2, 3
  return v;
}

__global__ __launch_bounds__(kTraceThreads) void k_traceback(const TraceArgs A)
{
  const int u = blockIdx.x, lane = threadIdx.x;
  if (u >= A.U) return;
  const TraceHead hd = A.heads[u];
  if (hd.bp == kNone) return;                                                  // (uniform: the whole wave leaves)
  int* const hopRec = A.hopRec + (size_t) u * A.hopStride; int* const hopOff = A.hopOff + (size_t) u * A.hopStride;
  // the walk stops where k_viterbi's did (hopCap records) and never leaves the hop scratch or the arena.  The scratch holds hopStride = min(hopCap, Tmax + 2)
  // hops and no status marks a chain cut there: a frame adds one record to a chain and the end expansion at most one (it replaces the token's record when it
  // takes no arc), so a chain has at most T + 1 <= Tmax + 1 of them.  A decoder that adds records per frame must size the scratch anew.
  const int walkCap = A.hopCap < A.hopStride ? A.hopCap : A.hopStride;
  int nHw = 0;
  if (hd.hops != kNone) nHw = (int) hd.hops;                                   // k_viterbi followed the chain itself: the records were its slot's next utterance's to overwrite
  else if (lane == 0) {
    const Bp* const arena = A.arena + hd.arenaOff; const unsigned long long arenaN = A.arenaN > hd.arenaOff ? A.arenaN - hd.arenaOff : 0ull;
    for (uint32_t bq = hd.bp; bq != kNone && nHw < walkCap && bq < arenaN; ) {
      const uint2 e = *reinterpret_cast<const uint2*>(&arena[bq]);
      hopRec[nHw++] = (int) e.y; bq = e.x;
    }
  }
  if (nHw > walkCap) nHw = walkCap;
  const int nH = __builtin_amdgcn_readfirstlane(nHw);
  __syncthreads();                                                             // lane 0's hop records are in memory before the wave reads them
  int nA = 0;
  for (int b0 = 0; b0 < nH; b0 += kTraceThreads) {                              // arcs per hop; hopOff = arcs of the hops walked before (= later in time)
    const int i = b0 + lane; int len = 0;
    if (i < nH) { const uint32_t rc = (uint32_t) hopRec[i]; len = (rc & kEndBit) ? A.erec[rc & ~kEndBit].pathLen : (int) (A.xrec[rc].meta & 0xFFFFu) + 1; }
    const int incl = trace_incl_scan(len);
    if (i < nH) hopOff[i] = nA + incl - len;
    nA += __builtin_amdgcn_readlane(incl, 63);
  }
  const int maxPath = A.maxPath;
  int* const ao = A.arcsOut ? A.arcsOut + (size_t) u * maxPath : nullptr;
  int nWloc = 0;
  for (int i = lane; i < nH; i += kTraceThreads) {                              // every hop writes its arcs, first..last
    const uint32_t rc = (uint32_t) hopRec[i]; int pos = nA - hopOff[i];
    if (rc & kEndBit) {
      const ERec e = A.erec[rc & ~kEndBit];
      for (int h = e.pathLen - 1; h >= 0; h--) { const int a = A.path[e.pathOff + h]; pos--; if (ao && pos < maxPath) ao[pos] = a; if (A.arcOut[a] != 0) nWloc++; }
    } else {
      const int a = A.xarc[rc]; pos--; if (ao && pos < maxPath) ao[pos] = a; if (A.arcOut[a] != 0) nWloc++;
      const int pl = (int) (A.xrec[rc].meta & 0xFFFFu); const int po = A.xpathOff[rc];
      for (int h = pl - 1; h >= 0; h--) { const int a2 = A.path[po + h]; pos--; if (ao && pos < maxPath) ao[pos] = a2; if (A.arcOut[a2] != 0) nWloc++; }
    }
  }
  const int nW = __builtin_amdgcn_readlane(trace_incl_scan(nWloc), 63);
  __syncthreads();                                                             // the arc list is complete before it is read back
  if (A.wordsOut && ao) {                                                      // the words of the arc list, in order
    unsigned* const wo = A.wordsOut + (size_t) u * maxPath; int q = 0;
    const int lim = nA < maxPath ? nA : maxPath;
    for (int b0 = 0; b0 < lim; b0 += kTraceThreads) {
      const int i = b0 + lane; unsigned o = 0u;
      if (i < lim) o = A.arcOut[ao[i]];
      const int v = o != 0u ? 1 : 0, incl = trace_incl_scan(v);
      if (o != 0u && q + incl - v < maxPath) wo[q + incl - v] = o;
      q += __builtin_amdgcn_readlane(incl, 63);
    }
  }
  if (lane == 0) {
    dsr_decode_result& r = A.res[u];
    if (r.status == DSR_OK) {
      r.nArcs = nA; r.nWords = nW;
      if (nH >= A.hopCap) r.status = DSR_E_ALLOCATION; else if (nA > maxPath && A.arcsOut) r.status = DSR_E_DIMENSION;
    }
  }
}

void traceback_launch(const TraceArgs& A, hipStream_t st)
{
  if (A.U <= 0) return;
  launch(k_traceback, dim3(A.U), dim3(kTraceThreads), 0, st, A);
}

}  // namespace dsr
