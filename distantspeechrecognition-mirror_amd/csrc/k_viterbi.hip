// csrc/k_viterbi.hip -- time-synchronous Viterbi token passing over a static WFST, batched over
// utterances, bit-exact with the reference's sequential decoder.
//
// Replaces _Decoder::decode and everything under it (asr/decoder/decoder.h:488-737, 956-1015),
// the _TokenList hash/list (decoder.h:48-320) and _Token (asr/lattice/lattice.h:37-79) for DecoderFlyWeight
// (decoder.h:1127-1139); bestHypo (decoder.h:748-773) is k_traceback.hip, launched behind this kernel from the heads it leaves.
//
// What "bit-exact" needs and how it is kept in a parallel kernel:
//   * token scores live as two floats; every placement is computed in double from them and rounded on
//     construction; recombination compares the UNROUNDED double candidate with the incumbent's
//     float sum (decoder.h:519-528).  That fold is order dependent, so it is replayed literally:
//     every placement of a frame gets its arrival rank ("slot") = its position in the reference's
//     nested loops (token list order x arc order x depth-first epsilon recursion); the placements
//     of one destination state are folded in slot order by one thread.
//   * the next frame's list order is "last inserted first" (decoder.h:246-247, replacement keeps the
//     position): a state's position is decided by its FIRST arrival, so the new list is the
//     first-arrival candidates in reverse slot order -- a stream compaction, no sort.
//   * the beam uses the previous frame's best UNROUNDED emitting placement (decoder.h:521,566-588).
//   * epsilon arcs are expanded depth first without recombination (decoder.h:979-983); the graph's
//     expansion tables (wfst_graph.h) enumerate those paths in the reference's order, and the float
//     rounding of every intermediate epsilon token is reproduced when the path is walked.
// One workgroup (1024 threads) owns one utterance at a time and loops over its frames; workgroups pull
// utterances from a queue.  All arithmetic that decides a comparison is done with explicit
// non-contracted IEEE operations (this file is compiled with -ffp-contract=off).
#include "launch.h"
#include "viterbi.h"
#include <algorithm>
#include <cmath>
#include <type_traits>

namespace dsr {

// (the records, the argument block and the constants the host sizes its buffers by -- kThreads, kFastC, kProfN, kSideLds -- are in viterbi.h)
static constexpr uint32_t kNone = 0xFFFFFFFFu;
static constexpr uint32_t kEndBit = 0x80000000u;
static constexpr int kWaves = kThreads / 64;
static constexpr int kFastK = 8;
static constexpr int kB = 2;                        // placements whose loads are in flight together (batch of the register-path phases)                  // placements a thread keeps in registers on the register path
static constexpr int kFastE = 8190;                // most expanding tokens per frame on the register path
static constexpr int kP1 = 16;                     // token rounds per wave in the register path's beam pass
static constexpr int kW = 4;                        // register placements whose P6 loads are in flight together (8: 3 % slower; parked ones: kB)

typedef const __attribute__((address_space(4))) VitArgs* KP;

__device__ __forceinline__ unsigned ld_u32(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int ld_i32(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_u32(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_i32(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// What an utterance carries from one CU to another (time slicing) is READ with device-scope loads (past the reader's L1).  The utterance never leaves its XCD --
// every XCD has its own queue -- so the L2 both CUs share is the point of coherence and the writes stay plain (the L1 writes through).  Measured alternatives: release /
// acquire fences at device scope write back and invalidate a whole L2 per hand-over (0.1 ms each); write-through stores for the back-pointer records cost 2 % of the launch.
__device__ __forceinline__ void st_u64_dev(void* p, unsigned long long v) { __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long ld_u64_dev(const void* p) { return __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// inclusive prefix sum over the wave: four row shifts inside every 16-lane row, then the row totals are handed on
// (row_bcast:15 into rows 1 and 3, row_bcast:31 into rows 2 and 3) -- six DPP adds, no LDS round trips
__device__ __forceinline__ int wave_incl_scan(int v, int /*lane*/)
{
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);      // row_shr:1
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);      // row_shr:2
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);      // row_shr:4
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);      // row_shr:8
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);     // row_bcast:15 -> rows 1, 3
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);     // row_bcast:31 -> rows 2, 3
  return v;
}
// full-wave min / max by DPP row shifts and row broadcasts (as the scan above): vector-ALU speed, the result in lane 63, handed out as a uniform value.
// (__shfl_xor goes through the LDS crossbar: six dependent ds_bpermute round trips, ~0.3 us per reduction, twice that for a double)
__device__ __forceinline__ float wave_max_f_uni(float v)
{
#define DSR_DPP_F(ctrl, rm) { const float o = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), ctrl, rm, 0xF, false)); v = fmaxf(v, o); }
  DSR_DPP_F(0x111, 0xF) DSR_DPP_F(0x112, 0xF) DSR_DPP_F(0x114, 0xF) DSR_DPP_F(0x118, 0xF) DSR_DPP_F(0x142, 0xA) DSR_DPP_F(0x143, 0xC)
#undef DSR_DPP_F
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ double wave_min_d_uni(double v)
{
#define DSR_DPP_D(ctrl, rm) { const int lo = __double2loint(v), hi = __double2hiint(v); \
    const double o = __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, ctrl, rm, 0xF, false), __builtin_amdgcn_update_dpp(lo, lo, ctrl, rm, 0xF, false)); v = (o < v) ? o : v; }
  DSR_DPP_D(0x111, 0xF) DSR_DPP_D(0x112, 0xF) DSR_DPP_D(0x114, 0xF) DSR_DPP_D(0x118, 0xF) DSR_DPP_D(0x142, 0xA) DSR_DPP_D(0x143, 0xC)
#undef DSR_DPP_D
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), 63), __builtin_amdgcn_readlane(__double2loint(v), 63));
}
__device__ __forceinline__ double wave_min_d(double v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const double o = __shfl_xor(v, d, 64); v = (o < v) ? o : v; }
  return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64(unsigned long long v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { const unsigned long long o = __shfl_xor(v, d, 64); v = (o < v) ? o : v; }
  return v;
}
__device__ __forceinline__ float wave_max_f(float v)
{
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  return v;
}
// clears a result record with a zero the optimiser cannot see through: the constant {0, 0, 0} tuple of a memset otherwise lives from the kernel's
// first instruction to its last, in scratch memory, and its 96-bit reload is what trips the register-alignment bug mentioned below
__device__ __forceinline__ void clear_result(dsr_decode_result* r)
{
  int z = 0; asm volatile("" : "+v"(z));
  int* p = reinterpret_cast<int*>(r);
#pragma unroll 1
  for (int i = 0; i < (int) (sizeof(dsr_decode_result) / 4); i++) p[i] = z;
}
// LDS-typed views: "cond ? lds[i] : mem[i]" is compiled as a select of two generic pointers and ONE flat load -- a flat load pays the memory path's
// latency even when it hits LDS.  Reads through these types are ds_read instructions; the two cases are kept in separate branches (fence below).
typedef __attribute__((address_space(3))) float lds_float_t;
typedef __attribute__((address_space(3))) Side lds_side_t;
#define DSR_NO_MERGE() asm volatile("" ::: "memory")
// a whole token as one 16-byte load (three of its four fields used -> the compiler narrows the load to 96 bits: same bug as below)
__device__ __forceinline__ TokA ld_tok(const TokA* p)
{
  const unsigned long long a = reinterpret_cast<const volatile unsigned long long*>(p)[0], b = reinterpret_cast<const volatile unsigned long long*>(p)[1];
  TokA t; t.ac = __uint_as_float((unsigned) (a & 0xFFFFFFFFull)); t.lm = __uint_as_float((unsigned) (a >> 32)); t.bp = (uint32_t) (b & 0xFFFFFFFFull); t.xs = (uint32_t) (b >> 32);
  return t;
}
// a winner's {ac, lm, rec} out of a side record: an 8-byte and a 4-byte load on purpose -- as three adjacent fields the compiler merges them into one
// 96-bit load, and a 96-bit value that gets spilled trips a register-alignment bug of this compiler on gfx950 ("requires even aligned vector registers")
__device__ __forceinline__ void side_winner(const Side* sideL, const Side* side, int sideLds, int idx, float& ac, float& lm, int& rec)
{
  if (idx < sideLds) {
    const lds_side_t* p = (const lds_side_t*) sideL + idx;
    const unsigned long long a = *reinterpret_cast<const volatile __attribute__((address_space(3))) unsigned long long*>(&p->ac);
    rec = *reinterpret_cast<const volatile __attribute__((address_space(3))) int*>(&p->rec);
    ac = __uint_as_float((unsigned) (a & 0xFFFFFFFFull)); lm = __uint_as_float((unsigned) (a >> 32));
    DSR_NO_MERGE();
  } else {
    const Side* p = side + idx;
    const unsigned long long a = *reinterpret_cast<const volatile unsigned long long*>(&p->ac); rec = *reinterpret_cast<const volatile int*>(&p->rec);
    ac = __uint_as_float((unsigned) (a & 0xFFFFFFFFull)); lm = __uint_as_float((unsigned) (a >> 32));
  }
}
// {slot, unrounded total, next} and {next, total} of a side record
__device__ __forceinline__ void side_link(const Side* sideL, const Side* side, int sideLds, int idx, int& c, double& ttl, unsigned& next)
{
  if (idx < sideLds) { const lds_side_t* p = (const lds_side_t*) sideL + idx; c = p->c; ttl = p->ttl; next = p->next; DSR_NO_MERGE(); }
  else { const Side* p = side + idx; c = p->c; ttl = p->ttl; next = p->next; }
}
__device__ __forceinline__ float side_score(const Side* sideL, const Side* side, int sideLds, int idx)
{
  float r;
  if (idx < sideLds) { const lds_side_t* p = (const lds_side_t*) sideL + idx; r = __fadd_rn(p->ac, p->lm); DSR_NO_MERGE(); }
  else { const Side* p = side + idx; r = __fadd_rn(p->ac, p->lm); }
  return r;
}
// "uniform base + 32-bit byte offset": the address form the hardware adds for free (global_load v, v_off, s[base]); a 64-bit element index costs a
// sign extension, a 64-bit shift and a 64-bit add per access.  Callers guarantee index * sizeof < 2^32 (checked on the host: DecoderState::fastOK).
template <class T> __device__ __forceinline__ const T* at32(const void* base, uint32_t byteOff) { return reinterpret_cast<const T*>(reinterpret_cast<const char*>(base) + byteOff); }
template <class T> __device__ __forceinline__ T* at32w(void* base, uint32_t byteOff) { return reinterpret_cast<T*>(reinterpret_cast<char*>(base) + byteOff); }
// wave-uniform values computed from LDS land in vector registers; these move them to scalar ones
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uni(double v) { return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v))); }
__device__ __forceinline__ unsigned f2ord(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }

// One decoded utterance per loop iteration of a persistent workgroup.
//
// A frame runs on one of two paths that produce identical lists:
//   * the register path (frames with at most kFastC placements, 16 per thread): thread t owns the arrival slots t, t+nthr, ...
//     and keeps those placements in registers from expansion to the write of the new list; the expanding
//     tokens are compacted first (slot offsets in LDS), recombination goes through the LDS state table, and only the
//     later arrivals at an occupied state (a few percent) are spilled to memory for the first arrival to fold;
//   * the memory path (any size, and the end expansion): placements are staged in global arrays, one thread per placement.
template <int MODES>
__global__ __launch_bounds__(kThreads) void k_viterbi(const VitArgs argsInKernarg)
{
  // The arguments are read from the kernarg segment where they are used, through a pointer that is made opaque again at every phase boundary
  // (RELOAD): a field is a scalar load from the constant cache in the phase that needs it and dead after it.  Taken by value the two structs are
  // ~130 scalar registers that live from the first instruction to the last; with the per-slot pointers and loop state derived from them the kernel
  // needed 444 more scalars than the 102 a wave has, and every use in the hot phases was a v_readlane reload from a spill lane.
  (void) argsInKernarg;
  constexpr bool PROF = (MODES & 1) != 0, EXTRA = (MODES & 2) != 0;      // EXTRA: lattice bookkeeping, topN, token dump compiled in
  constexpr bool NARROW = (MODES & 4) != 0;                              // the state table is 2 x hashN one-word buckets (below) instead of two arrays of hashN words
  const KP KA = (KP) __builtin_amdgcn_kernarg_segment_ptr();
  KP ka = KA;
#define RELOAD() do { ka = KA; asm volatile("" : "+s"(ka)); } while (0)
  RELOAD();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* srow = reinterpret_cast<float*>(smem);                       // [nDist] when useLdsRow
  // per-frame open-addressing table in LDS: destination state -> first-arrival slot, 2 x hashN words, 0 = unused.
  //   wide:   hashN buckets of two words in two arrays -- hkey (state + 1; from P4 on bit31 | newest side record) and hfirst (smallest arrival slot, 0xFFFFFFFF = none)
  //   narrow: 2 x hashN buckets of one word (graphs of at most 65 535 states) -- bit 31 chain flag (0 while placements are inserted), bits 30..15 state + 1 while
  //           inserting / the newest side record once the flag is set, bits 14..0 the smallest arrival slot (slots < 24 576 < 2^15).  Same bytes, twice the buckets:
  //           a register-path frame (at most kFastC = 0.75 x 2 x hashN placements) never needs a second pass, and the status and fold reads are one word.
  // Global atomics execute at the memory side on gfx950 (no L2 residency); the LDS table keeps the recombination
  // traffic on chip.  Frames with more placements than the table can take fall back to the tagged global table.
  const int useLdsRow = ka->useLdsRow, nDist = ka->nDist, hashN = ka->hashN, regionB = ka->regionB, cntCap = ka->cntCap;   // (the LDS layout: live for the whole kernel)
  unsigned* hkey = reinterpret_cast<unsigned*>(srow + (useLdsRow ? ((nDist + 3) & ~3) : 4));
  unsigned* hfirst = hkey + hashN;
  unsigned* const tab = hkey; const int tabN = NARROW ? 2 * hashN : hashN;      // (narrow: the one-word buckets; tabN: buckets of either kind)
  Side* sideL = reinterpret_cast<Side*>(hfirst + hashN);                        // [regionB / 32] later arrivals at an occupied state
  // [cntCap] expansion counts of the list P6 wrote, by list position: the next frame's P1 scans them without waiting for the tokens to come back from memory
  unsigned short* cntL = reinterpret_cast<unsigned short*>(reinterpret_cast<unsigned char*>(hfirst + hashN) + regionB);
  __shared__ int s_waveTot[kWaves];
  __shared__ int s_waveTotE[kWaves];
  __shared__ double s_waveMin[kWaves];
  __shared__ float s_waveMag[kWaves];
  __shared__ unsigned long long s_waveKey[kWaves];
  __shared__ int s_sideN;
  __shared__ unsigned s_bm[kFastC / 32];             // register path: slots where an expanding token's run starts
  // register path, per group of 64 slots: expanding tokens that start before the group (13 bits) | how far into its token's run the group's first slot is (19 bits)
  __shared__ unsigned s_gbase[kFastC / 64 + 4];
  __shared__ int s_cnt[(kFastK + 32) * kWaves];
  __shared__ int s_err;             // register path: first arrivals per (k, wave) group, then their exclusive prefix
  __shared__ long long s_prof[32]; __shared__ long long s_tlast;
  // profiling build: the frames by size class -- at most 8 192 placements (all in registers), up to 12 288, more (register path), memory path: frames [0..3], ticks [4..7], placements [8..11]
  // [12], [13]: register-path frames that started laid out by the frame before / that ran P1 and P2; [14], [15]: memory-path frames of at most 28 672 / 32 767 placements
  __shared__ long long s_hist[PROF ? 16 : 1]; __shared__ long long s_tfr;
  // profiling build: the hops of an epsilon path behind the first (tick p31), counted per wave and placement of P3: [0] wave-placements, [1] those with a path of two or more hops,
  // [2] those that load hop costs (three or more hops), [3] those that run the generic hop loop, [4] hop iterations the waves execute, [5] hops their lanes need
  __shared__ unsigned long long s_hop[PROF ? 8 : 1];
  // per-utterance statistics and the cold loop state (thread 0 updates them once per frame; they used to ride in scalar registers through every phase)
  __shared__ long long s_stat[3];    // activeHypos, placements, registerFrames (low word) | those of them that started laid out (high word)
  __shared__ int s_maxActive; __shared__ unsigned s_tag; __shared__ long long s_latOff;
  if (PROF && threadIdx.x < 32) s_prof[threadIdx.x] = 0;
  if (PROF && threadIdx.x < 16) s_hist[threadIdx.x] = 0;
  if (PROF && threadIdx.x < 8) s_hop[threadIdx.x] = 0ull;
#define TICK(ix) do { if (PROF && tid == 0) { const long long tn = (long long) wall_clock64(); s_prof[ix] += tn - s_tlast; s_tlast = tn; } } while (0)
  constexpr int nthr = kThreads, nw = kWaves;
  __shared__ int s_u, s_seg, s_help; __shared__ long long s_chunk;

  const int tid = threadIdx.x;
  const int slot = blockIdx.x;
  // token lists: buffers 0 and 1 of the slot (current / next, swapped every frame), buffer 2 the spare of topN mode; pointers are formed where they are used
#define TOKA(ix) ((EXTRA && (ix) == 2) ? ka->D.tokA3 + (size_t) slot * ka->D.maxTok : ka->D.tokA + ((size_t) slot * 2 + (size_t) (ix)) * ka->D.maxTok)
#define TOKB(ix) ((EXTRA && (ix) == 2) ? ka->D.tokB3 + (size_t) slot * ka->D.maxTok : ka->D.tokB + ((size_t) slot * 2 + (size_t) (ix)) * ka->D.maxTok)
#define curA TOKA(bufCur)
#define nxtA TOKA(bufNxt)
#define curB TOKB(bufCur)
#define nxtB TOKB(bufNxt)
#define sprA TOKA(bufSpr)
#define sprB TOKB(bufSpr)
#define ctok (ka->D.ctok + (size_t) slot * 8192)
#define side (ka->D.side + (size_t) slot * kFastC)
  // (the staging arrays of the memory path)
#define cA (ka->D.cA + (size_t) slot * ka->D.maxCand)
#define cB (ka->D.cB + (size_t) slot * ka->D.maxCand)
  // first[] holds (tag << 24 | slot); tags count DOWN so every entry of an older frame compares larger and never
  // needs resetting; the table is wiped when the 8-bit tag runs out (and on the very first use of a slot)
  if (tid == 0) s_tag = ka->D.tags[slot];
  // back pointers: one arena per slot (lattice mode: one per utterance -- they outlive the slot: the host builds the lattice from them)
#define arena (ka->D.arena + (size_t) ((EXTRA && ka->D.latOn) ? u : (ka->D.segFrames > 0 ? 0 : slot)) * ka->D.arenaCap)
#define sc (ka->scores + (size_t) u * ka->Tmax * nDist)
  constexpr int fastCapC = ((kFastK + 32) * nthr < kFastC) ? (kFastK + 32) * nthr : kFastC;
  constexpr int fastCapN = kP1 * 64 * nw;                                   // kP1 rounds of 64 tokens per wave
  const bool fastOK = ka->D.fastOK && hashN >= 8192;
  // capacities that follow from the LDS budget of this launch: table (load <= 0.75 per pass), slot offsets, LDS side records
  // (regC: most placements of a register-path frame -- two passes over the wide table, one over the narrow one: the same number)
  const int tableC = (tabN >> 1) + (tabN >> 2), regC = NARROW ? tableC : 2 * tableC, eCap = kFastE, sideLds = regionB >> 5;

  // time slicing: the XCD this workgroup runs on (HW_REG_XCC_ID, bits 3:0) picks its queue and its share of the utterances (u = xcd mod 8)
  // (segQueues == 1: one queue, any workgroup may take any utterance up -- the hand-over then pays device-scope fences; small grids and the tests)
  const int nq = (EXTRA || ka->D.segFrames <= 0) ? 1 : ka->D.segQueues;
  const int xcd = nq == 8 ? (int) (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 7u) : 0;
  // help > 0: this workgroup's own queue is empty and it looks into queue (xcd + help) mod 8 for utterances NOBODY HAS STARTED.  With workgroups on every XCD
  // there are none by then; this is the net under the one assumption the XCD-bound queues make (a queue whose XCD got no workgroup of the grid would otherwise
  // never be served): such an utterance is decoded here in one go -- no hand-over, so no coherence question -- and marked so that its own queue passes it by.
  // (the queue being served lives in LDS, the work item comes out of it as (utterance, segment): nothing of this rides in registers through the frame loop)
  if (tid == 0) { s_help = (nq == 8 && ((ka->D.segDrop >> xcd) & 1)) ? 1 : 0; s_u = -2; }      // (s_u == -2: this workgroup has not asked for work yet)
  for (;;) {
    __syncthreads();
    if (tid == 0) {
      const int segS0 = EXTRA ? 0 : ka->D.segFrames; int help = s_help, uu = -1, sg = 0;
      for (;;) {
        const int qx = (xcd + help) & (nq - 1), Uq = (ka->U - qx + nq - 1) / nq;     // (nq is 1 or 8); utterances of this queue: u = qx mod nq
        int it = -1;
        // (oneEach: as many workgroups as utterances, never sliced -- workgroup u decodes utterance u and is done, so that no slot's arena is used twice)
        if (help == 0) { it = ka->oneEach ? (s_u == -2 ? slot : Uq) : atomicAdd(ka->D.queue + qx, 1); if (it >= (segS0 > 0 ? ka->D.segCount * Uq : Uq)) it = -1; }
        else {                                                                // first-segment items only, and only by compare-and-swap: a later item of that queue is not ours to take
          int c = ld_i32(ka->D.queue + qx);
          while (c < Uq) { const int prev = atomicCAS(ka->D.queue + qx, c, c + 1); if (prev == c) { it = c; break; } c = prev; }
        }
        if (it >= 0) { uu = segS0 > 0 ? qx + nq * (it % Uq) : it; sg = segS0 > 0 ? it / Uq : 0; break; }
        if (segS0 > 0 && nq == 8 && help < 7) help++; else break;
      }
      if (uu >= 0 && help > 0) { st_i32(&ka->D.segState[uu].status, -2); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); st_i32(&ka->D.segDone[uu], 0x7FFFFFFF); sg = -1; }   // taken whole
      s_help = help; s_u = uu; s_seg = sg;
    }
    __syncthreads();
    RELOAD();
    const int segS = EXTRA ? 0 : ka->D.segFrames;                           // segS > 0: time slicing (never with the lattice / topN / dump modes)
    const int u = s_u; if (u < 0) break;
    const bool whole = s_seg < 0; const int seg = whole ? 0 : s_seg;        // whole: an utterance of another queue that nobody had started, decoded here in one go
    const int T = ka->nframesArr[u] < ka->Tmax ? ka->nframesArr[u] : ka->Tmax;
    const int fr0 = seg * segS, frEnd = (segS > 0 && !whole) ? fr0 + segS : 0x7FFFFFFF;   // this item: frames fr0 .. frEnd-1 (the end expansion is "frame" T)
    if (fr0 > T) continue;                                                     // the utterance ended in an earlier segment
    if (EXTRA && ka->D.latOn && tid == 0) ka->D.latFrameOff[(size_t) u * (ka->Tmax + 3)] = 0;
    if (PROF && tid == 0) { const long long tn = (long long) wall_clock64(); if (s_prof[15]) s_prof[10] += tn - s_prof[15]; s_tlast = tn; }
#define dump (EXTRA && ka->D.dumpOn && slot == 0)

    int status = DSR_OK;
    if (T <= 0) status = DSR_E_ITERATOR;         // no frame at all: the exception escapes decode() (decoder.h:691)

    int bufCur = 0, bufNxt = 1, bufSpr = 2;
    int n = 1; long arenaOff = 0, chunkEnd = 0, arenaUsed = 0;             // arenaUsed: back-pointer records of the utterance so far (time slicing: its runs of the pool are not contiguous)
    double thresh = HUGE_VAL, topScore = HUGE_VAL;
    for (int i = tid; i < 2 * hashN; i += nthr) hkey[i] = (NARROW || i < hashN) ? 0u : 0xFFFFFFFFu;
    if (seg == 0) {
      if (tid == 0) {
        s_stat[0] = 0; s_stat[1] = 0; s_stat[2] = 0; s_maxActive = 0; s_latOff = 0;
        TokA t0; t0.ac = 0.0f; t0.lm = 0.0f; t0.bp = kNone; t0.xs = (uint32_t) ka->G.xoff[ka->G.initial]; curA[0] = t0;
        TokB b0; b0.node = ka->G.initial; b0.cnt = ka->G.xoff[ka->G.initial + 1] - ka->G.xoff[ka->G.initial]; curB[0] = b0;
      }
    } else {
      // the segment before may still be running on another CU: wait for it, then take the utterance over (token list into buffer 0, scalars)
      if (tid == 0) { while (ld_i32(&ka->D.segDone[u]) < seg) __builtin_amdgcn_s_sleep(16); }
      __syncthreads();
      if (nq == 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      const SegState* const sst = ka->D.segState + u;
      status = ld_i32(&sst->status);
      if (status != DSR_OK) continue;                                          // it failed there: its result and its trace head are written (or it is being decoded whole elsewhere, -2: not ours to touch)
      n = ld_i32(&sst->n); arenaOff = (long) ld_u64_dev(&sst->arenaOff); chunkEnd = (long) ld_u64_dev(&sst->chunkEnd); arenaUsed = (long) ld_u64_dev(&sst->arenaUsed); thresh = __longlong_as_double((long long) ld_u64_dev(&sst->thresh));
      if (tid == 0) { s_stat[0] = (long long) ld_u64_dev(&sst->stat[0]); s_stat[1] = (long long) ld_u64_dev(&sst->stat[1]); s_stat[2] = (long long) ld_u64_dev(&sst->stat[2]); s_maxActive = ld_i32(&sst->maxActive); s_latOff = 0; }
      const TokA* const svA = ka->D.saveA + (size_t) u * ka->D.maxTok; const TokB* const svB = ka->D.saveB + (size_t) u * ka->D.maxTok;
      for (int i = tid; i < n; i += nthr) {
        const unsigned long long a0 = ld_u64_dev(&svA[i]), a1 = ld_u64_dev(reinterpret_cast<const unsigned long long*>(&svA[i]) + 1), b0 = ld_u64_dev(&svB[i]);
        unsigned long long* da = reinterpret_cast<unsigned long long*>(&curA[i]); da[0] = a0; da[1] = a1; *reinterpret_cast<unsigned long long*>(&curB[i]) = b0;
      }
    }
    __syncthreads();

    bool cntOK = false;                                                        // cntL holds the counts of the current list, and every token of it passes the beam
    int preC = -1;                                                             // >= 0: the frame before has already laid out this frame's slots (bitmap, group table): preC placements
    const bool preRow = useLdsRow && nDist <= 2 * nthr;
    float rowNext[2] = {0.0f, 0.0f};
    if (preRow && fr0 < T) {                                                   // (the thread index opaque here too: its byte offsets, hoisted to the kernel's start, were a spilled register per utterance)
      const float* r0 = sc + (size_t) fr0 * nDist; int tidU = (int) threadIdx.x; asm volatile("" : "+v"(tidU));
      if (tidU < nDist) rowNext[0] = r0[tidU]; if (tidU + nthr < nDist) rowNext[1] = r0[tidU + nthr];
    }
    TICK(11);
    // frames 0..T-1 (mode 0), then the end expansion (mode 1) -- with time slicing: this segment's share of them
    int fr = fr0;
    for (; fr <= T && fr < frEnd && status == DSR_OK; fr++) {
      RELOAD();
      // the thread index behind an opaque copy, once per frame: nothing derived from it (lane masks, per-thread addresses of any
      // phase or of the memory path) can be hoisted out of the frame loop, where it would sit in scratch memory and be re-read
      int tidO = (int) threadIdx.x; asm volatile("" : "+v"(tidO));
      const int tid = tidO, lane = tid & 63, wave = tid >> 6;
      const int mode = (fr == T) ? 1 : 0;
      if (mode == 0 && useLdsRow) {
        if (preRow) {
          // the frame's score row was fetched into registers a frame ago (the load -> LDS store round trip was ~0.9 us on every frame's critical path)
          if (tid < nDist) srow[tid] = rowNext[0];
          if (tid + nthr < nDist) srow[tid + nthr] = rowNext[1];
          if (fr + 1 < T) {
            const float* nr = sc + (size_t) (fr + 1) * nDist;
            if (tid < nDist) rowNext[0] = nr[tid];
            if (tid + nthr < nDist) rowNext[1] = nr[tid + nthr];
          }
        } else { for (int i = tid; i < nDist; i += nthr) srow[i] = sc[(size_t) fr * nDist + i]; }
      }
      const float* rowG = sc + (size_t) fr * nDist;                            // the frame's score row in memory
      int numNew = 0, numStat = -1;                                           // tokens written to the new list / tokens the reference's list would hold
      if (fr > 0) TICK(23);                                                   // end of the frame before -> here
      if (PROF && tid == 0) { s_tlast = (long long) wall_clock64(); s_tfr = s_tlast; }
      bool fast = fastOK && mode == 0 && n <= fastCapN && !(EXTRA && (ka->D.latOn || ka->D.topN > 0));   // lattice bookkeeping needs every placement in memory: the memory path has them
      int Cfr = 0;                                                             // placements of this frame (statistics)

      if (fast) {
        // ======================= register path =======================
        const bool pre = preC >= 0;                                            // the slots of this frame were laid out when the list was written (P6): no P1, no P2
        // ---- P1: beam test, per-wave exclusive scans of the placement counts and of the expanding tokens.
        // Token loads are issued eight at a time (straight-line, clamped indices) so their latencies overlap.
        const int chunkT = ((n + nw * 64 - 1) / (nw * 64)) * 64;
        int C = preC, E = n;
        if (!pre) {
        float psc[kP1]; int pcn[kP1]; unsigned pk[kP1];                        // score; expansion count; slot offset | token index << 15 | bit31: expands
        int runC = 0, runE = 0;
        {
          const int b0 = wave * chunkT, b1 = (b0 + chunkT < n) ? b0 + chunkT : n;
#pragma unroll
          for (int g = 0; g < kP1; g += 8) {
            if (g * 64 < chunkT && cntOK) {
              // the list was written by the register path with pruning on: every token is within the beam (it was tested against this very threshold
              // when it was written) and its expansion count waits in LDS
#pragma unroll
              for (int it = g; it < g + 8; it++) { int i = b0 + it * 64 + lane; i = (i < n) ? i : n - 1; pcn[it] = (int) cntL[i]; psc[it] = -HUGE_VALF; }
            } else if (g * 64 < chunkT) {
#pragma unroll
              for (int it = g; it < g + 8; it++) {
                int i = b0 + it * 64 + lane; i = (i < n) ? i : n - 1;
                const float2 a = *reinterpret_cast<const float2*>(&curA[i].ac); pcn[it] = curB[i].cnt;
                psc[it] = __fadd_rn(a.x, a.y);
              }
            } else {
#pragma unroll
              for (int it = g; it < g + 8; it++) { pcn[it] = 0; psc[it] = 0.0f; }
            }
          }
          TICK(16);
          for (int i = tid; i < kFastC / 32; i += nthr) s_bm[i] = 0u;
          TICK(17);
#pragma unroll
          for (int it = 0; it < kP1; it++) {
            const int base = b0 + it * 64; pk[it] = 0u;
            if (base < b1) {
              const int i = base + lane; int cnt = 0;
              if (i < b1) {
                if (!((double) psc[it] > thresh)) cnt = pcn[it];               // beam (decoder.h:586-588)
              }
              pcn[it] = cnt;
              const int incl = wave_incl_scan(cnt, lane);
              const unsigned long long bal = __ballot(cnt > 0);
              if (cnt > 0) pk[it] = 0x80000000u | (unsigned) ((runC + incl - cnt) & 0x7FFF) | ((unsigned) ((runE + __popcll(bal & ((1ull << lane) - 1ull))) & 0xFFFF) << 15);
              runC += __builtin_amdgcn_readlane(incl, 63); runE += __popcll(bal);
            }
          }
          TICK(18);
          if (lane == 0) { s_waveTot[wave] = runC; s_waveTotE[wave] = runE; }
          if (tid == 0) { s_sideN = 0; s_gbase[0] = 0; s_err = 0; }
        }
        __syncthreads();
        TICK(0);
        int cbase, ebase;
        {                                                                      // lane w reads wave w's totals: two scans instead of a serial walk over 32 LDS words
          const int a = (lane < nw) ? s_waveTot[lane] : 0, b = (lane < nw) ? s_waveTotE[lane] : 0;
          const int sa = wave_incl_scan(a, lane), sb = wave_incl_scan(b, lane);
          C = __builtin_amdgcn_readlane(sa, 63); E = __builtin_amdgcn_readlane(sb, 63);
          const int wu = uni(wave);
          cbase = __builtin_amdgcn_readlane(sa - a, wu); ebase = __builtin_amdgcn_readlane(sb - b, wu);
        }
        TICK(19);
        if (!(C > fastCapC || E > eCap || C > regC)) {
          // ---- P2: compact list of the expanding tokens (their slot offsets in LDS, the tokens themselves in memory); a bitmap
          // of the slots where a token's run starts and the token count before every group of 64 slots turn "slot -> token"
          // into a population count
          // (when every token expands -- the rule once the lists are pruned at write time -- compact index == list index and the
          // list itself serves as the compact list: no copy)
          RELOAD();
          const bool ident = (E == n);
#pragma unroll
          for (int it = 0; it < kP1; it++) if (pk[it] & 0x80000000u) {
            const int e = ebase + (int) ((pk[it] >> 15) & 0xFFFFu); const int off = cbase + (int) (pk[it] & 0x7FFFu);
            if (!ident) ctok[e] = curA[wave * chunkT + it * 64 + lane];
            atomicOr(&s_bm[off >> 5], 1u << (off & 31));
            for (int g = (off >> 6) + 1; g <= ((off + pcn[it]) >> 6); g++) s_gbase[g] = (unsigned) (e + 1) | ((unsigned) (64 * g - off) << 13);   // this token covers slot 64g-1
          }
          __syncthreads();
        }
        } else __syncthreads();                                                // (laid out by the frame before; this barrier: the score row is in LDS)
        if (C > fastCapC || E > eCap || C > regC) { fast = false; __syncthreads(); }     // uniform: the memory path redoes the frame
        else {
          RELOAD();
          const bool ident = (E == n);
          const TokA* __restrict__ ctk = ident ? curA : ctok;
          TICK(1);
          Cfr = C;
          if (pre && tid == nthr - 1) s_stat[2] += 1ll << 32;                  // (the thread that counts the frame below)
          if (PROF && tid == 0) s_hist[pre ? 12 : 13] += 1;
          RELOAD();
          // (tq/lq/wq = tid/lane/wave behind an opaque copy: keeps the per-slot address arithmetic of the unrolled phases inside
          // the frame loop -- hoisted out of it, those hundred-odd invariants would live in scratch memory)
          int tq = tid; asm volatile("" : "+v"(tq)); const int lq = tq & 63, wq = tq >> 6;
          // ---- P3: slots c = k * nthr + tid (neighbouring lanes expand neighbouring arcs of the same few tokens).
          // A placement is four words: ac, lm, expansion record (bit30: silence arc) and ek = compact token index (bits 0..12) | table
          // bucket << 13 (wide: 14 bits and bit 27 = waits for the second pass; narrow: 15 bits) | bit 28: in the table, not folded yet
          // (bit 29, between token load and expansion only: the token's edge was a silence edge; after the fold: bit31 | side index when
          // a later arrival won).  The first kFastK per thread stay in
          // registers for the whole frame; slots beyond (one more batch of eight) are parked in memory between the phases.
          const int K = (C + nthr - 1) / nthr;
          float qac[kFastK], qlm[kFastK]; int qrec[kFastK]; unsigned ek[kFastK];
          double* const ttlS = reinterpret_cast<double*>(cA);                  // unrounded totals, read back by later arrivals only
          uint4* const ovf = reinterpret_cast<uint4*>(cB);                     // parked placements [slot - kFastK * nthr]
          const XRecD* const xrecD = ka->G.xrecD; const float* const pathCost = ka->G.pathCost; const uint32_t silenceX = ka->D.silenceX;
          double locMin = HUGE_VAL; float locMag = 0.0f;                       // locMag: largest |ac| + |lm| of the frame's placements (bounds the rounding of a score, see P4)
          const bool prevNull0 = (fr == 0);                                    // only the start token has no edge (decoder.h:960)
          const double lmS = ka->D.lmScale, lsPen = __dmul_rn(ka->D.lmScale, ka->D.lmPenalty), lsSil = __dmul_rn(ka->D.lmScale, ka->D.silPenalty);
          const bool sil0 = (0u == silenceX);
#pragma unroll
          for (int k = 0; k < kFastK; k++) { qac[k] = 0.0f; qlm[k] = 0.0f; qrec[k] = 0; ek[k] = 0u; }

          const int nPass = (!NARROW && C > tableC) ? 2 : 1;
          auto table_insert = [&](const unsigned dst, const unsigned prod, const int c) __attribute__((always_inline)) -> unsigned {
            const unsigned key = dst + 1u;
            unsigned h = (prod >> 7) & (unsigned) (tabN - 1); int probes = 0;
            if (NARROW) {
              const unsigned w = (key << 15) | (unsigned) c;                   // (the flag is clear while placements are inserted: equal keys = equal high bits, the min is over the slot)
              for (;;) {
                const unsigned kk = atomicCAS(&tab[h], 0u, w);
                if (kk == 0u) break;
                if ((kk >> 15) == key) { atomicMin(&tab[h], w); break; }
                h = (h + 1u) & (unsigned) (tabN - 1);
                if (++probes > tabN) { s_err = 1; break; }                     // table full: cannot happen below its capacity; fail loudly, never spin
              }
              return h;
            }
            for (;;) {
              const unsigned kk = atomicCAS(&hkey[h], 0u, key);
              if (kk == 0u || kk == key) break;
              h = (h + 1u) & (unsigned) (hashN - 1);                           // (triangular steps instead of linear ones: 16.5 vs 16.6 ms, nothing)
              if (++probes > hashN) { s_err = 1; break; }                      // table full: cannot happen below its capacity; fail loudly, never spin
            }
            atomicMin(&hfirst[h], (unsigned) c);
            return h;
          };
          // what P4 and the fold ask of a bucket, for either table.  Narrow: nothing changes a word's slot field after P3's barrier, so "am I the first arrival"
          // needs no barrier against the pushes of P4; a push keeps the slot field and retries only when another later arrival of the same state got in between.
          constexpr unsigned ekBucket = NARROW ? 0x7FFFu : 0x3FFFu;            // the bucket in ek, bits 13.. (wide: bit 27 = the state waits for the second pass)
          auto in_pass = [&](const unsigned e, const int pass) __attribute__((always_inline)) -> bool { return NARROW || (int) ((e >> 27) & 1u) == pass; };
          auto is_first = [&](const unsigned h, const int c) __attribute__((always_inline)) -> bool { return NARROW ? (tab[h] & 0x7FFFu) == (unsigned) c : hfirst[h] == (unsigned) c; };
          auto push_side = [&](const unsigned h, const int sx) __attribute__((always_inline)) -> unsigned {      // -> the record's 'next': bit31 | older side record, or a word without bit31
            if (NARROW) {
              unsigned old = tab[h];
              for (;;) { const unsigned prev = atomicCAS(&tab[h], old, 0x80000000u | ((unsigned) sx << 15) | (old & 0x7FFFu)); if (prev == old) break; old = prev; }
              return (old & 0x80000000u) ? (0x80000000u | ((old >> 15) & 0xFFFFu)) : 0u;
            }
            return atomicExch(&hkey[h], 0x80000000u | (unsigned) sx);
          };
          auto chain_head = [&](const unsigned h) __attribute__((always_inline)) -> unsigned {                  // bit31 | newest side record, or a word without bit31
            if (NARROW) { const unsigned w = tab[h]; return (w & 0x80000000u) ? (0x80000000u | ((w >> 15) & 0xFFFFu)) : 0u; }
            return hkey[h];
          };
          // slot -> (compact token index, position in its expansion list), then the token: score halves into the placement's own registers,
          // record index = first record of the node + position, bit29 of ek = the token's edge was a silence edge
          auto locate = [&](const int k, int& rec, unsigned& ekk) __attribute__((always_inline)) {
            const int c = k * nthr + tq; const int grp = k * nw + wq;
            unsigned e = 0u; int j = 0;
            if (c < C) {
              const unsigned long long W = ((unsigned long long) s_bm[2 * grp + 1] << 32) | s_bm[2 * grp];
              const unsigned gb = s_gbase[grp]; const unsigned long long mine = W & ((2ull << lq) - 1ull);
              e = (gb & 0x1FFFu) + (unsigned) __popcll(mine) - 1u;
              // position in the token's run: slots since the run's start -- inside this group (highest start bit at or below the lane), or carried in from
              // the group before (no second, dependent LDS read of the token's slot offset)
              j = mine ? lq - (63 - __clzll((long long) mine)) : lq + (int) (gb >> 13);
            }
            ekk = e; rec = j;
          };
          auto tokload = [&](float& ac, float& lm, int& rec, unsigned& ekk) __attribute__((always_inline)) {
            const TokA t = *at32<TokA>(ctk, ekk * 16u);
            ac = t.ac; lm = t.lm; rec += (int) (t.xs & 0x7FFFFFFFu); ekk |= (t.xs >> 31) << 29;
          };
          auto expandR = [&](auto NOPEN, const int g8, float* ac8, float* lm8, int* rec8, unsigned* ek8) __attribute__((always_inline)) {
            // NP: both penalty products are zero and no placement's lm can be -0.0 (checked on the host, DecoderState::noPen): "l + 0.0" is then
            // the identity and the four conditional additions of a placement -- an add and two selects each -- are left out
            constexpr bool NP = decltype(NOPEN)::value;
            int4 xr[kB]; double2 xl[kB];                  // the hot record: {dist, meta, dst, p2} and {lmCost, lmEps1} = lmScale x the record's two costs (viterbi.h)
#pragma unroll
            for (int i = 0; i < kB; i++) {                                      // eight record loads in flight
              xr[i] = *at32<int4>(xrecD, (uint32_t) rec8[i] * 32u); xl[i] = *at32<double2>(xrecD, (uint32_t) rec8[i] * 32u + 16u);
            }
            if (PROF) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TICK(28); }
            // The epsilon path (decoder.h:979-983) of both placements ahead of everything else of them, in one basic block: hops 2 to 4 are computed for every lane and
            // dropped by select where the path is shorter, as the first hop is.  The costs of hops 2.. of a path of three or more hops are loaded here for both placements,
            // as soon as the records are there, and first used behind the first hops (a two-hop path has its second cost in p2).  pls: hops whose costs are in
            // p2 / pathCost (0: slot beyond the frame, or a path of more than 14 hops -- those are walked through the arc arrays below).
            float hc[kB][3]; int pls[kB]; bool more[kB];
#pragma unroll
            for (int i = 0; i < kB; i++) {
              const int c = (g8 + i) * nthr + tq; const uint32_t xmeta = (uint32_t) xr[i].y;
              const int pl = (c < C) ? (int) (xmeta & 0xFFFFu) : 0;
              pls[i] = (xmeta & 0x80000000u) ? 0 : pl; more[i] = pl > 4;
              // (hops 3 and 4 of a shorter path are dropped below whatever their costs: p2 rather than a constant, which would draw the conversions -- and a wait -- into the branch)
              hc[i][0] = hc[i][1] = hc[i][2] = __int_as_float(xr[i].w);
              if (pls[i] > 2) {
                const uint32_t o = (uint32_t) xr[i].w * 4u;
                hc[i][0] = *at32<float>(pathCost, o); hc[i][1] = *at32<float>(pathCost, o + 4u); hc[i][2] = *at32<float>(pathCost, o + (pls[i] > 3 ? 8u : 4u));
              }
            }
            if (PROF) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TICK(31); }
#pragma unroll
            for (int i = 0; i < kB; i++) {
              const uint32_t xmeta = (uint32_t) xr[i].y; const bool tsil = (ek8[i] >> 29) & 1u;
              // selects in place of branches: the additions that may not apply are computed and dropped (same values, one
              // basic block -- the scalar operands are fetched once per placement instead of once per branch)
              float lmNode;                                                    // (every hop ends in a float: the node's lm stays in the placement's own register)
              {                                                                // first epsilon hop: its cost travels with the record
                double l = __dadd_rn((double) lm8[i], xl[i].y);
                if (!NP) {
                  const double l1 = __dadd_rn(l, lsPen); l = (xmeta & 0x20000u) ? l1 : l;
                  const double l2 = __dadd_rn(l, lsSil); l = (sil0 && (prevNull0 || !tsil)) ? l2 : l;   // prevIn != silenceX <=> the token's edge was no silence edge
                }
                lmNode = (xmeta & 0xFFFFu) ? (float) l : lm8[i];
              }
              if (PROF) {                                                      // what the hops behind the first cost this wave (s_hop), and their own tick
                unsigned long long iters = 0ull, need = 0ull; const int pl = more[i] ? (int) (xmeta & 0xFFFFu) : pls[i];
                for (int k = 1; k < 0x10000; k++) { const unsigned long long b = __ballot(pl > k); if (!b) break; if (k > 3) iters++; need += (unsigned long long) __popcll(b); }
                const unsigned long long act = __ballot((g8 + i) * nthr + tq < C); const bool loads = __ballot(pls[i] > 2) != 0ull;
                if (act && lq == __ffsll((long long) act) - 1) {
                  atomicAdd(&s_hop[0], 1ull); if (need) { atomicAdd(&s_hop[1], 1ull); atomicAdd(&s_hop[5], need); }
                  if (loads) atomicAdd(&s_hop[2], 1ull);
                  if (iters) { atomicAdd(&s_hop[3], 1ull); atomicAdd(&s_hop[4], iters); }
                }
                asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); TICK(29);
              }
#pragma unroll
              for (int h = 1; h < 4; h++) {                                    // (the edge before is an epsilon edge: no silence penalty possible here)
                double l = __dadd_rn((double) lmNode, __dmul_rn(lmS, (double) hc[i][h - 1]));
                if (!NP) { const double l1 = __dadd_rn(l, lsPen); l = ((xmeta >> (17 + h)) & 1u) ? l1 : l; }
                lmNode = (pls[i] > h) ? (float) l : lmNode;
              }
              if (PROF) TICK(31);
              lm8[i] = lmNode;
            }
            bool anyMore = false;
#pragma unroll
            for (int i = 0; i < kB; i++) anyMore = anyMore || more[i];
            if (__any(anyMore)) {                                              // a path of more than four hops in the wave: its further hops, one independent load each
#pragma unroll
              for (int i = 0; i < kB; i++) if (more[i]) {
                const uint32_t xmeta = (uint32_t) xr[i].y; const int plen = (int) (xmeta & 0xFFFFu), xp2 = xr[i].w;
                double lmNode = (double) lm8[i];
                if (!(xmeta & 0x80000000u)) {
                  for (int h = 4; h < plen; h++) {
                    double l = __dadd_rn(lmNode, __dmul_rn(lmS, (double) pathCost[xp2 + h - 1]));
                    if (!NP && ((xmeta >> (17 + h)) & 1u)) l = __dadd_rn(l, lsPen);
                    lmNode = (double) (float) l;
                  }
                } else {
                  const int* pp = ka->G.path + ka->G.xpathOff[rec8[i]];
                  for (int h = 1; h < plen; h++) {
                    const int a = pp[h];
                    double l = __dadd_rn(lmNode, __dmul_rn(lmS, (double) ka->G.arcCost[a]));
                    if (!NP && ka->G.arcOut[a] != 0) l = __dadd_rn(l, lsPen);
                    lmNode = (double) (float) l;
                  }
                }
                lm8[i] = (float) lmNode;
              }
            }
            if (PROF) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TICK(31); }
#pragma unroll
            for (int i = 0; i < kB; i++) {
              const int c = (g8 + i) * nthr + tq;
              const bool tsil = (ek8[i] >> 29) & 1u; ek8[i] &= 0x1FFFu;       // (taken out of ek here, behind the loads: a flag per placement held across them cost scratch memory)
              if (c < C) {
                const int xdist = xr[i].x; const uint32_t xmeta = (uint32_t) xr[i].y; const int xdst = xr[i].z;
                const bool has = (xmeta & 0xFFFFu) != 0u;
                const bool pnull = has ? false : prevNull0;
                const bool pinSil = has ? sil0 : tsil;                         // after an epsilon hop the edge input is 0
                double lm = __dadd_rn((double) lm8[i], xl[i].x);
                if (!NP) { const double lm1 = __dadd_rn(lm, lsPen); lm = (xmeta & 0x10000u) ? lm1 : lm; }
                const bool silArc = ((uint32_t) (xdist + 1) == silenceX);
                if (!NP) { const double lm2 = __dadd_rn(lm, lsSil); lm = (silArc && (pnull || !pinSil)) ? lm2 : lm; }
                float rowv;                                                    // (two branches, not "useLdsRow ? srow[..] : rowG[..]": that is one FLAT load)
                if (useLdsRow) { rowv = ((const lds_float_t*) srow)[xdist]; DSR_NO_MERGE(); } else rowv = rowG[xdist];
                const double ac = __dadd_rn((double) ac8[i], (double) rowv);
                const double ttl = __dadd_rn(ac, lm);
                *at32w<double>(ttlS, (uint32_t) c * 8u) = ttl; ac8[i] = (float) ac; lm8[i] = (float) lm; rec8[i] |= (silArc ? 0x40000000 : 0);
                if (ttl < locMin) locMin = ttl;                                // _topScore
                locMag = fmaxf(locMag, __fadd_rn(fabsf(ac8[i]), fabsf(lm8[i])));
                // state table: claim the bucket, keep the smallest slot (with two passes, the other half of the states waits)
                if (PROF) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); TICK(29); }
                const unsigned prod = (unsigned) xdst * 2654435761u;
                if (!NARROW && nPass > 1 && (prod >> 31)) ek8[i] |= 1u << 27;
                else ek8[i] |= (table_insert((unsigned) xdst, prod, c) << 13) | (1u << 28);      // bit28: in the table, not folded yet
                if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); TICK(30); }
              }
            }
          };
          auto expand8 = [&](auto NOPEN, const int g8, float* ac8, float* lm8, int* rec8, unsigned* ek8) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < kB; i++) locate(g8 + i, rec8[i], ek8[i]);
            if (PROF) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); TICK(26); }
#pragma unroll
            for (int i = 0; i < kB; i++) tokload(ac8[i], lm8[i], rec8[i], ek8[i]);
            if (PROF) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); TICK(27); }
            expandR(NOPEN, g8, ac8, lm8, rec8, ek8);
          };
          auto park_store = [&](const int kb, const float* oac, const float* olm, const int* orec, const unsigned* oek) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < kB; i++) { const int c = (kb + i) * nthr + tq; if (c < C) ovf[c - kFastK * nthr] = make_uint4(__float_as_uint(oac[i]), __float_as_uint(olm[i]), (unsigned) orec[i], oek[i]); }
          };
          auto park_load = [&](const int kb, float* oac, float* olm, int* orec, unsigned* oek) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < kB; i++) {
              int c = (kb + i) * nthr + tq; c = (c < C) ? c : kFastK * nthr;                // K > kFastK: that slot exists
              const uint4 v = ovf[c - kFastK * nthr];
              oac[i] = __uint_as_float(v.x); olm[i] = __uint_as_float(v.y); orec[i] = (int) v.z; oek[i] = v.w;
            }
          };
          auto runP3 = [&](auto NOPEN) __attribute__((always_inline)) {
#pragma unroll
            for (int g8 = 0; g8 < kFastK; g8 += kB) if (g8 < K) expand8(NOPEN, g8, &qac[g8], &qlm[g8], &qrec[g8], &ek[g8]);
            for (int kb = kFastK; kb < K; kb += kB) {
              float oac[kB], olm[kB]; int orec[kB]; unsigned oek[kB];
              expand8(NOPEN, kb, oac, olm, orec, oek); park_store(kb, oac, olm, orec, oek);
            }
          };
          if (ka->D.noPen) runP3(std::true_type{}); else runP3(std::false_type{});
          TICK(2);
          locMin = wave_min_d_uni(locMin); locMag = wave_max_f_uni(locMag);
          if (lq == 0) { s_waveMin[wq] = locMin; s_waveMag[wq] = locMag; }
          TICK(3);
          __syncthreads();
          TICK(4);
          for (int i = tq; i < kFastC / 32; i += nthr) s_bm[i] = 0u;          // every slot has found its token: the bitmap is free for the layout of the next frame (P6)
          topScore = HUGE_VAL;
          float frameMag;
          { const double v = (lq < nw) ? s_waveMin[lq] : HUGE_VAL; const float g = (lq < nw) ? s_waveMag[lq] : 0.0f;
            topScore = wave_min_d_uni(v); frameMag = wave_max_f_uni(g); }
          // A token whose score is above (this frame's best emitting total + beam) fails the beam test of the next frame
          // (decoder.h:586-588) and is never looked at again: it is counted (activeHypos, maxActive) but neither written to the list
          // nor to the back-pointer arena.  The order of the tokens that stay is unchanged, so the next frame's arrival slots are too.
          // Not on the last frame (the end expansion takes every token) and not when the lists are dumped.
          RELOAD();
          const double threshNext = __dadd_rn(topScore, ka->D.beam);
          const bool prune = !dump && (fr + 1 < T);
          // A LATER arrival that far above the threshold cannot touch a token that stays: a token that stays has score <= threshNext, and its
          // unrounded total (what the recombination compares, decoder.h:519-528) is within 2^-23 (|ac| + |lm|) of its score, so it beats
          // both such an arrival and whatever incumbent that arrival would have replaced (whose score is above the arrival's total).  Which of
          // two tokens above the threshold a state ends with is not observable (neither is written).  Such arrivals skip the chain: no side
          // record, no replay -- about two thirds of the later arrivals at the usual beam.
          const double doomT = prune ? __dadd_rn(threshNext, (double) __fmul_rn(frameMag, 4.76837158203125e-07f)) : HUGE_VAL;   // gap = 2^-21 x bound
          // ---- P4/P5, once per pass over the state table: later arrivals hang themselves on their bucket (the key word becomes
          // the chain head), then every first arrival folds its chain in slot order (decoder.h:519-528)
          unsigned long long firstMask = 0ull;
          auto later8 = [&](const int g8, const int pass, const float* ac8, const float* lm8, const int* rec8, const unsigned* ek8) __attribute__((always_inline)) {
            double tt[kB]; uint32_t pb[kB];
#pragma unroll
            for (int i = 0; i < kB; i++) {                                      // what a later arrival hands over; loaded for all (coalesced, in flight together)
              int c = (g8 + i) * nthr + tq; c = (c < C) ? c : 0;
              tt[i] = ttlS[c]; pb[i] = ctk[ek8[i] & 0x1FFFu].bp;
            }
#pragma unroll
            for (int i = 0; i < kB; i++) {
              const int c = (g8 + i) * nthr + tq;
              if (c < C && (ek8[i] & (1u << 28)) && in_pass(ek8[i], pass) && !((firstMask >> (g8 + i)) & 1ull)) {
                const unsigned h = (ek8[i] >> 13) & ekBucket;
                if (is_first(h, c)) firstMask |= 1ull << (g8 + i);
                else if (!((double) __fadd_rn(ac8[i], lm8[i]) > doomT)) {
                  const int sx = atomicAdd(&s_sideN, 1);
                  const unsigned nx = push_side(h, sx);
                  Side sd; sd.ttl = tt[i]; sd.ac = ac8[i]; sd.lm = lm8[i]; sd.rec = rec8[i]; sd.prevBp = pb[i]; sd.c = c; sd.next = nx;
                  if (sx < sideLds) sideL[sx] = sd; else side[sx] = sd;
                }
              }
            }
          };
          // (a first arrival that has been folded carries neither bucket nor pass bit any more: ek = token index, or bit31 | side index)
          // The replay of a state with two or more later arrivals: next replacement = smallest later slot that beats the incumbent,
          // until none does.  Returns the winning side record or -1.
          auto fold_multi = [&](const int wslot0, const unsigned head, const float ac, const float lm) __attribute__((always_inline)) -> int {
            int wslot = wslot0, wIdx = -1; double fw = (double) __fadd_rn(ac, lm);
            for (;;) {
              int best = 0x7FFFFFFF, bi = -1, steps = 0;
              for (unsigned p = head; (p & 0x80000000u) && steps <= C; steps++) {
                const int pi = (int) (p & 0x7FFFFFFFu);
                int pc; double pt; unsigned pn;
                side_link(sideL, side, sideLds, pi, pc, pt, pn);
                if (pc > wslot && pc < best && pt < fw) { best = pc; bi = pi; }
                p = pn;
              }
              if (bi < 0) break;
              wslot = best; wIdx = bi;
              fw = (double) side_score(sideL, side, sideLds, bi);
            }
            return wIdx;
          };
          // One placement's fold.  defer == nullptr: everything in place.  Otherwise a chain of two or more later arrivals is left for
          // the deferred round (its head goes to *defer): there the lanes of a wave replay their chains side by side instead of one
          // placement slot after the other with a single lane at work.
          auto fold1 = [&](const int k, const int pass, float& ac, float& lm, int& rec, unsigned& ekk, unsigned* defer) __attribute__((always_inline)) {
            const bool mine = ((firstMask >> k) & 1ull) && !(ekk & 0x80000000u) && (ekk & (1u << 28)) && in_pass(ekk, pass);
            if (mine) {
              const unsigned head = chain_head((ekk >> 13) & ekBucket);
              // narrow table: the owner wipes its bucket.  After the barrier that ends P4 nothing but a bucket's own first arrival reads or writes the bucket's word (the
              // later arrivals' status reads and pushes are before that barrier, the replays walk side records), every occupied word was claimed by a key, and every key has
              // exactly one smallest slot -- whose placement, doomed or pruned or neither, comes through here.  So every word is zero again at the barrier after the fold.
              if (NARROW) tab[(ekk >> 13) & ekBucket] = 0u;
              ekk &= 0x1FFFu;
              if (head & 0x80000000u) {
                int wIdx = -1;
                const int hi = (int) (head & 0x7FFFFFFFu);
                unsigned hnext; double pt;
                { int cdummy; side_link(sideL, side, sideLds, hi, cdummy, pt, hnext); }
                if (!(hnext & 0x80000000u)) {                                  // one later arrival (the usual case): a single comparison
                  if (pt < (double) __fadd_rn(ac, lm)) wIdx = hi;
                } else if (defer) *defer = head;
                else wIdx = fold_multi(k * nthr + tq, head, ac, lm);
                if (wIdx >= 0) {
                  side_winner(sideL, side, sideLds, wIdx, ac, lm, rec);
                  ekk = 0x80000000u | (unsigned) wIdx;
                }
              }
            }
          };
          // second pass: the waiting half of the states enters the (wiped) table
          auto insert8 = [&](const int g8, const int* rec8, unsigned* ek8) __attribute__((always_inline)) {
            int xd[kB];
#pragma unroll
            for (int i = 0; i < kB; i++) xd[i] = ka->G.xrecC[rec8[i] & 0x3FFFFFFF].dst;     // (the cold record: half the bytes per line of the gather)
#pragma unroll
            for (int i = 0; i < kB; i++) {
              const int c = (g8 + i) * nthr + tq;
              if (c < C && (ek8[i] & (1u << 27)) && !(ek8[i] & 0x80000000u)) ek8[i] |= (table_insert((unsigned) xd[i], (unsigned) xd[i] * 2654435761u, c) << 13) | (1u << 28);
            }
          };
          for (int pass = 0; pass < nPass; pass++) {
            if (!NARROW && pass > 0) {
              __syncthreads();                                                 // every chain of the pass before has been folded
              { uint4* h4 = reinterpret_cast<uint4*>(hkey); const int q4 = hashN >> 2;
                for (int i = tq; i < 2 * q4; i += nthr) { unsigned wv = (i < q4) ? 0u : 0xFFFFFFFFu; asm volatile("" : "+v"(wv)); h4[i] = make_uint4(wv, wv, wv, wv); }   /* (opaque: a hoisted constant vector lived through the whole frame loop, partly in scratch) */ }
              __syncthreads();
#pragma unroll
              for (int g8 = 0; g8 < kFastK; g8 += kB) if (g8 < K) insert8(g8, &qrec[g8], &ek[g8]);
              for (int kb = kFastK; kb < K; kb += kB) {
                float oac[kB], olm[kB]; int orec[kB]; unsigned oek[kB]; park_load(kb, oac, olm, orec, oek);
                insert8(kb, orec, oek); park_store(kb, oac, olm, orec, oek);
              }
              __syncthreads();
            }
            {
              // the status of every register slot first (one table read each, all in flight), then the few later arrivals that matter hang
              // themselves on their buckets side by side: a lane works through its own, whatever their slot number, and only they fetch their
              // unrounded total and the parent's back pointer from memory (fetching them for every slot cost a memory round trip per batch)
              unsigned later = 0u;
#pragma unroll
              for (int k = 0; k < kFastK; k++) {
                const bool cand = k < K && k * nthr + tq < C && (ek[k] & (1u << 28)) && in_pass(ek[k], pass) && !((firstMask >> k) & 1ull);
                if (cand) {
                  if (is_first((ek[k] >> 13) & ekBucket, k * nthr + tq)) firstMask |= 1ull << k;
                  else if (!((double) __fadd_rn(qac[k], qlm[k]) > doomT)) later |= 1u << k;
                }
              }
              asm volatile("" : "+v"(later));
              __builtin_amdgcn_sched_barrier(0);
              while (__any(later != 0u)) {
                if (later) {
                  const int k = __ffs((int) later) - 1; later &= later - 1u;
                  unsigned ekk = ek[0];
#pragma unroll
                  for (int j = 1; j < kFastK; j++) ekk = (k == j) ? ek[j] : ekk;
                  const int c = k * nthr + tq;
                  const double tt = ttlS[c]; const uint32_t pb = ctk[ekk & 0x1FFFu].bp;
                  const unsigned h = (ekk >> 13) & ekBucket;
                  const int sx = atomicAdd(&s_sideN, 1);
                  const unsigned nx = push_side(h, sx);
                  float ac = qac[0], lm = qlm[0]; int rec = qrec[0];
#pragma unroll
                  for (int j = 1; j < kFastK; j++) { const bool is = (k == j); ac = is ? qac[j] : ac; lm = is ? qlm[j] : lm; rec = is ? qrec[j] : rec; }
                  Side* dstS = (sx < sideLds) ? nullptr : &side[sx];
                  if (!dstS) { Side& q = sideL[sx]; q.ttl = tt; q.ac = ac; q.lm = lm; q.rec = rec; q.prevBp = pb; q.c = c; q.next = nx; }
                  else { dstS->ttl = tt; dstS->ac = ac; dstS->lm = lm; dstS->rec = rec; dstS->prevBp = pb; dstS->c = c; dstS->next = nx; }
                }
              }
            }
            for (int kb = kFastK; kb < K; kb += kB) { float oac[kB], olm[kB]; int orec[kB]; unsigned oek[kB]; park_load(kb, oac, olm, orec, oek); later8(kb, pass, oac, olm, orec, oek); }
            if (pass == 0) TICK(20);
            __syncthreads();
            if (pass == 0) TICK(5);
            {
              unsigned pend = 0u, dh[kFastK];
#pragma unroll
              for (int k = 0; k < kFastK; k++) { dh[k] = 0u; if (k < K) { fold1(k, pass, qac[k], qlm[k], qrec[k], ek[k], &dh[k]); if (dh[k]) pend |= 1u << k; } }
              if (pass == 0) TICK(24);
              while (__any(pend != 0u)) {                                     // deferred round(s): one chain per lane at a time
                if (pend) {
                  const int k = __ffs((int) pend) - 1; pend &= pend - 1u;
                  unsigned head = dh[0]; float ac = qac[0], lm = qlm[0];
#pragma unroll
                  for (int j = 1; j < kFastK; j++) { const bool is = (k == j); head = is ? dh[j] : head; ac = is ? qac[j] : ac; lm = is ? qlm[j] : lm; }
                  const int wIdx = fold_multi(k * nthr + tq, head, ac, lm);
                  if (wIdx >= 0) {
                    float wac, wlm; int wrec;
                    side_winner(sideL, side, sideLds, wIdx, wac, wlm, wrec);
#pragma unroll
                    for (int j = 0; j < kFastK; j++) if (k == j) { qac[j] = wac; qlm[j] = wlm; qrec[j] = wrec; ek[j] = 0x80000000u | (unsigned) wIdx; }
                  }
                }
              }
            }
            if (pass == 0) TICK(25);
            for (int kb = kFastK; kb < K; kb += kB) {
              float oac[kB], olm[kB]; int orec[kB]; unsigned oek[kB]; park_load(kb, oac, olm, orec, oek);
#pragma unroll
              for (int i = 0; i < kB; i++) if (kb + i < K) fold1(kb + i, pass, oac[i], olm[i], orec[i], oek[i], nullptr);
              park_store(kb, oac, olm, orec, oek);
            }
          }
          TICK(12);
          if (s_err) { status = DSR_E_ALLOCATION; break; }                     // (uniform: written before the barriers above)
          unsigned long long keepMask = 0ull;
#pragma unroll
          for (int k = 0; k < kFastK; k++) if (k < K && ((firstMask >> k) & 1ull)) {
            const float sc1 = __fadd_rn(qac[k], qlm[k]);
            if (!prune || !((double) sc1 > threshNext)) keepMask |= 1ull << k;
          }
          for (int kb = kFastK; kb < K; kb += kB) {
            float oac[kB], olm[kB]; int orec[kB]; unsigned oek[kB]; park_load(kb, oac, olm, orec, oek);
#pragma unroll
            for (int i = 0; i < kB; i++) if (kb + i < K && ((firstMask >> (kb + i)) & 1ull)) {
              const float sc1 = __fadd_rn(oac[i], olm[i]);
              if (!prune || !((double) sc1 > threshNext)) keepMask |= 1ull << (kb + i);
            }
          }
          // count the tokens that stay per (k, wave) group of 64 slots, and all new tokens for the statistics
          int allFirst = 0;
          for (int k = 0; k < K; k++) {
            const unsigned long long bal = __ballot((keepMask >> k) & 1ull);
            if (lq == 0) s_cnt[k * nw + wq] = __popcll(bal);
            allFirst += __popcll(__ballot((firstMask >> k) & 1ull));
          }
          if (lq == 0) s_waveTotE[wq] = allFirst;
          TICK(13);
          __syncthreads();
          TICK(14);
          // every chain has been folded: the state table is dead.  The wide table is wiped here, under wave 0's prefix sum; the narrow one is clean already -- its first
          // arrivals zeroed their own words in the fold (fold1), ~5 k words a frame instead of 128 KB.  A frame that leaves the loop before this point or below (s_err above,
          // the allocation statuses below) ends its utterance or segment: the next work item of this workgroup starts with the full wipe at the head of the item loop.
          if (!NARROW) {
            uint4* h4 = reinterpret_cast<uint4*>(hkey); const int q4 = hashN >> 2;
            for (int i = tq; i < 2 * q4; i += nthr) { unsigned wv = (i < q4) ? 0u : 0xFFFFFFFFu; asm volatile("" : "+v"(wv)); h4[i] = make_uint4(wv, wv, wv, wv); }
          }
          if (wq == 0) {                                                       // exclusive prefix over (k, wave) = slot order of the groups
            const int nG = K * nw;                                             // <= 6 * 64
            int a[6], tot = 0;
#pragma unroll
            for (int q = 0; q < 6; q++) { a[q] = (6 * lq + q < nG) ? s_cnt[6 * lq + q] : 0; tot += a[q]; }
            const int incl = wave_incl_scan(tot, lq); int run = incl - tot;
#pragma unroll
            for (int q = 0; q < 6; q++) { if (6 * lq + q < nG) s_cnt[6 * lq + q] = run; run += a[q]; }
            if (lq == 63) s_waveTot[0] = incl;
          }
          __syncthreads();
          TICK(6);
          numNew = uni(s_waveTot[0]);
          { const int a = (lq < nw) ? s_waveTotE[lq] : 0; numStat = __builtin_amdgcn_readlane(wave_incl_scan(a, lq), 63); }
          RELOAD();
          if (numNew > ka->D.maxTok || (segS > 0 ? arenaUsed : arenaOff) + numNew > ka->D.arenaCap) { status = DSR_E_ALLOCATION; break; }
          if (segS > 0 && arenaOff + numNew > chunkEnd) {                      // (uniform) the utterance's next run of back-pointer records from the pool
            const long need = numNew > ka->D.poolChunk ? (long) numNew : ka->D.poolChunk;
            __syncthreads();
            if (tid == 0) s_chunk = (long long) atomicAdd(ka->D.poolNext, (unsigned long long) need);
            __syncthreads();
            arenaOff = (long) s_chunk; chunkEnd = arenaOff + need;
            if (chunkEnd > ka->D.poolCap) { status = DSR_E_ALLOCATION; break; }
          }
          const XRecC* const xrecW = ka->G.xrecC; TokA* const outA = nxtA; TokB* const outB = nxtB; Bp* const outBp = arena + arenaOff;
          // ---- P6: the new list in reverse first-arrival order + back pointers (the cold records: destination and its expansion range); the state table is clean for the next frame
          auto write4 = [&](auto NB, const int g4, const float* ac4, const float* lm4, const int* rec4, const unsigned* ek4) __attribute__((always_inline)) {
            constexpr int nb = decltype(NB)::value;
            int4 dx[nb]; uint32_t pv[nb];
#pragma unroll
            for (int i = 0; i < nb; i++) {                                      // unconditional loads (every index is in bounds), in flight together;
              const bool kp = (keepMask >> (g4 + i)) & 1ull;                   // placements that are not written all read record 0 / token 0 (one line)
              dx[i] = *reinterpret_cast<const int4*>(&xrecW[kp ? (rec4[i] & 0x3FFFFFFF) : 0]);       // same state for every arrival
              const bool sw = kp && (ek4[i] & 0x80000000u) != 0u; const unsigned si = ek4[i] & 0x7FFFFFFFu;
              const uint32_t* pb = (sw && si >= (unsigned) sideLds) ? &side[si].prevBp : &ctk[(sw || !kp) ? 0u : (ek4[i] & 0x1FFFu)].bp;
              pv[i] = *pb;
              if (sw && si < (unsigned) sideLds) pv[i] = sideL[si].prevBp;
            }
#pragma unroll
            for (int i = 0; i < nb; i++) {
              const int k = g4 + i;
              if (k < K) {
                const bool isFirst = (keepMask >> k) & 1ull;
                const unsigned long long bal = __ballot(isFirst);
                if (isFirst) {
                  const int pos = numNew - 1 - (s_cnt[k * nw + wq] + __popcll(bal & ((1ull << lq) - 1ull)));
                  TokA na; na.ac = ac4[i]; na.lm = lm4[i]; na.bp = (uint32_t) (arenaOff + pos); na.xs = (uint32_t) dx[i].y | ((rec4[i] & 0x40000000) ? 0x80000000u : 0u);
                  TokB nb; nb.node = dx[i].x; nb.cnt = dx[i].z;
                  Bp bp; bp.prev = pv[i]; bp.rec = (uint32_t) (rec4[i] & 0x3FFFFFFF);
                  outA[pos] = na; outB[pos] = nb; outBp[pos] = bp;
                  if (pos < cntCap) cntL[pos] = (unsigned short) dx[i].z;
                }
              }
            }
          };
          // Three placements in four are not written (pruned, or later arrivals): the ones that are go through the (wiped) state table as a dense
          // list -- {ac, lm, record, where the parent's back pointer is} at its rank -- and the loads and stores of the write run over that list,
          // every lane at work, instead of over all slots with a quarter of the lanes.  A thread restores the table words it has read.
          // (more than 8 192 new tokens -- a list of at most kFastE tokens can fan out to that many states; the frame behind it then takes the memory path -- are written from the
          // slots: nothing is staged, so the table stays as the fold left it, clean)
          const bool dense = numNew <= (hashN >> 1);
          if (dense) {
            uint4* const stage = reinterpret_cast<uint4*>(hkey);
            auto stage1 = [&](const int k, const float ac, const float lm, const int rec, const unsigned ekk) __attribute__((always_inline)) {
              const bool isFirst = (keepMask >> k) & 1ull;
              const unsigned long long bal = __ballot(isFirst);
              if (isFirst) stage[s_cnt[k * nw + wq] + __popcll(bal & ((1ull << lq) - 1ull))] = make_uint4(__float_as_uint(ac), __float_as_uint(lm), (unsigned) rec, ekk);
            };
#pragma unroll
            for (int k = 0; k < kFastK; k++) if (k < K) stage1(k, qac[k], qlm[k], qrec[k], ek[k]);
            for (int kb = kFastK; kb < K; kb += kB) {
              float oac[kB], olm[kB]; int orec[kB]; unsigned oek[kB]; park_load(kb, oac, olm, orec, oek);
#pragma unroll
              for (int i = 0; i < kB; i++) if (kb + i < K) stage1(kb + i, oac[i], olm[i], orec[i], oek[i]);
            }
            __syncthreads();
            TICK(21);
            const int q4 = hashN >> 2;
            const bool layNext = prune && numNew <= 4 * nthr;                  // (at most two rounds of two list entries per thread)
            preC = -1;
            // one round of the dense write, two list entries per thread: the loads ...
            auto denseLoad = [&](const int f0, uint4* en, int4* dx, uint32_t* pv) __attribute__((always_inline)) {
#pragma unroll
              for (int i = 0; i < 2; i++) {
                const int f = f0 + i * nthr + tq; const bool on = f < numNew;
                en[i] = stage[on ? f : 0];
                if (on) { unsigned wv = (NARROW || f < q4) ? 0u : 0xFFFFFFFFu; asm volatile("" : "+v"(wv)); stage[f] = make_uint4(wv, wv, wv, wv); }
              }
#pragma unroll
              for (int i = 0; i < 2; i++) {
                const bool on = f0 + i * nthr + tq < numNew;
                dx[i] = *at32<int4>(xrecW, (on ? (en[i].z & 0x3FFFFFFFu) : 0u) * 16u);
                const bool sw = on && (en[i].w & 0x80000000u) != 0u; const unsigned si = en[i].w & 0x7FFFFFFFu;
                const uint32_t* pb = (sw && si >= (unsigned) sideLds) ? &side[si].prevBp : &ctk[(sw || !on) ? 0u : (en[i].w & 0x1FFFu)].bp;
                pv[i] = *pb;
                if (sw && si < (unsigned) sideLds) pv[i] = sideL[si].prevBp;
              }
            };
            // ... and the stores
            auto denseStore = [&](const int f0, const uint4* en, const int4* dx, const uint32_t* pv) __attribute__((always_inline)) {
#pragma unroll
              for (int i = 0; i < 2; i++) {
                const int f = f0 + i * nthr + tq;
                if (f < numNew) {
                  const int pos = numNew - 1 - f;
                  TokA na; na.ac = __uint_as_float(en[i].x); na.lm = __uint_as_float(en[i].y); na.bp = (uint32_t) (arenaOff + pos); na.xs = (uint32_t) dx[i].y | ((en[i].z & 0x40000000u) ? 0x80000000u : 0u);
                  TokB nb; nb.node = dx[i].x; nb.cnt = dx[i].z;
                  Bp bp; bp.prev = pv[i]; bp.rec = (uint32_t) (en[i].z & 0x3FFFFFFFu);
                  outA[pos] = na; outB[pos] = nb; outBp[pos] = bp;
                  if (pos < cntCap) cntL[pos] = (unsigned short) dx[i].z;
                }
              }
            };
            // The list this loop writes is the list the next frame expands, every token of it (pruning on: all pass the beam).  A token's first slot
            // there is the sum of the expansion counts of the tokens before it in the list = after it in rank: one block-wide sum over the counts the
            // loop has in hand anyway gives every token its slot offset, and the bitmap of run starts and the per-group table -- what P1 and P2 of the
            // next frame would rebuild from the list -- are written here.  That frame then starts at P3 (one barrier for its score row).
            // cn[i]: the expansion count of list entry f = i * nthr + tq (0 past the list's end), NE = 2 or 4 entries per thread.  The sum runs over the
            // (entry, wave) groups of 64 ranks in rank order -- at most 4 x 16 of them: one wave-wide scan of their totals.
            // A list with more placements than the register path takes is not laid out (the bitmap ends at kFastC): the next frame's P1 sends it to the memory path.
            auto layOut = [&](auto NE_, const int* cn) __attribute__((always_inline)) {
              constexpr int NE = decltype(NE_)::value;
              int in[NE]; bool bad = false;
#pragma unroll
              for (int i = 0; i < NE; i++) {
                in[i] = wave_incl_scan(cn[i], lq);
                bad = bad || (i * nthr + tq < numNew && cn[i] == 0);           // a token without arcs: the list is not its own compact list
              }
              const int badW = __any(bad) ? 1 : 0;
              if (lq == 63) {
#pragma unroll
                for (int i = 0; i < NE; i++) s_cnt[i * nw + wq] = in[i];
                s_waveTotE[wq] = badW;
              }
              __syncthreads();
              const int tg = (lq < NE * nw) ? s_cnt[lq] : 0;
              const int sg = wave_incl_scan(tg, lq);
              const int total = __builtin_amdgcn_readlane(sg, 63), wu = uni(wq);
              const bool anyBad = __any(((lq < nw) ? s_waveTotE[lq] : 0) != 0);
              const bool fits = total <= fastCapC;
#pragma unroll
              for (int i = 0; i < NE; i++) {
                const int f = i * nthr + tq; const int off = total - (__builtin_amdgcn_readlane(sg - tg, i * nw + wu) + in[i]);
                if (fits && f < numNew && cn[i] > 0) {
                  const int e = numNew - 1 - f;
                  atomicOr(&s_bm[off >> 5], 1u << (off & 31));
                  for (int g = (off >> 6) + 1; g <= ((off + cn[i]) >> 6); g++) s_gbase[g] = (unsigned) (e + 1) | ((unsigned) (64 * g - off) << 13);
                }
              }
              if (tq == 0) { s_sideN = 0; s_gbase[0] = 0; s_err = 0; }
              preC = (anyBad || !fits) ? -1 : total;
            };
            if (layNext && numNew > 2 * nthr) {
              // two rounds, then the layout over the four counts a thread has kept (holding the four entries themselves across the layout's barrier cost scratch memory)
              int cn[4];
#pragma unroll
              for (int h = 0; h < 2; h++) {
                uint4 en[2]; int4 dx[2]; uint32_t pv[2];
                denseLoad(h * 2 * nthr, en, dx, pv); denseStore(h * 2 * nthr, en, dx, pv);
#pragma unroll
                for (int i = 0; i < 2; i++) cn[2 * h + i] = ((2 * h + i) * nthr + tq < numNew) ? dx[i].z : 0;
              }
              layOut(std::integral_constant<int, 4>{}, cn);
            } else {
              for (int f0 = 0; f0 < numNew; f0 += 2 * nthr) {
                uint4 en[2]; int4 dx[2]; uint32_t pv[2];
                denseLoad(f0, en, dx, pv);
                if (layNext) {                                                 // (one round; its stores drain under the layout's scan)
                  const int cn[2] = { (tq < numNew) ? dx[0].z : 0, (nthr + tq < numNew) ? dx[1].z : 0 };
                  layOut(std::integral_constant<int, 2>{}, cn);
                }
                denseStore(f0, en, dx, pv);
              }
            }
            TICK(22);
          } else
          {
#pragma unroll
          for (int g4 = 0; g4 < kFastK; g4 += kW) if (g4 < K) write4(std::integral_constant<int, kW>{}, g4, &qac[g4], &qlm[g4], &qrec[g4], &ek[g4]);
          for (int kb = kFastK; kb < K; kb += kB) {
            float oac[kB], olm[kB]; int orec[kB]; unsigned oek[kB]; park_load(kb, oac, olm, orec, oek);
            write4(std::integral_constant<int, kB>{}, kb, oac, olm, orec, oek);
          }
          TICK(21);
          TICK(22);
          preC = -1;
          }
          cntOK = prune && numNew <= cntCap;
        }
      }
      if (!fast) {
      cntOK = false; preC = -1;
      // ======================= memory path =======================
      RELOAD();
      int* tokOff = ka->D.tokOff + (size_t) slot * (ka->D.maxTok + 1);
      int* tokCnt = ka->D.tokCnt + (size_t) slot * (ka->D.maxTok + 1);
      int* chead = ka->D.chead + (size_t) slot * ka->D.maxCand;
      int* owner = ka->D.owner + (size_t) slot * ka->D.maxCand;
      int* rank = ka->D.rank + (size_t) slot * ka->D.maxCand;
      unsigned* first = ka->D.first + (size_t) slot * ka->G.nNodes;
      unsigned tag = s_tag;
      __syncthreads();                                                         // (every thread has read the tag before thread 0 replaces it)
      if (tag <= 1u) { for (int i = tid; i < ka->G.nNodes; i += nthr) first[i] = 0xFFFFFFFFu; tag = 255u; __syncthreads(); } else tag--;
      if (tid == 0) s_tag = tag;
      const unsigned tagw = tag << 24;
      const bool sorted = EXTRA && ka->D.topN > 0 && mode == 0 && fr > 0;
      if (sorted) {
        // SortedIterator (decoder.h:298-320): the list sorted by the tokens' float scores (ties: list order -- std::sort leaves them unspecified),
        // of which _processFrame expands the first topN (:571-581).  Rank by counting: the lists of this mode are short (topN tokens' expansions).
        unsigned long long* keys = reinterpret_cast<unsigned long long*>(cA);
        for (int i = tid; i < n; i += nthr) { const TokA t = curA[i]; keys[i] = ((unsigned long long) f2ord(__fadd_rn(t.ac, t.lm)) << 32) | (unsigned) i; }
        __syncthreads();
        for (int i = tid; i < n; i += nthr) {
          const unsigned long long ki = keys[i]; int rk = 0;
          for (int j = 0; j < n; j++) rk += (keys[j] < ki) ? 1 : 0;
          if (rk < ka->D.topN) { sprA[rk] = curA[i]; sprB[rk] = curB[i]; }
        }
        __syncthreads();
        { const int t = bufCur; bufCur = bufSpr; bufSpr = t; }
        n = n < ka->D.topN ? n : ka->D.topN;
      }
      const double threshM = (EXTRA && ka->D.topN > 0) ? HUGE_VAL : thresh;       // topN mode: no beam
      // ---------------- phase A: per-token placement counts, wave-local exclusive scan
      const int chunkT = ((n + nw * 64 - 1) / (nw * 64)) * 64;
      {
        int running = 0;
        const int b0 = wave * chunkT, b1 = (b0 + chunkT < n) ? b0 + chunkT : n;
        for (int base = b0; base < b1; base += 64) {
          const int i = base + lane; int cnt = 0;
          if (i < b1) {
            const TokA ta = curA[i]; const TokB tb = curB[i];
            if (mode == 0) {
              const float s = __fadd_rn(ta.ac, ta.lm);
              if (!((double) s > threshM)) cnt = tb.cnt;                       // beam (decoder.h:586-588)
            } else cnt = (ka->G.nodeFinal[tb.node] ? 1 : 0) + (ka->G.eoff[tb.node + 1] - ka->G.eoff[tb.node]);
          }
          const int incl = wave_incl_scan(cnt, lane);
          if (i < b1) { tokOff[i] = running + incl - cnt; tokCnt[i] = cnt; }
          running += __shfl(incl, 63, 64);
        }
        if (lane == 0) s_waveTot[wave] = running;
      }
      __syncthreads();
      int C = 0;
      for (int w = 0; w < nw; w++) C += s_waveTot[w];
      if (C > ka->D.maxCand) { status = DSR_E_ALLOCATION; break; }
      if (EXTRA && ka->D.latOn && s_latOff + C > ka->D.latCap) { status = DSR_E_ALLOCATION; break; }
      Cfr = C;
      const bool useHash = hashN > 0 && C <= tableC;                             // load factor <= 0.75 even if every placement is a new state (narrow: 24 576 -- and every slot fits the word's 15 bits)
      // ---------------- phase A2: absolute offsets + owner fill
      for (int i = tid; i < n; i += nthr) {
        const int cnt = tokCnt[i];
        if (cnt == 0) continue;
        const int w = i / chunkT; int base = 0;
        for (int q = 0; q < w; q++) base += s_waveTot[q];
        const int off = base + tokOff[i];
        tokOff[i] = off;
        for (int j = 0; j < cnt; j++) owner[off + j] = i;
      }
      __syncthreads();
      // ---------------- phase B: one thread per placement
      double locMin = HUGE_VAL;
      for (int c = tid; c < C; c += nthr) {
        const int i = owner[c]; const TokA ta = curA[i]; const int nd = curB[i].node; const bool tokSil = (ta.xs >> 31) != 0u;
        Tok t; t.node = nd; t.ac = ta.ac; t.lm = ta.lm; t.bp = ta.bp;
        const int j = c - tokOff[i];
        double ac = (double) t.ac, lm; int dst, recId; bool silArc = false;
        if (mode == 0) {
          recId = (int) (ta.xs & 0x7FFFFFFFu) + j; const XRec x = ka->G.xrec[recId];
          const int plen = (int) (x.meta & 0xFFFFu);
          double lmNode = (double) t.lm; uint32_t prevIn = tokSil ? ka->D.silenceX : (ka->D.silenceX + 1u);   // only equality with silenceX matters
          bool prevNull = (t.bp == kNone) && (fr == 0);
          if (plen) {
            const int* pp = ka->G.path + ka->G.xpathOff[recId];
            for (int h = 0; h < plen; h++) {                                   // intermediate epsilon tokens (decoder.h:979-983)
              const int a = pp[h];
              double l = __dadd_rn(lmNode, __dmul_rn(ka->D.lmScale, (double) ka->G.arcCost[a]));
              if (ka->G.arcOut[a] != 0) l = __dadd_rn(l, __dmul_rn(ka->D.lmScale, ka->D.lmPenalty));
              if (0u == ka->D.silenceX && (prevNull || prevIn != ka->D.silenceX)) l = __dadd_rn(l, __dmul_rn(ka->D.lmScale, ka->D.silPenalty));
              lmNode = (double) (float) l; prevIn = 0u; prevNull = false;
            }
          }
          lm = __dadd_rn(lmNode, __dmul_rn(ka->D.lmScale, (double) x.cost));
          if (x.meta & 0x10000u) lm = __dadd_rn(lm, __dmul_rn(ka->D.lmScale, ka->D.lmPenalty));
          if ((uint32_t) (x.dist + 1) == ka->D.silenceX && (prevNull || prevIn != ka->D.silenceX)) lm = __dadd_rn(lm, __dmul_rn(ka->D.lmScale, ka->D.silPenalty));
          ac = __dadd_rn(ac, (double) (useLdsRow ? srow[x.dist] : rowG[x.dist]));
          dst = x.dst; silArc = ((uint32_t) (x.dist + 1) == ka->D.silenceX);
        } else {
          const int hasSelf = ka->G.nodeFinal[nd] ? 1 : 0;
          if (hasSelf && j == 0) {                                             // _expandToEnd self placement (decoder.h:506-509)
            const float lmf = (float) __dadd_rn((double) t.lm, __dmul_rn(ka->D.lmScale, (double) ka->G.nodeCost[nd]));
            lm = (double) lmf; dst = nd; recId = (int) 0x7FFFFFFE;
          } else {
            recId = ka->G.eoff[nd] + (j - hasSelf); const ERec e = ka->G.erec[recId];
            const int* pp = ka->G.path + e.pathOff; double lmNode = (double) t.lm; double l = lmNode;
            uint32_t prevIn = tokSil ? ka->D.silenceX : (ka->D.silenceX + 1u);
            for (int h = 0; h < e.pathLen; h++) {                              // _expandNodeToEnd (decoder.h:992-1015)
              const int a = pp[h];
              l = __dadd_rn(lmNode, __dmul_rn(ka->D.lmScale, (double) ka->G.arcCost[a]));
              if (ka->G.arcOut[a] != 0) l = __dadd_rn(l, __dmul_rn(ka->D.lmScale, ka->D.lmPenalty));
              if (0u == ka->D.silenceX && prevIn != ka->D.silenceX) l = __dadd_rn(l, __dmul_rn(ka->D.lmScale, ka->D.silPenalty));
              lmNode = (double) (float) l; prevIn = 0u;
            }
            lm = __dadd_rn(l, __dmul_rn(ka->D.lmScale, (double) ka->G.nodeCost[e.lastSrc]));
            dst = e.dst; recId = (int) ((uint32_t) recId | kEndBit);
          }
        }
        const double ttl = __dadd_rn(ac, lm);
        CandA a2; a2.ttl = ttl; a2.ac = (float) ac; a2.lm = (float) lm; cA[c] = a2;
        if (useHash) {
          unsigned h = ((unsigned) dst * 2654435761u) >> 7 & (unsigned) (tabN - 1);
          if (NARROW) {
            const unsigned key = (unsigned) dst + 1u, w = (key << 15) | (unsigned) c;
            for (;;) {
              const unsigned k = atomicCAS(&tab[h], 0u, w);
              if (k == 0u) break;
              if ((k >> 15) == key) { atomicMin(&tab[h], w); break; }
              h = (h + 1u) & (unsigned) (tabN - 1);
            }
          } else {
            for (;;) {
              const unsigned k = atomicCAS(&hkey[h], 0u, (unsigned) dst + 1u);
              if (k == 0u || k == (unsigned) dst + 1u) break;
              h = (h + 1u) & (unsigned) (hashN - 1);
            }
            atomicMin(&hfirst[h], (unsigned) c);
          }
          rank[c] = (int) h;
        } else atomicMin(&first[dst], tagw | (unsigned) c);
        chead[c] = -1;
        if (silArc) recId |= 0x40000000;
        CandB b2; b2.dst = dst; b2.next = -1; b2.rec = recId; b2.prevBp = t.bp; cB[c] = b2;
        if (mode == 0 && ttl < locMin) locMin = ttl;                           // _topScore (emitting placements only)
      }
      locMin = wave_min_d(locMin);
      if (lane == 0) s_waveMin[wave] = locMin;
      __syncthreads();
      topScore = HUGE_VAL;
      for (int w = 0; w < nw; w++) { const double v = s_waveMin[w]; if (v < topScore) topScore = v; }
      // ---------------- phase C0: later arrivals hang themselves on their state's first-arrival placement
      for (int c = tid; c < C; c += nthr) {
        int f;
        if (useHash) f = NARROW ? (int) (tab[rank[c]] & 0x7FFFu) : (int) hfirst[rank[c]];
        else { const int dst = cB[c].dst; f = (int) (ld_u32(&first[dst]) & 0x00FFFFFFu); }
        if (f != c) { const int nx = atomicExch(&chead[f], c); cB[c].next = nx; chead[c] = -2; }      // -2: not a first arrival
      }
      __syncthreads();
      if (useHash) for (int i = tid; i < 2 * hashN; i += nthr) hkey[i] = (NARROW || i < hashN) ? 0u : 0xFFFFFFFFu;   // ready for the next frame
      // ---------------- phase C1: fold per destination state (by its first-arrival thread), count new tokens
      const int chunkC = ((C + nw * 64 - 1) / (nw * 64)) * 64;
      // (as on the register path: tokens above this frame's best emitting total + beam are counted but not written)
      const double threshNextM = __dadd_rn(topScore, ka->D.beam);
      const bool pruneM = !dump && mode == 0 && (fr + 1 < T) && !(EXTRA && ka->D.topN > 0);
      {
        int running = 0, runAll = 0;
        const int b0 = wave * chunkC, b1 = (b0 + chunkC < C) ? b0 + chunkC : C;
        for (int base = b0; base < b1; base += 64) {
          const int c = base + lane; bool isFirst = false, isAny = false;
          if (c < b1) {
            const int h0 = ld_i32(&chead[c]);
            isFirst = (h0 != -2);
            if (isFirst) {
              int w = c; CandA aw = cA[w];
              double fw = (double) __fadd_rn(aw.ac, aw.lm);                   // incumbent's float score()
              for (;;) {                                                       // next replacement = smallest later slot that beats it
                int best = 0x7FFFFFFF;
                int steps = 0;                                                 // the list has at most C nodes: never spin on a corrupt link
                for (int p = h0; p >= 0 && steps <= C; p = cB[p].next, steps++) if (p > w && p < best && cA[p].ttl < fw) best = p;
                if (best == 0x7FFFFFFF) break;
                w = best; aw = cA[w]; fw = (double) __fadd_rn(aw.ac, aw.lm);
              }
              isAny = true;
              if (pruneM && ((double) __fadd_rn(aw.ac, aw.lm) > threshNextM)) { isFirst = false; w = -3; }    // -3: a new token that is not written
              chead[c] = w;                                                    // winner of this state
            }
          }
          const unsigned long long bal = __ballot(isFirst);
          if (isFirst) rank[c] = running + __popcll(bal & ((1ull << lane) - 1ull));
          running += __popcll(bal); runAll += __popcll(__ballot(isAny));
        }
        if (lane == 0) { s_waveTot[wave] = running; s_waveTotE[wave] = runAll; }
      }
      __syncthreads();
      numStat = 0;
      for (int w = 0; w < nw; w++) { numNew += s_waveTot[w]; numStat += s_waveTotE[w]; }
      if (numNew > ka->D.maxTok || (segS > 0 ? arenaUsed : arenaOff) + numNew > ka->D.arenaCap) { status = DSR_E_ALLOCATION; break; }
      if (segS > 0 && arenaOff + numNew > chunkEnd) {
        const long need = numNew > ka->D.poolChunk ? (long) numNew : ka->D.poolChunk;
        __syncthreads();
        if (tid == 0) s_chunk = (long long) atomicAdd(ka->D.poolNext, (unsigned long long) need);
        __syncthreads();
        arenaOff = (long) s_chunk; chunkEnd = arenaOff + need;
        if (chunkEnd > ka->D.poolCap) { status = DSR_E_ALLOCATION; break; }
      }
      // ---------------- phase C2: write the new token list (reverse first-arrival order) + back pointers
      {
        int wbase = 0; for (int q = 0; q < wave; q++) wbase += s_waveTot[q];
        const int b0 = wave * chunkC, b1 = (b0 + chunkC < C) ? b0 + chunkC : C;
        for (int base = b0; base < b1; base += 64) {
          const int c = base + lane;
          if (c < b1) {
            const int w = chead[c];
            if (w >= 0) {
              const CandB bc = cB[c];
              const int pos = numNew - 1 - (wbase + rank[c]);
              const CandA aw = cA[w]; const CandB bw = (w == c) ? bc : cB[w]; const int recW = (bw.rec & 0x3FFFFFFF) | (bw.rec & (int) 0x80000000);
              const int xo = ka->G.xoff[bc.dst];
              TokA na; na.ac = aw.ac; na.lm = aw.lm; na.bp = (uint32_t) (arenaOff + pos); na.xs = (uint32_t) xo;
              TokB nb; nb.node = bc.dst; nb.cnt = ka->G.xoff[bc.dst + 1] - xo;
              Bp bp;
              if (mode == 0) {
                if (bw.rec & 0x40000000) na.xs |= 0x80000000u;
                bp.prev = bw.prevBp; bp.rec = (uint32_t) recW;
              } else {
                if (bw.rec == (int) 0x7FFFFFFE) { if (segS > 0) { const unsigned long long v = ld_u64_dev(&arena[bw.prevBp]); bp.prev = (uint32_t) v; bp.rec = (uint32_t) (v >> 32); } else { const Bp o = arena[bw.prevBp]; bp = o; } }     // replaces the token in its chain
                else { bp.prev = bw.prevBp; bp.rec = (uint32_t) bw.rec; }
              }
              nxtA[pos] = na; nxtB[pos] = nb; arena[arenaOff + pos] = bp;
              if (EXTRA && ka->D.latOn) ka->D.arenaLat[(size_t) u * ka->D.arenaCap + arenaOff + pos] = (int) (s_latOff + w);
            }
          }
        }
      }
      if (EXTRA && ka->D.latOn) {                                                 // this frame's placements, arrival order
        uint4* lat = ka->D.lat + (size_t) u * ka->D.latCap; double* ltt = ka->D.latTtl + (size_t) u * ka->D.latCap;
        const long latOff = (long) s_latOff;
        for (int c = tid; c < C; c += nthr) {
          const CandA a = cA[c]; const CandB b = cB[c];
          lat[latOff + c] = make_uint4(__float_as_uint(a.ac), __float_as_uint(a.lm), (unsigned) b.rec, b.prevBp); ltt[latOff + c] = a.ttl;
        }
        __syncthreads();                                                       // (every thread has read the offset before thread 0 advances it)
        if (tid == 0) { s_latOff = latOff + C; ka->D.latFrameOff[(size_t) u * (ka->Tmax + 3) + fr + 1] = latOff + C; }
      }
      }   // memory path
      __syncthreads();
      TICK(fast ? 7 : 8);
      if (PROF && tid == 0 && mode == 0) { const int cls = !fast ? 3 : Cfr <= kFastK * nthr ? 0 : Cfr <= 12288 ? 1 : 2; s_hist[cls] += 1; s_hist[4 + cls] += s_tlast - s_tfr; s_hist[8 + cls] += Cfr; if (!fast && Cfr <= 28672) s_hist[14] += 1; if (!fast && Cfr <= 32767) s_hist[15] += 1; }
      RELOAD();
      if (mode == 0) {
        if (dump) {
          long* cnt = ka->D.dumpCount; const long o = cnt[0];
          if (o + numNew <= ka->D.dumpCap) {
            for (int i = tid; i < numNew; i += nthr) {
              const TokA t = ld_tok(&nxtA[i]); ka->D.dumpNode[o + i] = nxtB[i].node; ka->D.dumpAc[o + i] = t.ac; ka->D.dumpLm[o + i] = t.lm;
              ka->D.dumpArc[o + i] = ka->G.xarc[arena[t.bp].rec];
            }
          }
          __syncthreads();
          if (tid == 0) { ka->D.dumpFrameOff[fr] = o; ka->D.dumpFrameOff[fr + 1] = o + numNew; cnt[0] = o + numNew; cnt[1] = fr + 1; }
        }
        if (numStat < 0) numStat = numNew;                                     // memory path: every new token is written
        if (numStat == 0 || numNew == 0) { status = DSR_E_CONSISTENCY; break; } // no token can be expanded in the next frame: the reference never terminates from here
        { const int t = bufCur; bufCur = bufNxt; bufNxt = t; }
        n = numNew; arenaOff += numNew; arenaUsed += numNew;
        if (tid == nthr - 1) { s_stat[0] += numStat; s_stat[1] += Cfr; if (fast) s_stat[2] += 1; if (numStat > s_maxActive) s_maxActive = numStat; }   // (off wave 0's path: it carries the prefix sums)
        thresh = __dadd_rn(topScore, ka->D.beam);
      } else {
        // ---------------- best token (decoder.h:639-685): list order, strict '<' on the float score
        const TokA* lst = numNew > 0 ? nxtA : curA; const int cntL = numNew > 0 ? numNew : n;
        unsigned long long key = ~0ull;
        for (int i = tid; i < cntL; i += nthr) {
          const TokA t = lst[i]; const float s = __fadd_rn(t.ac, t.lm);
          if (s == s) { const unsigned long long k = ((unsigned long long) f2ord(s) << 32) | (unsigned) i; if (k < key) key = k; }
        }
        key = wave_min_u64(key);
        if (lane == 0) s_waveKey[wave] = key;
        if (EXTRA && ka->D.latOn) {                                               // _next after _expandToEnd (or _current when no token is final), list order
          const TokB* lstB = numNew > 0 ? nxtB : curB; int4* lf = ka->D.latFinal + (size_t) u * ka->D.maxTok;
          for (int i = tid; i < cntL; i += nthr) { const TokA t = ld_tok(&lst[i]); lf[i] = make_int4(lstB[i].node, (int) t.bp, __float_as_int(t.ac), __float_as_int(t.lm)); }
          if (tid == 0) { int* li = ka->D.latInfo + 4 * (size_t) u; li[0] = cntL; li[1] = numNew > 0 ? 1 : 0; li[2] = (int) (arenaOff + (numNew > 0 ? numNew : 0)); li[3] = T; }
        }
        __syncthreads();
        // The traceback itself (bestHypo, decoder.h:748-773) is k_traceback's: this workgroup holds a whole CU, and the walk is one thread waiting on a chain of
        // dependent loads.  Thread 0 fills the result record up to the best token and leaves the head of the chain -- the token's back pointer and where this
        // utterance's records start in D.arena -- by UTTERANCE (slots are reused).  Only where this slot's next utterance overwrites the records (walkHere: run to
        // completion with more utterances than workgroups, outside lattice mode) the chain is followed here, into the hop scratch k_traceback works from.
        // (the result record is written by thread 0 alone and lives in memory: as a register struct of every thread it was
        // a block of zeros carried -- and spilled -- through the whole kernel)
        if (tid == 0) {
          dsr_decode_result* const res = ka->res;
          clear_result(&res[u]); dsr_decode_result& r = res[u];
          unsigned long long k = ~0ull; for (int w = 0; w < nw; w++) if (s_waveKey[w] < k) k = s_waveKey[w];
          r.frames = T - 1; r.reachedFinal = numNew > 0 ? 1 : 0; r.finalStatesN = numNew; /* every token of _next after _expandToEnd sits in a final state */ r.activeHypos = (long) s_stat[0]; r.placements = (long) s_stat[1] + Cfr; r.registerFrames = (long) (s_stat[2] & 0xFFFFFFFFll); r.laidOutFrames_ = (int) (s_stat[2] >> 32); r.maxActiveSeen = s_maxActive; r.status = DSR_OK;
          TraceHead hd; hd.arenaOff = (unsigned long long) ((size_t) ((EXTRA && ka->D.latOn) ? u : (ka->D.segFrames > 0 ? 0 : slot)) * ka->D.arenaCap); /* as the arena macro */ hd.bp = kNone; hd.hops = kNone;
          if (k != ~0ull) {
            const TokA bt = ld_tok(&lst[(unsigned) (k & 0xFFFFFFFFu)]);
            r.ac = bt.ac; r.lm = bt.lm; r.score = __dadd_rn((double) bt.ac, (double) bt.lm);
            hd.bp = bt.bp;
            if (ka->walkHere) {
              int* const hopRec = ka->hopRec + (size_t) u * ka->hopStride; const int walkCap = 2 * ka->D.maxCand < ka->hopStride ? 2 * ka->D.maxCand : ka->hopStride; int nH = 0;
              for (uint32_t bq = bt.bp; bq != kNone && nH < walkCap; ) { const uint2 e = *reinterpret_cast<const uint2*>(&arena[bq]); hopRec[nH++] = (int) e.y; bq = e.x; }
              hd.hops = (uint32_t) nH;
            }
          } else r.status = DSR_E_CONSISTENCY;
          ka->heads[u] = hd;
        }
        __syncthreads();
        TICK(9);
      }
    }   // frames

    RELOAD();
    if (PROF && tid == 0) s_prof[15] = (long long) wall_clock64();
    if (segS > 0 && status == DSR_OK && fr <= T) {
      // the segment is done and the utterance is not: it is put down -- list and scalars to memory, visible to the whole device, THEN the segment count
      TokA* const svA = ka->D.saveA + (size_t) u * ka->D.maxTok; TokB* const svB = ka->D.saveB + (size_t) u * ka->D.maxTok;
      for (int i = tid; i < n; i += nthr) { svA[i] = curA[i]; svB[i] = curB[i]; }
      if (tid == 0) {
        SegState* const sst = ka->D.segState + u;
        st_i32(&sst->n, n); st_i32(&sst->status, DSR_OK); st_i32(&sst->maxActive, s_maxActive); st_u64_dev(&sst->arenaOff, (unsigned long long) arenaOff); st_u64_dev(&sst->chunkEnd, (unsigned long long) chunkEnd); st_u64_dev(&sst->arenaUsed, (unsigned long long) arenaUsed);
        st_u64_dev(&sst->thresh, (unsigned long long) __double_as_longlong(thresh));
        st_u64_dev(&sst->stat[0], (unsigned long long) s_stat[0]); st_u64_dev(&sst->stat[1], (unsigned long long) s_stat[1]); st_u64_dev(&sst->stat[2], (unsigned long long) s_stat[2]);
      }
      if (nq == 1) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      else __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");                // every thread's stores have reached the L2 (s_waitcnt vmcnt(0): the L1 writes through)
      __syncthreads();
      if (tid == 0) st_i32(&ka->D.segDone[u], seg + 1);
      continue;
    }
    if (status != DSR_OK) {
      // abort: the tagged state table needs no cleaning
      if (tid == 0) {
        dsr_decode_result* const res = ka->res; clear_result(&res[u]); res[u].status = status; res[u].frames = T - 1;
        { TraceHead hd; hd.arenaOff = 0ull; hd.bp = kNone; hd.hops = kNone; ka->heads[u] = hd; }                                   // nothing for k_traceback to follow
        if (segS > 0) { st_i32(&ka->D.segState[u].status, status); asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); st_i32(&ka->D.segDone[u], 0x7FFFFFFF); }   // later segments pass by
      }
    }
  }
  RELOAD();
  if (tid == 0) ka->D.tags[slot] = s_tag;
  if (PROF && tid < 32) ka->D.prof[slot * kProfN + tid] = s_prof[tid];
  if (PROF && tid < 16) ka->D.prof[slot * kProfN + 32 + tid] = s_hist[tid];
  if (PROF && tid < 8) ka->D.prof[slot * kProfN + 48 + tid] = (long long) s_hop[tid];
#undef TICK
#undef RELOAD
#undef TOKA
#undef TOKB
#undef curA
#undef nxtA
#undef curB
#undef nxtB
#undef sprA
#undef sprB
#undef ctok
#undef side
#undef cA
#undef cB
#undef arena
#undef sc
#undef dump
}

}  // namespace dsr

// Which XCD a workgroup lands on: HW_REG_XCC_ID of workgroup i of a 64-workgroup grid (decoder.cpp, xcd_round_robin)
extern "C" __global__ void k_xcc_probe(int* out) { if (threadIdx.x == 0) out[blockIdx.x] = (int) (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u); }

namespace dsr {

void xcc_probe_launch(int* out64, hipStream_t st) { launch(k_xcc_probe, dim3(64), dim3(64), 0, st, out64); }

// modes -> instantiation (viterbi.h: bit 0 ticks, bit 1 lattice / topN / dump, bit 2 narrow table)
typedef void (*VitKernel)(const VitArgs);
static constexpr VitKernel kVitKernels[8] = { k_viterbi<0>, k_viterbi<1>, k_viterbi<2>, k_viterbi<3>, k_viterbi<4>, k_viterbi<5>, k_viterbi<6>, k_viterbi<7> };

size_t viterbi_static_lds(int modes)
{
  hipFuncAttributes fattr; DSR_HIP(hipFuncGetAttributes(&fattr, (const void*) kVitKernels[modes & 7]));
  return fattr.sharedSizeBytes;
}
void viterbi_launch(int modes, const VitArgs& A, int slots, size_t ldsBytes, hipStream_t st)
{
  const VitKernel k = kVitKernels[modes & 7];
  launch(k, dim3(slots), dim3(kThreads), ldsBytes, st, A);
}

}  // namespace dsr
