// csrc/src_kernels.hip -- the kernels of the sample-rate converter (include/dsr.h section 6d) and their launch.  Host side: csrc/src.cpp.
//
// Output n of a row sits at input time n M / L: base = floor(n M / L), phase p = (n M) mod L.  A sinc method sums 2K taps,
//   y[n] = sum_{jj = 0 .. 2K-1} h[row][jj] * x[base - K + 1 + jj],    row = n mod L  (the table's rows are in output order: src.cpp),
// as two chains acc = fmaf(h, x, acc) from acc = 0, one over the even jj and one over the odd jj, each ascending, and the rounded sum of the two.
// Every path below forms an output with exactly these operations -- a sample outside the stream is a zero that goes through its chain like any
// other -- so the paths, the tile splits and the block splits agree bit for bit.
//
//   k_src_sinc<TABLE, INPUT>  a workgroup walks tilesPerBlock tiles of `run` consecutive outputs of one (u, c) row.  Per tile it stages the
//                input span the tile reads, run M / L + 2K floats, in LDS with coalesced loads; each lane then forms whole outputs (which of the
//                tile's: src_lane_pitch), which leave through LDS in order.  TABLE says where h comes from: LDS (copied once per workgroup, row stride 2K + 1: odd, so
//                the rows of the 32 lanes of an LDS cycle, an odd pitch apart, start on 32 different banks), memory (through the cache: the table
//                does not fit beside the tile), or uniform (L = 1, integer decimation: one row for all lanes, read with wave-uniform addresses).
//                M = 1 (integer interpolation) needs no kernel of its own: L consecutive lanes read the same input window, which LDS broadcasts.
//                INPUT direct reads x from memory instead of LDS: ratios whose 2K alone is larger than a tile.
//   k_src_simple zoh and linear (and the copy of equal rates): a thread an output, straight from memory.
//   k_src_hist / k_src_counts  the carried state after a block: the last 2K input samples of every row, then the counts of every utterance.
#include "src.h"
#include "launch.h"

namespace dsr {

enum { TBL_LDS = DSR_SRC_TABLE_LDS, TBL_MEM = DSR_SRC_TABLE_MEM, TBL_UNIFORM = DSR_SRC_TABLE_UNIFORM };
constexpr int kSrcThreads = 1024;
constexpr size_t kSrcLds = 160 * 1024;          // LDS of a CU: the most one workgroup can ask for
constexpr size_t kSrcTileLds = 64 * 1024;       // the most a tile takes when the table is not in LDS (two workgroups a CU)

struct SrcArgs {
  const float* x; const int32_t* nsamp; float* y; int32_t* nout; SrcCount* cnt; float* hist; const float* table;
  long inStride, outStride; int C, L, M, K, taps, stride, H, flush, run, tilesPerBlock, chunks, linear, lanePitch;
};

// what a call does for utterance u: the stream position a of its first input sample, its nIn samples, the first output n0 and the count of outputs
struct SrcRange { int64_t a, n0; int nIn, count; };
__device__ __forceinline__ SrcRange src_range(const SrcArgs& g, int u)
{
  SrcRange r;
  long n = g.nsamp ? (long) g.nsamp[u] : g.inStride; n = n < 0 ? 0 : n > g.inStride ? g.inStride : n;
  r.nIn = (int) n; r.a = g.cnt ? g.cnt[u].nin : 0; r.n0 = g.cnt ? g.cnt[u].nout : 0;
  const int64_t b = r.a + n, all = (b * g.L) / g.M;                       // floor(b L / M): what a stream of b samples gives in all
  int64_t end = all;
  if (g.cnt && !g.flush) {                                               // the outputs whose last tap base + K lies below b: n M < (b - K) L
    const int64_t t = b - g.K; end = t > 0 ? (t * g.L + g.M - 1) / g.M : 0;
    if (end > all) end = all;
  }
  int64_t c = end - r.n0; c = c < 0 ? 0 : c > g.outStride ? g.outStride : c;
  r.count = (int) c;
  return r;
}

// sample `rel` of the call's input row (0 = its first sample); before it the carried history, zeros where there is neither.  One load site.
__device__ __forceinline__ float src_fetch(const float* x, const float* hist, int H, long rel, int nIn)
{
  const float* p = rel >= 0 ? x + rel : hist + (H + rel);
  const bool ok = rel >= 0 ? rel < nIn : (hist != nullptr && rel >= -(long) H);
  float v = 0.0f;
  if (ok) v = *p;
  return v;
}

constexpr int kSrcStage = 8;                    // input samples a lane holds in registers for the next tile: a span is at most 8 x 1024 floats

// a tile of a workgroup's walk: outputs [o0, oEnd) of the call; live: some of them exist (the others are zeros); its first output's base and phase
struct SrcTile { bool in, live; long o0, oEnd, lo; unsigned p0, q0; int span; };
__device__ __forceinline__ SrcTile src_tile(const SrcArgs& g, const SrcRange& r, int chunk, int t)
{
  SrcTile k; k.o0 = ((long) chunk * g.tilesPerBlock + t) * g.run; k.in = t < g.tilesPerBlock && k.o0 < g.outStride;
  k.oEnd = k.o0 + g.run < g.outStride ? k.o0 + g.run : g.outStride; k.live = k.in && k.o0 < r.count;
  const int64_t nFirst = r.n0 + k.o0, t0 = nFirst * g.M, base0 = t0 / g.L;
  k.p0 = (unsigned) (t0 % g.L); k.q0 = (unsigned) (nFirst % g.L);
  k.lo = (long) (base0 - g.K + 1 - r.a);                               // the tile's first input sample, relative to the call's
  k.span = (int) (((unsigned) (g.run - 1) * (unsigned) g.M + k.p0) / (unsigned) g.L) + g.taps;
  return k;
}

template <int TABLE, bool XLDS>
__global__ __launch_bounds__(kSrcThreads) void k_src_sinc(SrcArgs g)
{
  extern __shared__ float src_lds[];
  const int row = blockIdx.x / g.chunks, chunk = blockIdx.x % g.chunks, u = row / g.C, tid = threadIdx.x;
  const SrcRange r = src_range(g, u);
  const float* x = g.x + (size_t) row * g.inStride; float* y = g.y + (size_t) row * g.outStride;
  const float* hist = g.hist ? g.hist + (size_t) row * g.H : nullptr;
  if (chunk == 0 && tid == 0 && g.nout && row % g.C == 0) g.nout[u] = r.count;
  // LDS: the table (TBL_LDS), the tile's outputs, the tile's input span
  float* tl = src_lds; float* ys = src_lds + (TABLE == TBL_LDS ? (size_t) g.L * g.stride : 0); float* xs = ys + g.run;
  const unsigned L = (unsigned) g.L, M = (unsigned) g.M;
  // The input of a tile is loaded into registers while the tile before it is computed, so that the memory latency hides behind the sums: with a
  // large table in LDS there is one workgroup a CU and nothing else to hide it.
  float stage[kSrcStage];
  auto load = [&](const SrcTile& k) {
#pragma unroll
    for (int e = 0; e < kSrcStage; e++) { const int s = tid + e * kSrcThreads; stage[e] = s < k.span ? src_fetch(x, hist, g.H, k.lo + s, r.nIn) : 0.0f; }
  };
  SrcTile cur = src_tile(g, r, chunk, 0);
  if (XLDS && cur.live) load(cur);
  if (TABLE == TBL_LDS) for (int s = tid; s < g.L * g.stride; s += kSrcThreads) tl[s] = g.table[s];
  for (int t = 0; cur.in; t++) {
    const SrcTile nxt = src_tile(g, r, chunk, t + 1);
    if (!cur.live) { for (long o = cur.o0 + tid; o < cur.oEnd; o += kSrcThreads) y[o] = 0.0f; cur = nxt; continue; }
    if (XLDS) {
      __syncthreads();                                                 // the previous tile is read and copied out
#pragma unroll
      for (int e = 0; e < kSrcStage; e++) { const int s = tid + e * kSrcThreads; if (s < cur.span) xs[s] = stage[e]; }
      __syncthreads();                                                 // (before the first tile: the table is written, too)
      if (nxt.live) load(nxt);
    }
    // Slot s of the tile forms output (s lanePitch) mod run: run is a power of two and lanePitch odd, so every output has one slot.  The pitch
    // spreads the windows and the table rows of the 32 lanes of an LDS cycle over the banks (src_lane_pitch); the outputs go through LDS
    // so that they still leave in order, coalesced.  A lane forms two outputs at a time, four independent chains: the LDS latency of one
    // hides behind the others.  A slot without an output sums row 0 over the span's first samples and drops the result.
    for (int s = tid; s < g.run; s += 2 * kSrcThreads) {
      unsigned i[2], off[2] = {0, 0}, q[2] = {0, 0}; bool out[2], live[2];
#pragma unroll
      for (int e = 0; e < 2; e++) {
        const int se = s + e * kSrcThreads;
        i[e] = XLDS ? ((unsigned) se * (unsigned) g.lanePitch) & (unsigned) (g.run - 1) : (unsigned) se;
        out[e] = se < g.run && cur.o0 + i[e] < cur.oEnd; live[e] = out[e] && cur.o0 + i[e] < r.count;
        if (live[e]) { off[e] = (cur.p0 + i[e] * M) / L; q[e] = TABLE == TBL_UNIFORM ? 0u : (cur.q0 + i[e]) % L; }
      }
      const float* tb = TABLE == TBL_LDS ? tl : g.table;
      const float* h0 = tb + (size_t) q[0] * g.stride; const float* h1 = tb + (size_t) q[1] * g.stride;
      float a0 = 0.0f, b0 = 0.0f, a1 = 0.0f, b1 = 0.0f;
      if (XLDS) {
        const float* w0 = xs + off[0]; const float* w1 = xs + off[1];
#pragma unroll 4
        for (int jj = 0; jj < g.taps; jj += 2) {
          a0 = __fmaf_rn(h0[jj], w0[jj], a0); b0 = __fmaf_rn(h0[jj + 1], w0[jj + 1], b0);
          a1 = __fmaf_rn(h1[jj], w1[jj], a1); b1 = __fmaf_rn(h1[jj + 1], w1[jj + 1], b1);
        }
      } else {
        for (int jj = 0; jj < g.taps; jj += 2) {
          a0 = __fmaf_rn(h0[jj], src_fetch(x, hist, g.H, cur.lo + off[0] + jj, r.nIn), a0);
          b0 = __fmaf_rn(h0[jj + 1], src_fetch(x, hist, g.H, cur.lo + off[0] + jj + 1, r.nIn), b0);
          a1 = __fmaf_rn(h1[jj], src_fetch(x, hist, g.H, cur.lo + off[1] + jj, r.nIn), a1);
          b1 = __fmaf_rn(h1[jj + 1], src_fetch(x, hist, g.H, cur.lo + off[1] + jj + 1, r.nIn), b1);
        }
      }
      const float acc[2] = {live[0] ? __fadd_rn(a0, b0) : 0.0f, live[1] ? __fadd_rn(a1, b1) : 0.0f};
#pragma unroll
      for (int e = 0; e < 2; e++) if (out[e]) { if (XLDS) ys[i[e]] = acc[e]; else y[cur.o0 + i[e]] = acc[e]; }
    }
    if (XLDS) {
      __syncthreads();
      for (long o = cur.o0 + tid; o < cur.oEnd; o += kSrcThreads) y[o] = ys[o - cur.o0];
    }
    cur = nxt;
  }
}

// zoh: y[n] = x[base]; linear: y[n] = x[base] + f (x[base+1] - x[base]), f = float(p) / float(L), every operation rounded to fp32 on its own
__global__ __launch_bounds__(256) void k_src_simple(SrcArgs g)
{
  const int row = blockIdx.y, u = row / g.C;
  const long o = (long) blockIdx.x * 256 + threadIdx.x;
  const SrcRange r = src_range(g, u);
  if (o == 0 && g.nout && row % g.C == 0) g.nout[u] = r.count;
  if (o >= g.outStride) return;
  float v = 0.0f;
  if (o < r.count) {
    const float* x = g.x + (size_t) row * g.inStride; const float* hist = g.hist ? g.hist + (size_t) row * g.H : nullptr;
    const int64_t t = (r.n0 + o) * g.M, base = t / g.L; const int p = (int) (t % g.L);
    const long rel = (long) (base - r.a);
    const float x0 = src_fetch(x, hist, g.H, rel, r.nIn);
    v = x0;
    if (g.linear) {
      const float x1 = src_fetch(x, hist, g.H, rel + 1, r.nIn), f = __fdiv_rn((float) p, (float) g.L);
      v = __fadd_rn(x0, __fmul_rn(f, __fsub_rn(x1, x0)));
    }
  }
  g.y[(size_t) row * g.outStride + o] = v;
}

// the last H samples of the stream after this block, in place: passes of 256 in ascending order, every pass reads before it writes, and what a pass
// reads of the old history lies at or above its own first entry, which no earlier pass has written
__global__ __launch_bounds__(256) void k_src_hist(SrcArgs g)
{
  const int row = blockIdx.x, u = row / g.C, tid = threadIdx.x;
  const SrcRange r = src_range(g, u);
  if (r.nIn == 0) return;
  const float* x = g.x + (size_t) row * g.inStride; float* hist = g.hist + (size_t) row * g.H;
  for (int k0 = 0; k0 < g.H; k0 += 256) {
    const int k = k0 + tid; const long rel = (long) r.nIn - g.H + k;
    float v = 0.0f;
    if (k < g.H) v = rel >= 0 ? x[rel] : hist[k + r.nIn];
    __syncthreads();
    if (k < g.H) hist[k] = v;
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void k_src_counts(SrcArgs g, int U)
{
  const int u = blockIdx.x * 256 + threadIdx.x;
  if (u >= U) return;
  const SrcRange r = src_range(g, u);
  g.cnt[u].nin = r.a + r.nIn; g.cnt[u].nout = r.n0 + r.count;
}

// The pitch between the outputs of neighbouring lanes: the odd pitch below 128 for which the 32 lanes of an LDS cycle meet the fewest times on a
// bank, counted over their input windows (start floor(i M / L)) and, with the table in LDS, over their table rows (start (i mod L) stride).
// Lanes on one address share a broadcast and do not count.
static int src_lane_pitch(const SrcState& s, bool tableInLds)
{
  auto worst = [&](int pitch, int first, bool rows) {
    int n[32] = {0}; long seen[32][32]; int w = 0;
    for (int l = 0; l < 32; l++) {
      const long i = (long) (first + l) * pitch, a = rows ? (i % s.L) * s.stride : i * s.M / s.L; const int b = (int) (a & 31);
      bool dup = false; for (int k = 0; k < n[b]; k++) dup = dup || seen[b][k] == a;
      if (!dup) { seen[b][n[b]++] = a; if (n[b] > w) w = n[b]; }
    }
    return w;
  };
  int best = 1; long bestCost = -1;
  for (int pitch = 1; pitch < 128; pitch += 2) {
    long cost = 0;
    for (int first : {0, 32, 480, 992}) cost += worst(pitch, first, false) + (tableInLds ? worst(pitch, first, true) : 0);
    if (bestCost < 0 || cost < bestCost) { best = pitch; bestCost = cost; }
  }
  return best;
}

SrcPath src_path(const SrcState& s)
{
  SrcPath r = {DSR_SRC_TABLE_NONE, DSR_SRC_INPUT_DIRECT, 256, 0, 1};
  if (s.method > SRC_BEST || s.copy) return r;
  const char* e = getenv("DSR_SRC_TABLE"); const bool forceMem = e && !strcmp(e, "mem");
  const char* er = getenv("DSR_SRC_RUN"); const int maxRun = er ? atoi(er) : 0;                     // a smaller tile, for tests of the tile split
  const size_t tbl = (size_t) s.L * s.stride * sizeof(float);
  auto tile = [&](int run) { return (size_t) (((int64_t) (run - 1) * s.M + s.L - 1) / s.L + s.taps + run) * sizeof(float); };   // the span and the outputs
  auto allowed = [&](int run) {                                        // the switch, and a span that the lanes' stage registers hold
    return (maxRun <= 0 || run <= maxRun || run == 256) && ((int64_t) (run - 1) * s.M + s.L - 1) / s.L + s.taps <= (int64_t) kSrcStage * kSrcThreads;
  };
  r.input = DSR_SRC_INPUT_LDS;
  if (s.L == 1 && !forceMem) r.table = DSR_SRC_TABLE_UNIFORM;
  else {
    r.table = DSR_SRC_TABLE_MEM;
    for (int run : {2048, 1024, 512, 256})
      if (!forceMem && allowed(run) && tbl + tile(run) <= kSrcLds) { r.table = DSR_SRC_TABLE_LDS; r.run = run; r.ldsBytes = tbl + tile(run); r.lanePitch = src_lane_pitch(s, true); return r; }
  }
  for (int run : {2048, 1024, 512, 256}) if (allowed(run) && tile(run) <= kSrcTileLds) { r.run = run; r.ldsBytes = tile(run); r.lanePitch = src_lane_pitch(s, false); return r; }
  r.input = DSR_SRC_INPUT_DIRECT; r.run = 1024; r.ldsBytes = 0;
  return r;
}

void src_launch(SrcState& s, const float* x, const int32_t* nsamp, int U, int C, long inStride, void* state, int flush, float* y, int32_t* nout,
                long outStride, hipStream_t st)
{
  const SrcPath p = src_path(s);
  SrcArgs g;
  g.x = x; g.nsamp = nsamp; g.y = y; g.nout = nout; g.cnt = (SrcCount*) state; g.H = s.hist();
  g.hist = state && g.H ? (float*) ((char*) state + (size_t) U * sizeof(SrcCount)) : nullptr;
  g.table = s.d_table.p; g.inStride = inStride; g.outStride = outStride; g.C = C; g.L = s.L; g.M = s.M; g.K = s.K; g.taps = s.taps; g.stride = s.stride;
  g.flush = flush; g.run = p.run; g.linear = s.method == SRC_LINEAR && !s.copy; g.tilesPerBlock = 1; g.chunks = 1; g.lanePitch = 1;
  const long rows = (long) U * C;
  if (p.table == DSR_SRC_TABLE_NONE) {
    if (rows > 65535) throw Error(DSR_E_DIMENSION, "SampleRateConverter: %ld rows, at most 65535 for zoh, linear and equal rates", rows);
    launch(k_src_simple, dim3(cdiv(outStride > 0 ? outStride : 1, 256), (unsigned) rows), dim3(256), 0, st, g);
  } else {
    const long tiles = cdiv(outStride > 0 ? outStride : 1, p.run);
    long tpb = rows * tiles / 2048; tpb = tpb < 1 ? 1 : tpb > 16 ? 16 : tpb;      // enough workgroups to fill the device, then longer walks per table copy
    if (const char* et = getenv("DSR_SRC_TILES")) { const int v = atoi(et); if (v >= 1 && v <= 16) tpb = v; }          // for tests of the walk
    g.tilesPerBlock = (int) tpb; g.chunks = cdiv(tiles, tpb);
    if (rows * g.chunks > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "SampleRateConverter: %ld rows of %ld tiles are too many workgroups", rows, tiles);
    const dim3 grid((unsigned) (rows * g.chunks)), block(kSrcThreads);
    const bool xl = p.input == DSR_SRC_INPUT_LDS;
    g.lanePitch = p.lanePitch;
    if (p.table == DSR_SRC_TABLE_LDS) launch(k_src_sinc<TBL_LDS, true>, grid, block, p.ldsBytes, st, g);
    else if (p.table == DSR_SRC_TABLE_UNIFORM && xl) launch(k_src_sinc<TBL_UNIFORM, true>, grid, block, p.ldsBytes, st, g);
    else if (p.table == DSR_SRC_TABLE_UNIFORM) launch(k_src_sinc<TBL_UNIFORM, false>, grid, block, 0, st, g);
    else if (xl) launch(k_src_sinc<TBL_MEM, true>, grid, block, p.ldsBytes, st, g);
    else launch(k_src_sinc<TBL_MEM, false>, grid, block, 0, st, g);
  }
  if (state) {
    if (g.H) launch(k_src_hist, dim3((unsigned) rows), dim3(256), 0, st, g);
    launch(k_src_counts, dim3(cdiv(U, 256)), dim3(256), 0, st, g, U);
  }
}

}  // namespace dsr
