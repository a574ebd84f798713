// csrc/ms_kernels.hip -- the multi-stream combination of two score matrices (include/dsr.h section 8b).
//
// Replaces DistribMultiStream::_score (asr/gaussian/distribBasic.h:148-152) for every (frame, state) at once:
//     out[n][k] = float(wA * double(sA[n][k]) + wV * double(sV[n][map[k]]))
// two fp64 products, one fp64 sum, one rounding to float -- the reference is built without fused multiply-add, and so is this translation unit
// (-ffp-contract=off): neither product is contracted into the sum.  map[k] in [0, KV) names the video state of audio state k; many audio states
// may share one.  out is sA itself (a pipe has no use for the audio-only matrix afterwards) or disjoint from both inputs.
//
// The kernel moves 4 N (2 KA + KV) bytes and does three fp64 operations an element: it is bound by HBM traffic, so every byte of sA and sV is
// read from memory once and out is written once.
//
//   k_ms_combine<W, STAGED>   one workgroup of 256 threads per tile of R consecutive rows.
//     STAGED: the tile's video rows -- R KV consecutive floats of sV -- are copied to LDS with 16-byte loads.  The copy keeps the phase the tile
//             has within a 16-byte word of memory (lds[ph + i] = tile[i], ph = the tile's address / 4 mod 4), so every full word is one aligned
//             float4 load and one aligned ds_write_b128 whatever KV and the alignment of sV are; the words at the two ends that the tile covers
//             in part are copied float by float, and nothing outside the tile is read.  The many-to-one gather sV[n][map[k]] then reads LDS.
//     A thread owns the columns W (t + 256 j) ... + W - 1 of every row of the tile: their map entries are loaded once and stay in registers over
//             the rows, the audio rows stream through as float4 (W = 4) or float (W = 1), kUnroll rows' loads in flight before the first store
//             (in place a thread reads and writes its own elements only, so the order is safe).
//     !STAGED: one video row alone exceeds the LDS budget; sV[n][map[k]] is read from memory (W = 1).
//
// The dispatch is ms_path() (multistream.h): vector + LDS when KA % 4 == 0 and sA / out are 16-byte aligned, scalar + LDS for any other KA or
// 4-byte alignment, the global gather when 4 KV > DSR_MS_LDS_BUDGET.
#include "launch.h"
#include "multistream.h"

namespace dsr {

static constexpr int kMsThreads = 256, kMsUnroll = 4;

template <int W> struct MsVec;
template <> struct MsVec<1> { typedef float f; typedef int i; };
template <> struct MsVec<4> { typedef float4 f; typedef int4 i; };

template <int W, bool STAGED>
__global__ __launch_bounds__(kMsThreads) void k_ms_combine(const float* sA, const float* __restrict__ sV, const int* __restrict__ map, float* out,
                                                           long N, int KA, int KV, int R, double wA, double wV)
{
  extern __shared__ __attribute__((aligned(16))) float tile[];
  typedef typename MsVec<W>::f vf; typedef typename MsVec<W>::i vi;
  const long row0 = (long) blockIdx.x * R;
  const int rows = (int) (N - row0 < (long) R ? N - row0 : (long) R);
  const float* v = sV + (size_t) row0 * KV;                                   // the tile's video rows: rows * KV consecutive floats
  int ph = 0;
  if (STAGED) {
    ph = (int) ((reinterpret_cast<uintptr_t>(v) >> 2) & 3);
    const int n = rows * KV, words = (ph + n + 3) >> 2;
    for (int w = threadIdx.x; w < words; w += kMsThreads) {
      const int lo = 4 * w - ph;                                              // the tile element the word starts with
      if (lo >= 0 && lo + 4 <= n) reinterpret_cast<float4*>(tile)[w] = *reinterpret_cast<const float4*>(v + lo);
      else for (int j = 0; j < 4; j++) if (lo + j >= 0 && lo + j < n) tile[4 * w + j] = v[lo + j];
    }
    __syncthreads();
  }
  const int groups = (KA + W - 1) / W;
  for (int g = threadIdx.x; g < groups; g += kMsThreads) {
    const vi mv = reinterpret_cast<const vi*>(map)[g];
    int m[W]; memcpy(m, &mv, sizeof mv);
    for (int r0 = 0; r0 < rows; r0 += kMsUnroll) {
      vf av[kMsUnroll];
#pragma unroll
      for (int u = 0; u < kMsUnroll; u++)
        if (r0 + u < rows) av[u] = *reinterpret_cast<const vf*>(sA + (size_t) (row0 + r0 + u) * KA + (size_t) g * W);
#pragma unroll
      for (int u = 0; u < kMsUnroll; u++) {
        if (r0 + u >= rows) break;
        float a[W], o[W]; memcpy(a, &av[u], sizeof(vf));
#pragma unroll
        for (int j = 0; j < W; j++) {
          const float s = STAGED ? tile[ph + (r0 + u) * KV + m[j]] : sV[(size_t) (row0 + r0 + u) * KV + m[j]];
          o[j] = (float) (wA * (double) a[j] + wV * (double) s);
        }
        vf ov; memcpy(&ov, o, sizeof ov);
        *reinterpret_cast<vf*>(out + (size_t) (row0 + r0 + u) * KA + (size_t) g * W) = ov;
      }
    }
  }
}

void ms_combine(const float* sA, const float* sV, const int* map, int64_t N, int KA, int KV, double wA, double wV, float* out, hipStream_t st)
{
  if (N <= 0) return;
  const bool aligned16 = ((reinterpret_cast<uintptr_t>(sA) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  const MsPath p = ms_path(KA, KV, aligned16);
  const int64_t tiles = (N + p.rows - 1) / p.rows;
  if (tiles > 0x7fffffffL) throw Error(DSR_E_DIMENSION, "%lld rows in tiles of %d exceed the grid", (long long) N, p.rows);
  const dim3 grid((unsigned) tiles), block(kMsThreads);
  switch (p.path) {
    case DSR_MS_VECTOR_LDS: launch(k_ms_combine<4, true>, grid, block, (size_t) p.ldsBytes, st, sA, sV, map, out, N, KA, KV, p.rows, wA, wV); break;
    case DSR_MS_SCALAR_LDS: launch(k_ms_combine<1, true>, grid, block, (size_t) p.ldsBytes, st, sA, sV, map, out, N, KA, KV, p.rows, wA, wV); break;
    default:                launch(k_ms_combine<1, false>, grid, block, 0, st, sA, sV, map, out, N, KA, KV, p.rows, wA, wV); break;
  }
}

}  // namespace dsr
