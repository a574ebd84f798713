// csrc/multistream.h -- multi-stream decoding (include/dsr.h section 8b): what ms_kernels.hip, multistream.cpp and streams_asr.cpp share.
#pragma once
#include "common.h"

struct dsr_stream;

// The combiner: the resolved table [KA] of video state indices, on the host and on the device, and the two stream weights.
struct dsr_ms {
  int KA = 0, KV = 0; double wA = 0.95, wV = 0.05;
  std::vector<int> table; dsr::DevBuf<int> d_table;
};

// A distribution set as the decoder sees it (include/dsr.h section 8).  A plain set is a GMM bound to a feature stream; a multi-stream set
// (ms != nullptr) has no model or stream of its own: names and count are the audio child's, every score is the combiner's.
struct dsr_distribset {
  int refs = 1;                                          // the creator's reference, and one per multi-stream set built on this one
  dsr_gmm* gmm = nullptr; dsr_stream* feat = nullptr; int mode = 0;
  dsr_distribset* audio = nullptr; dsr_distribset* video = nullptr; dsr_ms* ms = nullptr;
  int cachedFrame = -1; bool hostRow = false;            // d_row holds frame cachedFrame; row is its host copy when hostRow
  std::vector<float> row; dsr::DevBuf<float> d_row, d_scores; dsr::DevBuf<int> d_T;
};

namespace dsr {

// The dispatch of k_ms_combine, a pure function of (KA, KV, alignment).  The launch and dsr_ms_combine_path both ask here.
// Tile height, measured at [998000][1024]: 2 rows of 1024 video states and 4 rows of 64 are the fastest, taller tiles lose
// 5 - 8 %: a workgroup stages before it streams, and short tiles keep more workgroups of a CU in different phases.  So a tile holds up to
// kMsTileBytes of video rows and at most kMsMaxRows rows.
struct MsPath { int path; int rows; int64_t ldsBytes; };
constexpr int kMsMaxRows = 4;
constexpr int64_t kMsTileBytes = 8192;
inline MsPath ms_path(int KA, int KV, bool aligned16)
{
  const int64_t rowBytes = 4 * (int64_t) KV;
  MsPath p; p.ldsBytes = 0;
  p.rows = (int) (kMsTileBytes / rowBytes); if (p.rows > kMsMaxRows) p.rows = kMsMaxRows; if (p.rows < 1) p.rows = 1;
  if (rowBytes > DSR_MS_LDS_BUDGET) { p.path = DSR_MS_GATHER; return p; }
  p.ldsBytes = ((p.rows * rowBytes + 15) / 16) * 16 + 16;                    // the tile at its phase within a 16-byte word: up to 12 bytes in front
  p.path = (KA % 4 == 0 && aligned16) ? DSR_MS_VECTOR_LDS : DSR_MS_SCALAR_LDS;
  return p;
}

// out[n][k] = float(wA * double(sA[n][k]) + wV * double(sV[n][map[k]])); out == sA or disjoint from both (ms_kernels.hip)
void ms_combine(const float* sA, const float* sV, const int* map, int64_t N, int KA, int KV, double wA, double wV, float* out, hipStream_t st);

}  // namespace dsr
