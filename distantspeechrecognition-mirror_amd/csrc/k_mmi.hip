// csrc/k_mmi.hip -- the frame loop of SubbandMMI (next / calcInterferenceOutputs / binaryMasking, btk/beamformer/beamformer.cc:1973-2319;
// ZelinskiFilter(_f), btk/postfilter/postfilter.cc:59-221): one generalized sidelobe canceller per sound source, the target's output
// post-filtered (Zelinski) and optionally masked against the other sources' outputs.  The weights and the dsr_mmi_* entries: csrc/mmi.cpp.
//
// k_mmi: one workgroup per utterance, a thread per frequency bin walking the frames -- the post-filter's spectral densities and the
// mask's averaged output are first-order recursions over time, independent across bins (the averaged output couples neighbouring bins only
// when useBinaryMask's fwidth > 1: those frames take a workgroup barrier and one thread does the bins in order, as the reference's loop).
// fp64 arithmetic in the reference's order on the pipe's complex64 snapshots (-ffp-contract=off).
//
// The TYPE_APAB post-filter (beamformer.cc:2047-2049, 2177-2179; ApabFilter / ApabFilter_f postfilter.cc:225-340, always called with channelX =
// chanN/2) filters the bins below fftLen/2 only (with halfBandShift it mirrors the weights onto fftLen-1-k): without halfBandShift its output vector
// is not conjugate-symmetric, so in that configuration the kernel writes all fftLen bins of a frame (dsr_mmi_out_bins) -- the upper ones as the
// reference leaves them: the conjugate of the UNFILTERED lower bin, or, where the mask struck, the mask's value itself, unconjugated (:2302-2304).
// In every other configuration the half spectrum is handed on and the mask's averaged value lands in bin k only.
#include "launch.h"
#include "mmi.h"

namespace dsr {

// ---------------------------------------------------------------------------------------------------------------------------------
// The frame loop.  X [U][C][Tmax][F] complex64 snapshots, Y [U][Tmax][F].  weff / wup / mani: [S][F][C] fp64 complex (entire weight
// wq - wl with bin 0's wq alone when !hbs; upper branch wq; the post-filter's steering vectors).  csd: [S][U][C*C][F] spectral densities
// (only the i <= j entries are used).  taScr: [U][F][C] scratch for arrays above 16 channels.
template <int CT>
__global__ __launch_bounds__(256) void k_mmi(const float2* __restrict__ X, const int* __restrict__ nframesArr, const double2* __restrict__ weff,
                                             const double2* __restrict__ wup, const double2* __restrict__ mani, double2* __restrict__ csd,
                                             double2* __restrict__ taScr, float2* __restrict__ Y, int U, int C, int Tmax, int F, int S, int target,
                                             int hbs, int pfType, double alphaCfg, int useMask, int maskType, double avgFactor, int fwidth, int M, int Fout)
{
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  double2* avgOut = reinterpret_cast<double2*>(smem);             // [F] _avgOutput
  double2* outS = avgOut + F;                                     // [F] this frame's output (fwidth > 1 only)
  double2* mirS = outS + F;                                       // [F] what bin M - f of a full output frame holds unless the mask strikes (fwidth > 1 only)
  int* maskS = reinterpret_cast<int*>(mirS + F);                  // [F] target weaker than an interferer
  const int u = blockIdx.x, tid = threadIdx.x, nthr = blockDim.x;
  const int T = nframesArr[u] < Tmax ? nframesArr[u] : Tmax;
  const float2* Xu = X + (size_t) u * C * Tmax * F;
  float2* Yu = Y + (size_t) u * Tmax * Fout;
  for (int f = tid; f < F; f += nthr) avgOut[f] = make_double2(0.0, 0.0);
  __syncthreads();
  const bool apab = (pfType & 0x04) != 0;                         // tested first (beamformer.cc:2047)
  const bool zel = !apab && ((pfType & 0x01) || (pfType & 0x02));
  const bool fullOut = Fout > F;                                  // APAB without halfBandShift: all M bins of a frame are written
  const int M2 = M / 2;
  const bool wide = useMask && avgFactor >= 0.0 && fwidth > 1;
  const int NE = C * C;
  double2 taR[CT > 0 ? CT : 1];


  for (int t = 0; t < Tmax; t++) {
    if (t >= T) { for (int f = tid; f < Fout; f += nthr) Yu[(size_t) t * Fout + f] = make_float2(0.f, 0.f); continue; }   // (uniform: T is per utterance)
    const int frameX = t - 1;                                      // _frameX when next() runs (FrameResetX = -1)
    const double alpha = (frameX > 0) ? alphaCfg : 0.0;            // beamformer.cc:2042-2045
    const int type = (frameX < 0) ? 0 : pfType;                    // MINFRAMES 0 (:1136): the first frame only updates the densities
    for (int f = tid; f < F; f += nthr) {
      // ---- outputs of the target and, for the mask, of the other sources
      double2* ta = CT > 0 ? taR : taScr + ((size_t) u * F + f) * C;
      double tr = 0.0, ti = 0.0;                                   // target output
      double tgtPow = 0.0, maxPow = 0.0;
      auto dotAt = [&](const double2* w, const int fb, double& yr, double& yi) {   // sum_c conj(w_c) x_c at bin fb, products as gsl_complex_mul
        yr = 0.0; yi = 0.0;
        for (int c = 0; c < C; c++) {
          const float2 x = Xu[((size_t) c * Tmax + t) * F + fb]; const double wr = w[c].x, wi = -w[c].y;
          yr += wr * (double) x.x - wi * (double) x.y; yi += wr * (double) x.y + wi * (double) x.x;
        }
      };
      auto dot = [&](const double2* w, double& yr, double& yi) { dotAt(w, f, yr, yi); };
      // ApabFilter_f (postfilter.cc:225-264) for source s at bin fb, whose beamformed value there is (yr, yi): |y|^2 over the power of the
      // time-aligned channel chanN/2, cut at 1
      auto apabW = [&](const int s, const int fb, const double yr, const double yi) -> double {
        const int ch = C / 2;
        const double2 d = mani[((size_t) s * F + fb) * C + ch]; const float2 x = Xu[((size_t) ch * Tmax + t) * F + fb];
        const double dr = d.x, di = -d.y;
        const double pr = dr * (double) x.x - di * (double) x.y, pi = dr * (double) x.y + di * (double) x.x;
        const double pxx = pr * pr + pi * pi, pyy = yr * yr + yi * yi;
        double W = pyy / pxx;
        if (W >= 1.0) W = 1.0;
        if (W <= -1.0) W = -1.0;
        return W;
      };
      // ApabFilter (postfilter.cc:275-340) on bin f of source s's vector (computed with the weights wsel [S][F][C]): bins below M/2 take their own
      // weight; with halfBandShift bin f >= M/2 takes the weight of bin M-1-f (from that bin's snapshot, manifold and beamformed value); without it
      // bins >= M/2 are left alone
      auto apabApply = [&](const int s, const double2* wsel, double& yr, double& yi) {
        double W;
        if (f < M2) W = apabW(s, f, yr, yi);
        else if (hbs) { const int fb = M - 1 - f; double br, bi; dotAt(wsel + ((size_t) s * F + fb) * C, fb, br, bi); W = apabW(s, fb, br, bi); }
        else return;
        const double a = W * yr - 0.0 * yi, b = W * yi + 0.0 * yr; yr = a; yi = b;
      };
      auto pfw = [&](int s) -> double {                            // ZelinskiFilter for source s at this bin: returns the weight (1 when unused)
        if (!zel) return 1.0;
        const double2* d = mani + ((size_t) s * F + f) * C;
        for (int c = 0; c < C; c++) {                              // TimeAlignment: conj(d_c) x_c
          const float2 x = Xu[((size_t) c * Tmax + t) * F + f]; const double dr = d[c].x, di = -d[c].y;
          ta[c] = make_double2(dr * (double) x.x - di * (double) x.y, dr * (double) x.y + di * (double) x.x);
        }
        double2* st = csd + ((size_t) s * U + u) * NE * F + f;
        double sr = 0.0, si = 0.0;
        for (int i = 0; i < C - 1; i++)
          for (int j = i + 1; j < C; j++) {
            const double ar = ta[i].x, ai = ta[i].y, br = ta[j].x, bi = -ta[j].y;
            const double pr = ar * br - ai * bi, pi = ar * bi + ai * br;
            double er = pr, ei = pi;
            const size_t e = (size_t) (i * C + j) * F;
            if (alpha > 0.0) { const double2 p = st[e]; er = p.x * alpha + pr * (1.0 - alpha); ei = p.y * alpha + pi * (1.0 - alpha); }
            sr += er; si += ei; st[e] = make_double2(er, ei);
          }
        double numerator;
        if (1 & type) { numerator = sr; if (numerator < 0.0) numerator = 0.0; } else numerator = hypot(sr, si);
        double denominator = 0.0;
        for (int i = 0; i < C; i++) {
          const double a2 = ta[i].x * ta[i].x + ta[i].y * ta[i].y;
          const size_t e = (size_t) (i * C + i) * F;
          double est = a2;
          if (alpha > 0.0) est = alpha * st[e].x + (1.0 - alpha) * a2;
          denominator += est; st[e] = make_double2(est, 0.0);
        }
        double W = (numerator / denominator) * (2.0 / ((double) C - 1.0));
        if (W >= 1.0) W = 1.0;
        if (W < 0.0001) W = 0.0001;
        return W;                                                  // (type 0 = NO_USE_POST_FILTER: the densities are updated, the caller does not filter)
      };
      dot(weff + ((size_t) target * F + f) * C, tr, ti);
      const double ur = tr, ui = ti;                               // before the post-filter: what the mirror bin of a full frame keeps
      const bool filt = zel && type != 0;
      if (apab) apabApply(target, weff, tr, ti);
      else { const double W = pfw(target); if (filt) { const double a = W * tr - 0.0 * ti, b = W * ti + 0.0 * tr; tr = a; ti = b; } }   // polar(W, 0) * y
      bool masked = false;
      const bool maskBin = useMask && (hbs || f >= 1);             // bin 0 is never masked (:2283), but calcInterferenceOutputs runs its post-filters too:
      if (useMask) {                                               // with mask type 1 that is the second update of the target's densities in this frame
        for (int s = 0; s < S; s++) {
          if (maskType == 0 && s == target) continue;
          double yr, yi;
          dot((maskType == 0 ? weff : wup) + ((size_t) s * F + f) * C, yr, yi);
          if (apab) apabApply(s, maskType == 0 ? weff : wup, yr, yi);
          else { const double W = pfw(s); if (filt) { const double a = W * yr - 0.0 * yi, b = W * yi + 0.0 * yr; yr = a; yi = b; } }
          const double p = yr * yr + yi * yi;
          if (s == target) tgtPow = p; else if (p > maxPow) maxPow = p;
        }
        if (maskType == 0) tgtPow = tr * tr + ti * ti;             // _interferenceOutputs[target] = the post-filtered output (:2064-2065)
        masked = maskBin && tgtPow < maxPow;
      }
      const bool mir = fullOut && f >= 1 && f < M2;                // bin M - f of a full frame: conj of the unfiltered value (:2026-2027) unless the mask strikes
      if (!maskBin) { Yu[(size_t) t * Fout + f] = make_float2((float) tr, (float) ti); if (mir) Yu[(size_t) t * Fout + (M - f)] = make_float2((float) ur, (float) -ui); }
      else if (!wide) {
        // binaryMasking (:2241-2319) for one bin: the averaged output is this bin's own recursion
        double nr = 0.0, ni = 0.0;
        if (avgFactor >= 0.0) { nr = avgOut[f].x * avgFactor; ni = avgOut[f].y * avgFactor; }
        if (masked) { tr = nr; ti = ni; if (avgFactor >= 0.0) avgOut[f] = make_double2(nr, ni); }
        else if (avgFactor >= 0.0) avgOut[f] = make_double2(avgOut[f].x * avgFactor + tr * (1.0 - avgFactor), avgOut[f].y * avgFactor + ti * (1.0 - avgFactor));
        Yu[(size_t) t * Fout + f] = make_float2((float) tr, (float) ti);
        if (mir) Yu[(size_t) t * Fout + (M - f)] = masked ? make_float2((float) tr, (float) ti) : make_float2((float) ur, (float) -ui);
      } else { outS[f] = make_double2(tr, ti); maskS[f] = masked ? 1 : 0; mirS[f] = make_double2(ur, -ui); }
    }
    if (wide) {
      // the mean over neighbouring bins reads values this frame's loop has already replaced below the bin and last frame's above it
      // (getMeanOfSubbandC on _avgOutput while it is being updated, :2212-2231): one thread, bins in order
      __syncthreads();
      if (tid == 0) {
        const int f0 = hbs ? 0 : 1, f1 = hbs ? M - 1 : M / 2, lim = hbs ? M : M / 2;
        for (int f = f0; f <= f1; f++) {
          int fs = f - fwidth / 2; if (fs < 1) fs = 1;
          int fe = f + fwidth / 2; if (fe >= lim) fe = lim - 1;
          double sr = 0.0, si = 0.0; unsigned cnt = 0;
          for (int i = fs; i <= fe; i++, cnt++) { sr += avgOut[i].x; si += avgOut[i].y; }
          const double nr = (sr / (double) cnt) * avgFactor, ni = (si / (double) cnt) * avgFactor;
          if (maskS[f]) { outS[f] = make_double2(nr, ni); avgOut[f] = make_double2(nr, ni); }
          else avgOut[f] = make_double2(avgOut[f].x * avgFactor + outS[f].x * (1.0 - avgFactor), avgOut[f].y * avgFactor + outS[f].y * (1.0 - avgFactor));
        }
      }
      __syncthreads();
      for (int f = tid; f < F; f += nthr) if (hbs || f >= 1) {
        Yu[(size_t) t * Fout + f] = make_float2((float) outS[f].x, (float) outS[f].y);
        if (fullOut && f < M2) { const double2 v = maskS[f] ? outS[f] : mirS[f]; Yu[(size_t) t * Fout + (M - f)] = make_float2((float) v.x, (float) v.y); }
      }
    }
  }
}

void mmi_launch(dsr_mmi& m, const float* X, const int* nf, int U, int Tmax, float* Y, hipStream_t st)
{
  const int M = m.M, C = m.C, S = m.S, F = m.hbs ? M : M / 2 + 1;
  const bool zel = !(m.pfType & 0x04) && ((m.pfType & 0x01) || (m.pfType & 0x02));
  m.d_csd.reserve(zel ? (size_t) S * U * C * C * F : 1);
  if (C > 16) m.d_ta.reserve((size_t) U * F * C);
  const size_t lds = (size_t) F * (3 * sizeof(double2) + sizeof(int));
  if (lds > 150 * 1024) throw Error(DSR_E_DIMENSION, "SubbandMMI: %d bins need %zu bytes of LDS", F, lds);
  for_value(ints<16, 0>{}, C <= 16 ? 16 : 0, [&](auto cap) {   // a thread's vectors in registers up to 16 channels
    launch(k_mmi<cap()>, dim3(U), dim3(256), lds, st, (const float2*) X, nf, m.d_weff.p, m.d_wup.p, m.d_mani.p, m.d_csd.p, m.d_ta.p, (float2*) Y, U, C, Tmax, F, S,
           m.target, m.hbs, m.pfType, m.alpha, m.useMask ? 1 : 0, (int) m.maskType, m.avgFactor, (int) m.fwidth, M, dsr_mmi_out_bins(&m)); });
}

}  // namespace dsr
