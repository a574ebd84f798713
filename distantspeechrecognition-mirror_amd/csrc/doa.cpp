// csrc/doa.cpp -- host side of the linear-array steered-response-power estimator, DOAEstimatorSRPDSBLA (kernels: csrc/k_doa.hip; the handle and the
// launchers: csrc/srp_common.h).  Set-up work, as in the reference: the theta grid, the look delays and the steering table
// (_calcSteeringUnitTable :3105-3152, setLookDirection :3257-3271, calcMainlobe :531-594), the final N-best from the accumulators
// (_getNBestHypothesesFromACCRP :2986-3025), and the dsr_doa_* entries.  No HIP call is made by the set-up, so the table can be inspected without a GPU.
#include "srp_common.h"
#include <algorithm>
#include <cmath>
#include <complex>

using namespace dsr;

typedef std::complex<double> zc;

namespace {

int theta_n(const dsr_doa& s) { return (int) (unsigned) ((s.maxTheta - s.minTheta) / s.widthTheta + 0.5); }    // :3113

void look_delays(const dsr_doa& s, double theta, double* d)   // setLookDirection (:3257-3271): |x_c - x_0| cos(theta), x only, no speed of sound
{
  if (s.pos.empty()) throw Error(DSR_E_ERROR, "set the array geometry first (setArrayGeometry)");
  if ((int) s.pos.size() < s.C) throw Error(DSR_E_DIMENSION, "the array geometry has %d positions, the estimator %d channels", (int) s.pos.size(), s.C);
  const double ref = s.pos[0];
  d[0] = 0.0;
  for (int c = 1; c < s.C; c++) { double dist = s.pos[c] - ref; if (dist < 0) dist = -dist; d[c] = dist * cos(theta); }
}

void build_table(dsr_doa& s)                                 // _calcSteeringUnitTable (:3105-3152)
{
  if (s.tbl) return;
  check_range(s.fbinMin, s.fbinMax, s.M, s.M / 2);
  const int nT = theta_n(s), C = s.C, M = s.M, M2 = M / 2;
  if (nT < 1 || nT > 65536) throw Error(DSR_E_PARAMETER, "search grid of %d directions (minTheta %g, maxTheta %g, widthTheta %g)", nT, s.minTheta, s.maxTheta, s.widthTheta);
  std::vector<double> d(C);
  look_delays(s, s.minTheta, d.data());                      // geometry errors before anything changes
  s.thetas.assign(nT, 0.0); s.W.assign((size_t) (s.fbinMax + 1) * nT * C, zc(0, 0));
  const double fs = (double) s.sampleRate;
  double theta = s.minTheta;
  for (int k = 0; k < nT; k++, theta += s.widthTheta) {      // theta accumulated in double, as the reference's loop does
    s.thetas[k] = theta;
    look_delays(s, theta, d.data());
    for (int c = 0; c < C; c++) s.W[(size_t) k * C + c] = zc(1, 0);             // bin 0: (1, 0) unless the range starts at 0
    for (int f = s.fbinMin; f <= s.fbinMax; f++)                                // wq_f of calcMainlobe (:557-581)
      for (int c = 0; c < C; c++) {
        zc w;
        if (f == 0) w = std::polar(1.0, 0.0) / (double) C;
        else if (f < M2) { const double val = -2.0 * M_PI * f * d[c] * fs / M; w = std::polar(1.0, val) / (double) C; }
        else { const double val = -M_PI * fs * d[c]; w = std::polar(1.0, val) / (double) C; }
        s.W[((size_t) f * nT + k) * C + c] = w;
      }
  }
  s.nTheta = nT; s.tblFbinMax = s.fbinMax; s.tbl = true; s.tableGen++; s.dDirty = true;
}

}  // namespace

extern "C" {

dsr_status dsr_doa_create(int nBest, int sampleRate, int fftLen, int chanN, dsr_doa** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (nBest < 1) throw Error(DSR_E_PARAMETER, "nBest %d < 1", nBest);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_PARAMETER, "fftLen %d", fftLen);
    if (chanN < 1 || chanN > 128) throw Error(DSR_E_DIMENSION, "%d channels (1..128 supported)", chanN);
    if (sampleRate <= 0) throw Error(DSR_E_PARAMETER, "sampleRate %d", sampleRate);
    dsr_doa* s = new dsr_doa(); s->nBest = nBest; s->sampleRate = (unsigned) sampleRate; s->M = fftLen; s->C = chanN; s->fbinMax = fftLen / 2;
    *out = s;
  });
}
void dsr_doa_destroy(dsr_doa* s) { delete s; }
int dsr_doa_nbest(const dsr_doa* s) { return s ? s->nBest : 0; }
int dsr_doa_chan_n(const dsr_doa* s) { return s ? s->C : 0; }
int dsr_doa_fft_len(const dsr_doa* s) { return s ? s->M : 0; }
unsigned dsr_doa_table_generation(const dsr_doa* s) { return s ? s->tableGen : 0u; }
int dsr_doa_has_table(const dsr_doa* s) { return s && s->tbl ? 1 : 0; }

dsr_status dsr_doa_set_array_geometry(dsr_doa* s, const double* positions, int n)
{
  return guard([&] {
    if (!s || !positions || n < 1) throw Error(DSR_E_PARAMETER, "null argument");
    s->pos.assign(positions, positions + n);                 // the table is not rebuilt (the reference neither)
  });
}
dsr_status dsr_doa_set_search_param(dsr_doa* s, double minTheta, double maxTheta, double widthTheta)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (!(widthTheta > 0.0)) throw Error(DSR_E_PARAMETER, "widthTheta %g must be positive", widthTheta);
    if (minTheta > maxTheta) { fprintf(stderr, "Invalid argument\n"); std::swap(minTheta, maxTheta); }   // beamformer.h:531-537
    s->minTheta = minTheta; s->maxTheta = maxTheta; s->widthTheta = widthTheta;
    s->tbl = false; s->thetas.clear(); s->W.clear(); s->nTheta = 0;     // clearTable (:2962-2984)
  });
}
dsr_status dsr_doa_set_frequency_range(dsr_doa* s, int fbinMin, int fbinMax)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if (fbinMin < 0 || fbinMin > fbinMax || fbinMax > s->M / 2) throw Error(DSR_E_DIMENSION, "frequency range [%d, %d] outside [0, %d]", fbinMin, fbinMax, s->M / 2);
    s->fbinMin = fbinMin; s->fbinMax = fbinMax;
  });
}
dsr_status dsr_doa_frequency_range(const dsr_doa* s, int* fbinMin, int* fbinMax)
{ return guard([&] { if (!s || !fbinMin || !fbinMax) throw Error(DSR_E_PARAMETER, "null argument"); *fbinMin = s->fbinMin; *fbinMax = s->fbinMax; }); }
dsr_status dsr_doa_set_energy_threshold(dsr_doa* s, float threshold)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->threshold = threshold; }); }
float dsr_doa_energy_threshold(const dsr_doa* s) { return s ? s->threshold : 0.0f; }

dsr_status dsr_doa_theta_n(dsr_doa* s, int* n)
{
  return guard([&] {
    if (!s || !n) throw Error(DSR_E_PARAMETER, "null argument");
    *n = s->tbl ? s->nTheta : theta_n(*s);
  });
}
dsr_status dsr_doa_thetas(dsr_doa* s, double* out, int n)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    const int nT = s->tbl ? s->nTheta : theta_n(*s);
    if (n < nT) throw Error(DSR_E_DIMENSION, "room for %d directions, the grid has %d", n, nT);
    double theta = s->minTheta;
    for (int k = 0; k < nT; k++, theta += s->widthTheta) out[k] = theta;
  });
}
dsr_status dsr_doa_look_delays(dsr_doa* s, double theta, double* delays)
{ return guard([&] { if (!s || !delays) throw Error(DSR_E_PARAMETER, "null argument"); look_delays(*s, theta, delays); }); }
dsr_status dsr_doa_build_table(dsr_doa* s)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); build_table(*s); }); }
dsr_status dsr_doa_srp_cell(dsr_doa* s, int cell[3], int64_t* ldsBytes)
{
  return guard([&] {
    if (!s || !cell) throw Error(DSR_E_PARAMETER, "null argument");
    build_table(*s);
    const SrpCell c = doa_srp_cell(s->nTheta, s->C);
    cell[0] = c.TG; cell[1] = c.BC; cell[2] = c.KS;
    if (ldsBytes) *ldsBytes = (int64_t) c.ldsBytes;
  });
}
dsr_status dsr_doa_steering(dsr_doa* s, int thetaX, double* out, size_t outDoubles)
{
  return guard([&] {
    if (!s || !out) throw Error(DSR_E_PARAMETER, "null argument");
    build_table(*s);
    if (thetaX < 0 || thetaX >= s->nTheta) throw Error(DSR_E_INDEX, "direction %d of %d", thetaX, s->nTheta);
    const int F = s->M / 2 + 1, C = s->C;
    if (outDoubles < (size_t) F * C * 2) throw Error(DSR_E_DIMENSION, "output holds %zu doubles, %d needed", outDoubles, F * C * 2);
    for (int f = 0; f < F; f++)
      for (int c = 0; c < C; c++) {
        const zc w = f <= s->tblFbinMax ? s->W[((size_t) f * s->nTheta + thetaX) * C + c] : zc(0, 0);
        out[((size_t) f * C + c) * 2] = w.real(); out[((size_t) f * C + c) * 2 + 1] = w.imag();
      }
  });
}

dsr_status dsr_doa_srp(dsr_doa* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, float* energy_dev, double* rp_dev,
                       double* nbest_rp_dev, int32_t* nbest_idx_dev, double* acc_dev, float* Y_dev, int32_t* gated_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !nframes_dev || !energy_dev || !nbest_rp_dev || !nbest_idx_dev || !acc_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "U %d, Tmax %d", U, Tmax);
    build_table(*s);
    check_range(s->fbinMin, s->fbinMax, s->M, s->tblFbinMax);
    require_device();
    if (U == 0 || Tmax == 0) return;
    hipStream_t st = (hipStream_t) stream;
    double* rp = rp_dev;
    if (!rp) { DevBuf<double>& w = s->ws.at(st); w.reserve((size_t) U * Tmax * s->nTheta); rp = w.p; }
    doa_launch_rp(*s, X_dev, nframes_dev, U, Tmax, rp, energy_dev, Y_dev, st);
    doa_launch_frame(rp, energy_dev, nframes_dev, U, Tmax, s->nTheta, s->nBest, s->threshold, nbest_rp_dev, nbest_idx_dev, gated_dev, st);
    doa_launch_acc(rp, energy_dev, nframes_dev, U, Tmax, s->nTheta, s->threshold, acc_dev, st);
  });
}

dsr_status dsr_doa_final_nbest(dsr_doa* s, const double* acc, int U, double* nbest_rp, int32_t* nbest_idx)
{
  return guard([&] {
    if (!s || !acc || !nbest_rp || !nbest_idx) throw Error(DSR_E_PARAMETER, "null argument");
    if (!s->tbl) throw Error(DSR_E_ERROR, "no steering table: run the estimator after construction / setSearchParam first");
    final_nbest(acc, U, s->nTheta, s->nBest, nbest_rp, nbest_idx);      // _getNBestHypothesesFromACCRP (:2986-3025)
  });
}

}  // extern "C"
