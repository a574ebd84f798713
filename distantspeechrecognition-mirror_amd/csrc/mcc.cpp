// csrc/mcc.cpp -- host side of multichannel cross-correlation source localisation, include/dsr.h section 2f (kernels: csrc/k_mcc.hip; what the two
// share: csrc/mcc.h).  Restates SearchGridBuilder / SGB4LinearArray / SGB4CircularArray of btk/localization (MCCLocalizer.h:55-301,
// MCCLocalizer.cc:10-576; the delay functions localization.cc:110-142): the grid code is host-only and keeps the reference's float arithmetic.
// Then the localiser's and the calculator's checks and the dsr_sgb_* / dsr_mcc_* entries.
#include "mcc.h"
#include <cmath>

using namespace dsr;

namespace {

constexpr double SSPEED = 343740.0, TPI = 6.28318530717958647692;
constexpr int MAX_GRID = 65536;

// ---- the search grids (host, float arithmetic as in the reference) ------------------------------------------------------------------------
void sgb_need_geometry(const dsr_sgb& g)
{
  if (!(g.maxTimeDelay >= 0.0f)) throw Error(DSR_E_INITIALIZATION, "set the geometry of the array before the search grid is used");
}
// nextSearchGridFF of the two builders; false = the walk is over
bool sgb_step(const dsr_sgb& g, double* hypo)
{
  if (!g.farField) { fprintf(stderr, "need to be implemented\n"); return false; }                       // nextSearchGridNF hands out NULL
  if (g.kind == DSR_SGB_LINEAR) {                                                                        // MCCLocalizer.cc:114-143
    const float azimuth = (float) hypo[1], oldSin = sinf(azimuth); float newAzimuth, newSin;
    if (azimuth < M_PI_2) {
      newSin = oldSin + g.constV;
      newAzimuth = newSin >= 1 ? (float) M_PI_2 : asinf(newSin);
    } else if (azimuth < (3 * M_PI_2)) {
      newAzimuth = (float) (3 * M_PI_2);
    } else {
      newSin = oldSin + g.constV;
      if ((newSin + g.constV / 2.0) >= 0) return false;
      newAzimuth = (float) (TPI + asinf(newSin));
    }
    hypo[1] = newAzimuth;
    return true;
  }
  // MCCLocalizer.cc:202-237 with the two stated deviations: |sin|, |cos| in the polar step, and the walk ends when the azimuth reaches 2 pi
  const float azimuth = (float) hypo[1], polarAngle = (float) hypo[2]; float newAzimuth, newPolarAngle, val1, val2;
  if (azimuth >= TPI) return false;
  if ((azimuth >= M_PI_4 && azimuth < (3 * M_PI_4)) || (azimuth >= (5 * M_PI_4) && azimuth < (7 * M_PI_4))) val1 = g.constV / fabsf(sinf(azimuth));
  else val1 = g.constV / fabsf(cosf(azimuth));
  newPolarAngle = (val1 < 1) ? asinf(val1) : (float) M_PI_2;
  if ((newPolarAngle + polarAngle) < M_PI) {
    newPolarAngle += polarAngle; newAzimuth = azimuth;
  } else {
    val2 = g.constV / sinf(newPolarAngle);
    newAzimuth = (val2 < 1) ? (float) acos((double) (g.constV / val2)) : (float) M_PI;
    newAzimuth += azimuth;
  }
  if (newAzimuth >= TPI) return false;
  hypo[1] = newAzimuth; hypo[2] = newPolarAngle;
  return true;
}
void sgb_delays(const dsr_sgb& g, const double* hypo, double* delays)
{
  const int C = g.C;
  if (g.kind == DSR_SGB_LINEAR) {                                                                        // localization.cc:110-121
    const float azimuth = (float) hypo[1];
    delays[0] = 0.0;
    for (int i = 1; i < C; i++) {
      const float dist = (float) fabs(g.mpos[3 * i + 1] - g.mpos[1]);
      delays[i] = -dist * sin((double) azimuth) / SSPEED;
    }
    return;
  }
  const float azimuth = (float) hypo[1], polarAngle = (float) hypo[2], sspeed = (float) SSPEED;            // localization.cc:130-142
  for (int i = 0; i < C; i++) {
    const float cx = -sinf(polarAngle) * cosf(azimuth), cy = -sinf(polarAngle) * sinf(azimuth), cz = -cosf(polarAngle);
    const float delay = (float) ((cx * g.mpos[3 * i] + cy * g.mpos[3 * i + 1] + cz * g.mpos[3 * i + 2]) / sspeed);
    delays[i] = (double) delay;
  }
}
inline int tau_of(unsigned fs, double delay) { const float tau_l = (float) (fs * delay); return (int) tau_l; }   // MCCLocalizer.cc:330-331
inline int sgb_max_sample_delay(const dsr_sgb& g) { return (int) (size_t) (g.fs * g.maxTimeDelay); }            // :268
// the whole walk from (0, 0, 0); any of the outputs may be null
int sgb_enumerate(const dsr_sgb& g, int maxG, double* positions, double* delays, int32_t* tau)
{
  sgb_need_geometry(g);
  if (!g.farField) { fprintf(stderr, "need to be implemented\n"); throw Error(DSR_E_INITIALIZATION, "need to be implemented"); }
  double hypo[3] = {0.0, 0.0, 0.0}; std::vector<double> d(g.C); int G = 0;
  do {
    if (G >= MAX_GRID) throw Error(DSR_E_DIMENSION, "the search grid has more than %d points", MAX_GRID);
    if (G < maxG) {
      sgb_delays(g, hypo, d.data());
      if (positions) for (int k = 0; k < 3; k++) positions[(size_t) G * 3 + k] = hypo[k];
      if (delays) for (int c = 0; c < g.C; c++) delays[(size_t) G * g.C + c] = d[c];
      if (tau) for (int c = 0; c < g.C; c++) tau[(size_t) G * g.C + c] = tau_of(g.fs, d[c]);
    }
    G++;
  } while (sgb_step(g, hypo));
  return G;
}

void mcc_check_block(int D, int L, int N)
{
  if (L < 1 || N < L) throw Error(DSR_E_DIMENSION, "block length %d, %d samples a channel", L, N);
  if (L < 2 * D) { fprintf(stderr, "Data samples are insufficient. It must be more than %d\n", 2 * D); throw Error(DSR_E_ERROR, "Data samples are insufficient"); }
}

void mcc_validate(const dsr_sgb* g, int maxSource, int* Gout, int* Dout, std::vector<int>* tau, std::vector<double>* pos)
{
  if (!g) throw Error(DSR_E_PARAMETER, "null argument");
  if (maxSource < 1 || maxSource > 64) throw Error(DSR_E_DIMENSION, "maxSource %d outside [1, 64]", maxSource);
  if (g->C < 2 || g->C > 64) throw Error(DSR_E_DIMENSION, "%d channels: 2 to 64 are supported", g->C);
  sgb_need_geometry(*g);                                                                                 // the reference casts maxTimeDelay = -1 to size_t
  const int G = sgb_enumerate(*g, 0, nullptr, nullptr, nullptr), D = sgb_max_sample_delay(*g);
  std::vector<int> t((size_t) G * g->C); std::vector<double> ps((size_t) G * 3);
  sgb_enumerate(*g, G, ps.data(), nullptr, t.data());
  for (size_t i = 0; i < t.size(); i++)
    if (t[i] > D || t[i] < -D) throw Error(DSR_E_DIMENSION, "grid point %zu shifts channel %zu by %d samples, more than the maximum sample delay %d", i / g->C, i % g->C, t[i], D);
  if (Gout) *Gout = G; if (Dout) *Dout = D;
  if (tau) tau->swap(t); if (pos) pos->swap(ps);
}

}  // namespace

extern "C" {

dsr_status dsr_sgb_create(int kind, int nChan, int isFarField, unsigned samplingFreq, dsr_sgb** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind != DSR_SGB_LINEAR && kind != DSR_SGB_CIRCULAR) throw Error(DSR_E_PARAMETER, "unknown search grid kind %d", kind);
    if (nChan < 1 || samplingFreq < 1) throw Error(DSR_E_DIMENSION, "%d channels at %u Hz", nChan, samplingFreq);
    dsr_sgb* g = new dsr_sgb(); g->kind = kind; g->C = nChan; g->farField = isFarField != 0; g->fs = samplingFreq;
    g->mpos.assign((size_t) nChan * 3, 0.0); g->delays.assign(nChan, 0.0);
    *out = g;
  });
}
void dsr_sgb_destroy(dsr_sgb* g) { delete g; }

dsr_status dsr_sgb_set_distance(dsr_sgb* g, float distance)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null argument");
    if (g->kind != DSR_SGB_LINEAR) throw Error(DSR_E_PARAMETER, "setDistanceBtwMicrophones belongs to the linear array");
    const size_t nMic = (size_t) g->C;
    for (size_t micX = 0; micX < nMic; micX++) { g->mpos[3 * micX] = 0.0; g->mpos[3 * micX + 1] = micX * distance; g->mpos[3 * micX + 2] = 0.0; }
    g->constV = (float) (0.99 * SSPEED / ((nMic - 1) * distance * g->fs));
    g->maxTimeDelay = (float) ((nMic - 1) * distance / SSPEED);
  });
}
dsr_status dsr_sgb_set_positions(dsr_sgb* g, const double* mpos, int rows)
{
  return guard([&] {
    if (!g || !mpos) throw Error(DSR_E_PARAMETER, "null argument");
    if (g->kind != DSR_SGB_LINEAR) throw Error(DSR_E_PARAMETER, "setPositionsOfMicrophones belongs to the linear array");
    if (rows != g->C) throw Error(DSR_E_DIMENSION, "The size of the matrix for the geometry of the array should be %d x %d", g->C, 3);
    float maxDist = -1; const float pos0[3] = {(float) mpos[0], (float) mpos[1], (float) mpos[2]};
    for (int micX = 0; micX < rows; micX++) {                                                            // every row, distances from microphone 0
      for (int k = 0; k < 3; k++) g->mpos[3 * micX + k] = mpos[3 * micX + k];
      if (micX > 0) {
        const float dx = pos0[0] - (float) mpos[3 * micX], dy = pos0[1] - (float) mpos[3 * micX + 1], dz = pos0[2] - (float) mpos[3 * micX + 2];
        const float dist = sqrtf(dx * dx + dy * dy + dz * dz);
        if (dist > maxDist) maxDist = dist;
      }
    }
    g->constV = (float) (0.99 * SSPEED / (maxDist * g->fs));
    g->maxTimeDelay = (float) (maxDist / SSPEED);
  });
}
dsr_status dsr_sgb_set_radius(dsr_sgb* g, float radius, float height)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null argument");
    if (g->kind != DSR_SGB_CIRCULAR) throw Error(DSR_E_PARAMETER, "setRadius belongs to the circular array");
    const size_t nMic = (size_t) g->C; const float bias = (float) (TPI / (float) nMic);
    for (size_t micX = 0; micX < nMic; micX++) {
      g->mpos[3 * micX] = radius * cosf(micX * bias); g->mpos[3 * micX + 1] = radius * sinf(micX * bias); g->mpos[3 * micX + 2] = height;
    }
    g->constV = (float) (SSPEED / (2 * radius * g->fs));
    g->maxTimeDelay = (float) (2 * radius / SSPEED);
  });
}
dsr_status dsr_sgb_reset(dsr_sgb* g) { return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->hypo[0] = g->hypo[1] = g->hypo[2] = 0.0; }); }
dsr_status dsr_sgb_next(dsr_sgb* g, int32_t* more)
{
  return guard([&] {
    if (!g || !more) throw Error(DSR_E_PARAMETER, "null argument");
    sgb_need_geometry(*g);
    *more = sgb_step(*g, g->hypo) ? 1 : 0;
  });
}
dsr_status dsr_sgb_position(const dsr_sgb* g, double* pos3)
{ return guard([&] { if (!g || !pos3) throw Error(DSR_E_PARAMETER, "null argument"); for (int k = 0; k < 3; k++) pos3[k] = g->hypo[k]; }); }
dsr_status dsr_sgb_time_delays(dsr_sgb* g, double* delays)
{
  return guard([&] {
    if (!g || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    sgb_need_geometry(*g);
    sgb_delays(*g, g->hypo, g->delays.data());
    for (int c = 0; c < g->C; c++) delays[c] = g->delays[c];
  });
}
double dsr_sgb_max_time_delay(const dsr_sgb* g) { return g ? (double) g->maxTimeDelay : -1.0; }
int dsr_sgb_chan_n(const dsr_sgb* g) { return g ? g->C : 0; }
int dsr_sgb_sampling_frequency(const dsr_sgb* g) { return g ? (int) g->fs : 0; }
dsr_status dsr_sgb_microphone_positions(const dsr_sgb* g, double* mpos)
{ return guard([&] { if (!g || !mpos) throw Error(DSR_E_PARAMETER, "null argument"); for (size_t i = 0; i < g->mpos.size(); i++) mpos[i] = g->mpos[i]; }); }
dsr_status dsr_sgb_enumerate(const dsr_sgb* g, int maxG, int32_t* G, double* positions, double* delays, int32_t* tau)
{
  return guard([&] {
    if (!g || !G) throw Error(DSR_E_PARAMETER, "null argument");
    *G = sgb_enumerate(*g, maxG < 0 ? 0 : maxG, positions, delays, tau);
  });
}

dsr_status dsr_mcc_check(const dsr_sgb* g, int maxSource, int blockLen)
{
  return guard([&] {
    int G = 0, D = 0; mcc_validate(g, maxSource, &G, &D, nullptr, nullptr);
    if (blockLen > 0) mcc_check_block(D, blockLen, blockLen);
  });
}
dsr_status dsr_mcc_create(const dsr_sgb* g, int maxSource, dsr_mcc** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    std::unique_ptr<dsr_mcc> m(new dsr_mcc());
    mcc_validate(g, maxSource, &m->G, &m->D, &m->tau, &m->pos);
    m->C = g->C; m->fs = g->fs; m->S = maxSource;
    require_device();
    *out = m.release();
  });
}
void dsr_mcc_destroy(dsr_mcc* m) { delete m; }
dsr_status dsr_mcc_check_block(const dsr_mcc* m, int blockLen)
{ return guard([&] { if (!m) throw Error(DSR_E_PARAMETER, "null argument"); mcc_check_block(m->D, blockLen, blockLen); }); }
int dsr_mcc_grid_n(const dsr_mcc* m) { return m ? m->G : 0; }
int dsr_mcc_chan_n(const dsr_mcc* m) { return m ? m->C : 0; }
int dsr_mcc_max_source(const dsr_mcc* m) { return m ? m->S : 0; }
int dsr_mcc_max_sample_delay(const dsr_mcc* m) { return m ? m->D : 0; }
dsr_status dsr_mcc_set_timing(dsr_mcc* m, int on)
{
  return guard([&] {
    if (!m) throw Error(DSR_E_PARAMETER, "null argument");
    m->tm.enable(on != 0);
  });
}
dsr_status dsr_mcc_kernel_ms(const dsr_mcc* m, double* ms3)
{
  return guard([&] {
    if (!m || !ms3 || !m->tm.on) throw Error(DSR_E_PARAMETER, "timing is off");
    m->tm.wait(3);
    for (int k = 0; k < 3; k++) ms3[k] = m->tm.ms(k, k + 1);
  });
}

dsr_status dsr_mcc_run(dsr_mcc* m, const float* x_dev, const int32_t* nsamples_dev, int U, int N, int blockLen, int32_t* valid_dev, int32_t* index_dev, double* cost_dev,
                       int32_t* tau_dev, double* position_dev, double* eig_dev, double* costmap_dev, double* R_dev, void* stream)
{
  return guard([&] {
    if (!m || !x_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 1) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d", U);
    mcc_check_block(m->D, blockLen, N);
    require_device();
    hipStream_t st = (hipStream_t) stream;
    if (!m->uploaded) { m->d_tau.upload(m->tau); m->d_pos.upload(m->pos); m->uploaded = true; }
    mcc_launch(m, x_dev, nsamples_dev, U, N, blockLen, m->G, m->d_tau.p, m->d_pos.p, m->S, 1,
               MOut{valid_dev, index_dev, cost_dev, tau_dev, position_dev, eig_dev, costmap_dev, R_dev}, st);
  });
}

dsr_status dsr_mcc_calc(dsr_mcc* m, const float* x_dev, const int32_t* nsamples_dev, int U, int N, int blockLen, const double* delays, int normalizeVariance,
                        int32_t* valid_dev, double* cost_dev, int32_t* tau_host, double* eig_dev, double* R_dev, void* stream)
{
  return guard([&] {
    if (!m || !x_dev || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 1) throw Error(DSR_E_PARAMETER, "bad batch shape U=%d", U);
    mcc_check_block(m->D, blockLen, N);
    std::vector<int> t(m->C);
    for (int c = 0; c < m->C; c++) {
      t[c] = tau_of(m->fs, delays[c]);
      if (t[c] > m->D || t[c] < -m->D) throw Error(DSR_E_INDEX, "channel %d is shifted by %d samples, more than the maximum sample delay %d", c, t[c], m->D);
      if (tau_host) tau_host[c] = t[c];
    }
    require_device();
    hipStream_t st = (hipStream_t) stream;
    const std::vector<double> zero(3, 0.0);
    m->d_tau1.upload(t, st); m->d_pos1.upload(zero, st);
    mcc_launch(m, x_dev, nsamples_dev, U, N, blockLen, 1, m->d_tau1.p, m->d_pos1.p, 1, normalizeVariance != 0,
               MOut{valid_dev, nullptr, cost_dev, nullptr, nullptr, eig_dev, nullptr, R_dev}, st);
    DSR_HIP(hipStreamSynchronize(st));                                                                  // the one-row table may be rewritten by the next call
  });
}

dsr_status dsr_mcc_channel_delays(const dsr_mcc* m, const int32_t* tau, double* delays)
{
  return guard([&] {
    if (!m || !tau || !delays) throw Error(DSR_E_PARAMETER, "null argument");
    for (int c = 0; c < m->C; c++) delays[c] = (double) tau[c] / (double) m->fs;
  });
}

}  // extern "C"
