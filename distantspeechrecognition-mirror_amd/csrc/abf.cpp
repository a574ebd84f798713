// csrc/abf.cpp -- the host side of the adaptive subband beamformers of btk/lib/subbandBeamforming.py (dsr_abf_*): the set-up helpers restated in
// the reference's order of operations, the handle's configuration and the C entries.  Kernels and launch: csrc/abf_kernels.hip, through csrc/abf.h.
//   calcBlockingMatrix        btk/lib/subbandBeamforming.py:249-277     getInverseMat22 :495-514     calcNullBeamformer :517-546
//   calcArrayManifold_f / calcArrayManifoldWoNorm_f :438-493
#include "abf.h"
#include <cmath>

namespace dsr {

// :249-277 -- the projector I - conj(vs) vs^T / (vs . conj vs), Gram-Schmidt over its first C - NC columns in that order.  B [C][C - NC].
static void abf_blocking_matrix(const zc* vs, int C, int NC, zc* B)
{
  const int bs = C - NC;
  for (int i = 0; i < C * bs; i++) B[i] = zc(0, 0);
  zc norm(0, 0); for (int i = 0; i < C; i++) norm += vs[i] * std::conj(vs[i]);
  if (!(norm.real() > 0.0)) return;
  std::vector<zc> vec(C);
  for (int d = 0; d < bs; d++) {
    for (int i = 0; i < C; i++) vec[i] = (i == d ? zc(1, 0) : zc(0, 0)) - std::conj(vs[i]) * vs[d] / norm;
    for (int j = 0; j < d; j++) {
      zc ip(0, 0); for (int i = 0; i < C; i++) ip += std::conj(B[i * bs + j]) * vec[i];
      for (int i = 0; i < C; i++) vec[i] -= B[i * bs + j] * ip;
    }
    zc nn(0, 0); for (int i = 0; i < C; i++) nn += std::conj(vec[i]) * vec[i];
    const double nv = std::sqrt(std::abs(nn));
    for (int i = 0; i < C; i++) B[i * bs + d] = vec[i] / nv;
  }
}

// :517-546 with getInverseMat22 (:495-514): wq = C (C^H C)^-1 g, C = [w_t w_j], g = (1, 0)
static void abf_null_beamformer(const zc* wt, const zc* wj, int C, zc* wq)
{
  zc m00(0, 0), m01(0, 0), m10(0, 0), m11(0, 0);
  for (int i = 0; i < C; i++) { m00 += std::conj(wt[i]) * wt[i]; m01 += std::conj(wt[i]) * wj[i]; m10 += std::conj(wj[i]) * wt[i]; m11 += std::conj(wj[i]) * wj[i]; }
  zc det = m00 * m11 - m01 * m10;
  if (std::abs(det) < 1.0e-07) { m00 += 0.01; m11 += 0.01; det = m00 * m11 - m01 * m10; }       // "compensate for non-invertibility"
  const zc v0 = m11 / det, v1 = -m10 / det;                                                    // the inverse's first column: g = (1, 0)
  for (int i = 0; i < C; i++) wq[i] = wt[i] * v0 + wj[i] * v1;
}

static void abf_need(const AbfState& s, bool B)
{
  if (!s.haveWq) throw Error(DSR_E_ERROR, "call calcArrayManifoldVectors() once");
  if (B && !s.haveB) throw Error(DSR_E_ERROR, "call calcArrayManifoldVectors() once: no blocking matrix");
}

static void abf_upload(AbfState& s)
{
  const int C = s.C, F = s.M / 2 + 1, nb = C - s.NC;
  if (!s.dirty) return;
  auto up = [](const std::vector<zc>& v, DevBuf<double2>& d) {
    std::vector<double2> a(v.size()); for (size_t i = 0; i < v.size(); i++) a[i] = make_double2(v[i].real(), v[i].imag());
    d.upload(a);
  };
  if (s.kind == DSR_ABF_DS || s.kind == DSR_ABF_GSC) {
    std::vector<zc> w(s.wq);
    if (s.kind == DSR_ABF_GSC)
      for (int f = 0; f < F; f++) for (int i = 0; i < C; i++) {
        zc wl(0, 0); for (int j = 0; j < nb; j++) wl += s.B[((size_t) f * C + i) * nb + j] * s.wa[(size_t) f * nb + j];
        w[(size_t) f * C + i] -= wl;
      }
    up(w, s.d_weff);
  } else {
    // the blocking matrices bin-fastest for the recursion kernels, whose neighbouring lanes are neighbouring bins: B [C][C-1][F]
    std::vector<zc> bt((size_t) F * C * nb);
    for (int f = 0; f < F; f++) for (int c = 0; c < C; c++)
      for (int j = 0; j < nb; j++) bt[((size_t) c * nb + j) * F + f] = s.B[((size_t) f * C + c) * nb + j];
    up(s.wq, s.d_wq); up(bt, s.d_B);
  }
  s.dirty = false;
}

}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_abf_create(int kind, int fftLen, int chanN, int NC, int halfBandShift, dsr_abf** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < DSR_ABF_DS || kind > DSR_ABF_MPDR) throw Error(DSR_E_PARAMETER, "bad kind %d", kind);
    if (halfBandShift) throw Error(DSR_E_CONSISTENCY, "halfBandShift==True is not supported");
    if (NC != 1 && !(kind == DSR_ABF_GSC && NC == 2)) throw Error(DSR_E_CONSISTENCY, "NC = %d: one constraint (two for the static GSC only)", NC);
    if (fftLen < 2 || (fftLen & 1)) throw Error(DSR_E_DIMENSION, "bad fftLen=%d", fftLen);
    if (chanN < 1 + NC || chanN > DSR_ABF_MAX_CHAN) throw Error(DSR_E_DIMENSION, "%d to %d channels (%d)", 1 + NC, DSR_ABF_MAX_CHAN, chanN);
    dsr_abf* s = new dsr_abf(); s->kind = kind; s->M = fftLen; s->C = chanN; s->NC = NC;
    s->wa.assign((size_t) (fftLen / 2 + 1) * (chanN - NC), zc(0, 0));
    *out = s;
  });
}
void dsr_abf_destroy(dsr_abf* s) { delete s; }

dsr_status dsr_abf_config(dsr_abf* s, double beta, double gamma, double initDiagLoad, double floorSubBandSigmaK, double silThresh, double alpha2,
                          int staticAfter, double diagLoad, double forgetFactor, int end)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    if ((s->kind == DSR_ABF_MVDR || s->kind == DSR_ABF_MPDR) && !(diagLoad > 0.0))
      throw Error(DSR_E_PARAMETER, "diagLoad must be positive (%g): the loaded matrix is factorised, not inverted", diagLoad);
    if (s->kind == DSR_ABF_GJ && !(silThresh > 0.0 && floorSubBandSigmaK > 0.0)) throw Error(DSR_E_PARAMETER, "silThresh and floorSubBandSigmaK must be positive");
    AbfParams& p = s->p;
    p.beta = beta; p.gamma = gamma; p.initDiagLoad = initDiagLoad; p.floorSb = floorSubBandSigmaK; p.silThresh = silThresh; p.alpha2 = alpha2;
    p.staticAfter = staticAfter; p.diagLoad = diagLoad; p.lambda = forgetFactor; p.end = end;
  });
}

dsr_status dsr_abf_set_fixed_weights(dsr_abf* s, const double* wq, const double* B)
{
  return guard([&] {
    if (!s || !wq) throw Error(DSR_E_PARAMETER, "null argument");
    const int C = s->C, F = s->M / 2 + 1, nb = C - s->NC;
    const zc* q = reinterpret_cast<const zc*>(wq);
    s->wq.assign(q, q + (size_t) F * C); s->haveWq = true;
    s->B.assign((size_t) F * C * nb, zc(0, 0));
    if (B) { const zc* b = reinterpret_cast<const zc*>(B); s->B.assign(b, b + (size_t) F * C * nb); }
    else for (int f = 0; f < F; f++) abf_blocking_matrix(&s->wq[(size_t) f * C], C, s->NC, &s->B[(size_t) f * C * nb]);
    s->haveB = true; s->dirty = true;
  });
}
dsr_status dsr_abf_get_fixed_weights(const dsr_abf* s, double* wq, double* B)
{
  return guard([&] {
    if (!s) throw Error(DSR_E_PARAMETER, "null argument");
    abf_need(*s, B != nullptr);
    if (wq) memcpy(wq, s->wq.data(), s->wq.size() * sizeof(zc));
    if (B) memcpy(B, s->B.data(), s->B.size() * sizeof(zc));
  });
}
dsr_status dsr_abf_set_active_weights(dsr_abf* s, const double* wa)
{
  return guard([&] {
    if (!s || !wa) throw Error(DSR_E_PARAMETER, "null argument");
    if (s->kind != DSR_ABF_GSC) throw Error(DSR_E_CONSISTENCY, "setWa: the static GSC only (the adaptive kinds find their own active weights)");
    const zc* w = reinterpret_cast<const zc*>(wa); s->wa.assign(w, w + s->wa.size()); s->dirty = true;
  });
}

dsr_status dsr_abf_blocking_matrix(const double* vs, int chanN, int NC, double* B)
{
  return guard([&] {
    if (!vs || !B) throw Error(DSR_E_PARAMETER, "null argument");
    if (NC < 1 || chanN <= NC) throw Error(DSR_E_DIMENSION, "calcBlockingMatrix: %d channels, %d constraints", chanN, NC);
    abf_blocking_matrix(reinterpret_cast<const zc*>(vs), chanN, NC, reinterpret_cast<zc*>(B));
  });
}
dsr_status dsr_abf_null_beamformer(const double* wt, const double* wj, int chanN, int NC, double* wq)
{
  return guard([&] {
    if (!wt || !wj || !wq) throw Error(DSR_E_PARAMETER, "null argument");
    if (NC != 2) throw Error(DSR_E_CONSISTENCY, "The number of constraints must be 2: %d", NC);                  // :524-526
    if (chanN < 2) throw Error(DSR_E_DIMENSION, "calcNullBeamformer: %d channels", chanN);
    abf_null_beamformer(reinterpret_cast<const zc*>(wt), reinterpret_cast<const zc*>(wj), chanN, reinterpret_cast<zc*>(wq));
  });
}
dsr_status dsr_abf_manifold(int fbinX, int fftLen, int chanN, double sampleRate, const double* delays, int halfBandShift, int normalize, double* vs)
{
  return guard([&] {
    if (!delays || !vs) throw Error(DSR_E_PARAMETER, "null argument");
    if (halfBandShift) throw Error(DSR_E_CONSISTENCY, "halfBandShift==True is not supported");
    if (fftLen < 2 || (fftLen & 1) || chanN < 1) throw Error(DSR_E_DIMENSION, "bad fftLen=%d chanN=%d", fftLen, chanN);
    if (fbinX < 0 || fbinX >= fftLen) throw Error(DSR_E_INDEX, "frequency bin %d out of range", fbinX);
    const double df = sampleRate / (double) fftLen; zc* v = reinterpret_cast<zc*>(vs);
    for (int c = 0; c < chanN; c++) {
      const double ph = fbinX <= fftLen / 2 ? -(2.0 * M_PI * fbinX * df * delays[c]) : 2.0 * M_PI * (fftLen - fbinX) * df * delays[c];
      v[c] = zc(std::cos(ph), std::sin(ph)); if (normalize) v[c] /= (double) chanN;
    }
  });
}

dsr_status dsr_abf_run(dsr_abf* s, const float* X_dev, const int32_t* nframes_dev, int U, int Tmax, const float* wp_dev, const int32_t* wpFrames_dev,
                       float* Y_dev, double* wOut_dev, void* stream)
{
  return guard([&] {
    if (!s || !X_dev || !Y_dev) throw Error(DSR_E_PARAMETER, "null argument");
    if (U < 0 || Tmax < 0) throw Error(DSR_E_DIMENSION, "bad batch U=%d Tmax=%d", U, Tmax);
    const bool adaptive = s->kind >= DSR_ABF_GJ;
    abf_need(*s, s->kind == DSR_ABF_GSC || s->kind == DSR_ABF_GJ || s->kind == DSR_ABF_MPDR);
    if (s->kind == DSR_ABF_GJ && !s->spkr) throw Error(DSR_E_ERROR, "SubbandBeamformerGriffithsJim: call nextSpkr() before the first frame");
    if (wOut_dev && !adaptive) throw Error(DSR_E_PARAMETER, "final weights: the adaptive kinds only");
    if (adaptive && s->carry && s->haveState && s->stateU != U)
      throw Error(DSR_E_CONSISTENCY, "AdaptiveBeamformer: the carried state holds %d streams, this call has %d (reset the state first)", s->stateU, U);
    require_device();
    if (U == 0 || Tmax == 0) return;
    abf_upload(*s);
    abf_launch(*s, X_dev, nframes_dev, U, Tmax, wp_dev, wpFrames_dev, Y_dev, wOut_dev, (hipStream_t) stream);
  });
}

dsr_status dsr_abf_set_carry(dsr_abf* s, int on)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->carry = on != 0; if (!on) s->haveState = false; }); }
dsr_status dsr_abf_reset(dsr_abf* s)
{ return guard([&] { if (!s) throw Error(DSR_E_PARAMETER, "null argument"); s->haveState = false; s->spkr = true; }); }

dsr_status dsr_abf_path(int kind, int chanN, int path[3], int64_t lds[2])
{
  return guard([&] {
    if (!path) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind < DSR_ABF_GJ || kind > DSR_ABF_MPDR) throw Error(DSR_E_PARAMETER, "bad kind %d: the adaptive kinds have a dispatch", kind);
    if (chanN < 2 || chanN > DSR_ABF_MAX_CHAN) throw Error(DSR_E_DIMENSION, "AdaptiveBeamformer: 2 to %d channels (%d)", DSR_ABF_MAX_CHAN, chanN);
    const AbfPath r = abf_path(kind, chanN);
    path[0] = r.ct; path[1] = r.cap; path[2] = r.residence;
    if (lds) { lds[0] = (int64_t) r.stateBytes; lds[1] = (int64_t) r.ldsBytes; }
  });
}

}  // extern "C"
