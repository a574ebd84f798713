// csrc/gsc_weights.h -- the host-side generalized-sidelobe-canceller weight pieces of beamformerWeights that more than one file needs
// (beamformer.cpp, mmi.cpp, sph.cpp): the blocking matrix of a quiescent vector (_calcBlockingMatrix, beamformer.cc:398-479, any NC) and
// the sidelobe canceller's wl = B wa (calcSidelobeCancellerP_f / U_f, :761-799).  GSL's complex product, so that values agree with the
// reference to rounding.
#pragma once
#include <complex>
#include <cmath>
#include <vector>

namespace dsr {

namespace gsc {
typedef std::complex<double> zc;
inline zc mul(zc a, zc b) { return zc(a.real() * b.real() - a.imag() * b.imag(), a.real() * b.imag() + a.imag() * b.real()); }
inline double abs2(zc a) { return a.real() * a.real() + a.imag() * a.imag(); }
}  // namespace gsc

// _calcBlockingMatrix (beamformer.cc:398-479): d [C] the quiescent vector -> B [C][C - NC], orthonormal columns with B^H d = 0
inline bool blocking_matrix_nc(const std::complex<double>* d, int C, int NC, std::complex<double>* B)
{
  using namespace gsc;
  const int bs = C - NC;
  if (bs <= 0) return false;
  std::vector<zc> P((size_t) C * C), vec(C);
  double nrm = 0; for (int i = 0; i < C; i++) nrm += abs2(d[i]);
  nrm = std::sqrt(nrm); nrm = nrm * nrm;
  for (int i = 0; i < C; i++) for (int j = 0; j < C; j++) P[(size_t) i * C + j] = zc(i == j ? 1.0 : 0.0, 0.0) + mul(mul(zc(-1.0 / nrm, 0.0), std::conj(d[i])), d[j]);
  for (int k = 0; k < C * bs; k++) B[k] = zc(0, 0);
  for (int id = 0; id < bs; id++) {
    for (int i = 0; i < C; i++) vec[i] = P[(size_t) i * C + id];
    for (int jd = 0; jd < id; jd++) {
      zc ip(0, 0); for (int i = 0; i < C; i++) ip += mul(std::conj(B[(size_t) i * bs + jd]), vec[i]);
      ip = zc(ip.real() * -1.0, ip.imag() * -1.0);
      for (int i = 0; i < C; i++) vec[i] += mul(ip, B[(size_t) i * bs + jd]);
    }
    double nv = 0; for (int i = 0; i < C; i++) nv += abs2(vec[i]);
    nv = std::sqrt(nv);
    for (int i = 0; i < C; i++) B[(size_t) i * bs + id] = zc(vec[i].real() * (1.0 / nv), vec[i].imag() * (1.0 / nv));
  }
  return true;
}

// calcSidelobeCancellerP_f / U_f (:761-799): wl [C] = B [C][bs] wa [bs]
inline void sidelobe_wl(const std::complex<double>* B, const std::complex<double>* wa, int C, int bs, std::complex<double>* wl)
{
  for (int i = 0; i < C; i++) {
    gsc::zc acc(0, 0);
    for (int j = 0; j < bs; j++) acc += gsc::mul(B[(size_t) i * bs + j], wa[j]);
    wl[i] = acc;
  }
}

}  // namespace dsr
