// csrc/train.cpp -- the host side of GMM training: parameter updates, Gaussian splitting and the accumulator files.
//
// Replaces CodebookTrain::Accu::update / updateMMI / save / load / add, CodebookTrain::split / fixGConsts / invertVariance / floorVariances and
// CodebookSetTrain::saveAccus / loadAccus (asr/train/codebookTrain.cc, "cT"), DistribTrain::Accu::update / updateMMI / save / load / add,
// DistribTrain::split, AccMap and DistribSetTrain::saveAccus / loadAccus (asr/train/distribTrain.cc, "dT").  Everything here is arithmetic over
// a few thousand numbers in the reference's order and precision (float where the reference rounds to float); the accumulator rows are pulled
// from the device, worked on and pushed back (csrc/train.h).  Compiled with -ffp-contract=off.
#include "common.h"
#include "train.h"
#include "befile.h"
#include <cmath>
#include <map>

using namespace dsr;

namespace {

struct Rows {                                              // the columns of an accumulator row (csrc/train.h)
  int D;
  double* sumO(double* r) const { return r; }
  double* sumOsq(double* r) const { return r + D; }
  double& count(double* r) const { return r[2 * D]; }
  double& den(double* r) const { return r[2 * D + 1]; }
  double& dcount(double* r) const { return r[2 * D + 2]; }
  double& dden(double* r) const { return r[2 * D + 3]; }
};

void reupload(GmmModel& m) { gmm_finish(m); }              // device copies of the parameters; mode 2 rebuilds its operand image

}  // namespace

extern "C" {

dsr_status dsr_train_zero(dsr_train* t, int what, int nParts, int part)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    int k0, k1; part_range(t->g->K, nParts, part, k0, k1);
    t->pull(); const Rows c{t->D};
    for (int g = t->g->off[k0]; g < t->g->off[k1]; g++) {
      double* r = t->row(g);
      if (what & 1) { for (int d = 0; d < 2 * t->D; d++) r[d] = 0.0; c.count(r) = c.den(r) = 0.0; }
      if (what & 2) c.dcount(r) = c.dden(r) = 0.0;
    }
    t->push();
  });
}

dsr_status dsr_train_get(dsr_train* t, double* count, double* denCount, double* sumO, double* sumOsq, double* distCount, double* distDenCount)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    t->pull(); const Rows c{t->D}; const int D = t->D;
    for (int g = 0; g < t->G; g++) {
      double* r = t->row(g);
      if (count) count[g] = c.count(r); if (denCount) denCount[g] = c.den(r);
      if (distCount) distCount[g] = c.dcount(r); if (distDenCount) distDenCount[g] = c.dden(r);
      if (sumO) memcpy(sumO + (size_t) g * D, c.sumO(r), D * sizeof(double));
      if (sumOsq) memcpy(sumOsq + (size_t) g * D, c.sumOsq(r), D * sizeof(double));
    }
  });
}

dsr_status dsr_train_set(dsr_train* t, const double* count, const double* denCount, const double* sumO, const double* sumOsq, const double* distCount,
                         const double* distDenCount)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    t->pull(); const Rows c{t->D}; const int D = t->D;
    for (int g = 0; g < t->G; g++) {
      double* r = t->row(g);
      if (count) c.count(r) = count[g]; if (denCount) c.den(r) = denCount[g];
      if (distCount) c.dcount(r) = distCount[g]; if (distDenCount) c.dden(r) = distDenCount[g];
      if (sumO) memcpy(c.sumO(r), sumO + (size_t) g * D, D * sizeof(double));
      if (sumOsq) memcpy(c.sumOsq(r), sumOsq + (size_t) g * D, D * sizeof(double));
    }
    t->push();
  });
}

dsr_status dsr_train_add(dsr_train* t, dsr_train* o, double factor)
{
  return guard([&] {
    if (!t || !o) throw Error(DSR_E_PARAMETER, "null argument");
    if (t->G != o->G || t->D != o->D || t->g->refN != o->g->refN) throw Error(DSR_E_DIMENSION, "accumulators of different shape");
    t->pull(); if (o != t) o->pull();
    const Rows c{t->D};
    for (int g = 0; g < t->G; g++) {
      double* r = t->row(g); double* s = o->row(g);
      const double dc = c.dcount(s), dd = c.dden(s);
      c.count(r) += factor * c.count(s); c.den(r) += factor * c.den(s);                                     // cT:396-397
      for (int d = 0; d < t->D; d++) { c.sumO(r)[d] += factor * c.sumO(s)[d]; c.sumOsq(r)[d] += factor * c.sumOsq(s)[d]; }   // cT:400-401
      c.dcount(r) += dc; c.dden(r) += dd;                                                                   // dT:258-259: no factor
    }
    t->push();
  });
}

dsr_status dsr_train_save_codebook_accus(dsr_train* t, const char* fileName, float totalPr, unsigned totalT, int countsOnly)
{
  return guard([&] {
    if (!t || !fileName) throw Error(DSR_E_PARAMETER, "null argument");
    t->pull(); const Rows c{t->D}; const GmmModel& m = *t->g; const int D = t->D;
    std::vector<char> live(m.K, 0); std::map<std::string, long> amap; long offset = 0;
    for (int k = 0; k < m.K; k++) {                        // AccMap(cbs, countsOnly) dT:357-373, zeroOccupancy cT:574-581, size cT:542-563
      for (int g = m.off[k]; g < m.off[k + 1]; g++) if (c.count(t->row(g)) != 0.0 || c.den(t->row(g)) != 0.0) live[k] = 1;
      if (!live[k]) continue;
      if (amap.count(m.cbNames[k])) throw Error(DSR_E_KEY, "Entry for %s is not unique.", m.cbNames[k].c_str());
      amap[m.cbNames[k]] = offset;
      long sz = 2L * m.refN[k] * 4; if (!countsOnly) sz += 2L * m.refN[k] * 4 * D;
      offset += sz + 2 + (long) m.cbNames[k].size() + 1 + 5 * 4 + 4;
    }
    BEFile f(fileName, "wb");
    f.wf(totalPr); f.w32((int) totalT);
    write_map(f, amap);
    for (int k = 0; k < m.K; k++) {
      if (!live[k]) continue;
      f.wstr(m.cbNames[k]); f.w32(m.refN[k]); f.w32(D); f.w32(1); f.w32(kCovDiagonal); f.w32(countsOnly ? 1 : 0);   // cT:299-307
      for (int g = m.off[k]; g < m.off[k + 1]; g++) {      // cT:326-346
        double* r = t->row(g);
        f.wf((float) c.count(r)); f.wf((float) c.den(r));
        if (countsOnly) continue;
        for (int d = 0; d < D; d++) f.wf((float) c.sumO(r)[d]);
        for (int d = 0; d < D; d++) f.wf((float) c.sumOsq(r)[d]);
      }
      f.w32(kCbMarker);
    }
  });
}

dsr_status dsr_train_load_codebook_accus(dsr_train* t, const char* fileName, float* totalPr, unsigned* totalT, float factor, int nParts, int part)
{
  return guard([&] {
    if (!t || !fileName) throw Error(DSR_E_PARAMETER, "null argument");
    const GmmModel& m = *t->g; const int D = t->D;
    int k0, k1; part_range(m.K, nParts, part, k0, k1);
    BEFile f(fileName, "rb");
    const float pr = f.f32(); const int tt = f.i32();
    const std::map<std::string, long> amap = read_map(f);
    const long startOfAccs = ftell(f.fp);
    t->pull(); const Rows c{D}; std::vector<double> work = t->h;      // a failed load leaves the accumulators as they were
    std::swap(work, t->h);
    try {
      for (int k = k0; k < k1; k++) {
        std::map<std::string, long>::const_iterator it = amap.find(m.cbNames[k]); if (it == amap.end()) continue;
        if (fseek(f.fp, startOfAccs + it->second, SEEK_SET)) throw Error(DSR_E_IO, "seek failed");
        (void) f.str();                                    // cT:369-390
        const int refN = f.i32(), dimN = f.i32(), subN = f.i32(), type = f.i32(); const bool countsOnly = f.i32() != 0;
        if (refN != m.refN[k]) throw Error(DSR_E_DIMENSION, "'refN' does not match (%d vs. %d)", refN, m.refN[k]);
        if (dimN != D) throw Error(DSR_E_DIMENSION, "'dimN' does not match (%d vs. %d)", dimN, D);
        if (subN != 1) throw Error(DSR_E_DIMENSION, "'subN' does not match (%d vs. %d)", subN, 1);
        if (type != kCovDiagonal) throw Error(DSR_E_DIMENSION, "'type' does not match (%d vs. %d)", type, kCovDiagonal);
        for (int g = m.off[k]; g < m.off[k + 1]; g++) {    // cT:407-426: float factor x float value, added in double
          double* r = t->row(g);
          c.count(r) += (double) (factor * f.f32()); c.den(r) += (double) (factor * f.f32());
          if (countsOnly) continue;
          for (int d = 0; d < D; d++) c.sumO(r)[d] += (double) (factor * f.f32());
          for (int d = 0; d < D; d++) c.sumOsq(r)[d] += (double) (factor * f.f32());
        }
        const int marker = f.i32();
        if (marker != kCbMarker) throw Error(DSR_E_IO, "CheckMarker: Marker expected in accu file (%d vs. %d).", marker, kCbMarker);
      }
    } catch (...) { std::swap(work, t->h); throw; }
    t->push();
    if (totalPr) *totalPr = pr; if (totalT) *totalT = (unsigned) tt;
  });
}

dsr_status dsr_train_save_distrib_accus(dsr_train* t, const char* fileName)
{
  return guard([&] {
    if (!t || !fileName) throw Error(DSR_E_PARAMETER, "null argument");
    t->pull(); const Rows c{t->D}; const GmmModel& m = *t->g;
    std::vector<char> live(m.K, 0); std::map<std::string, long> amap; long offset = 0;
    for (int k = 0; k < m.K; k++) {                        // AccMap(dss) dT:375-393, zeroOccupancy dT:230-237 ('> 0'), size dT:314-318
      for (int g = m.off[k]; g < m.off[k + 1]; g++) if (c.dcount(t->row(g)) > 0.0 || c.dden(t->row(g)) > 0.0) live[k] = 1;
      if (!live[k]) continue;
      if (amap.count(m.dsNames[k])) throw Error(DSR_E_KEY, "Entry for %s is not unique.", m.dsNames[k].c_str());
      amap[m.dsNames[k]] = offset; offset += 2L * m.refN[k] * 4 + 3 * 4;
    }
    BEFile f(fileName, "wb");
    write_map(f, amap);
    for (int k = 0; k < m.K; k++) {
      if (!live[k]) continue;
      f.w32(m.refN[k]); f.w32(1);                          // dT:239-252
      for (int g = m.off[k]; g < m.off[k + 1]; g++) { f.wf((float) c.dcount(t->row(g))); f.wf((float) c.dden(t->row(g))); }
      f.w32(kDsMarker);
    }
  });
}

dsr_status dsr_train_load_distrib_accus(dsr_train* t, const char* fileName, float factor, int nParts, int part)
{
  return guard([&] {
    if (!t || !fileName) throw Error(DSR_E_PARAMETER, "null argument");
    const GmmModel& m = *t->g;
    int k0, k1; part_range(m.K, nParts, part, k0, k1);
    BEFile f(fileName, "rb");
    const std::map<std::string, long> amap = read_map(f);
    const long startOfAccs = ftell(f.fp);
    t->pull(); const Rows c{t->D}; std::vector<double> work = t->h;
    std::swap(work, t->h);
    try {
      for (int k = k0; k < k1; k++) {
        std::map<std::string, long>::const_iterator it = amap.find(m.dsNames[k]); if (it == amap.end()) continue;
        if (fseek(f.fp, startOfAccs + it->second, SEEK_SET)) throw Error(DSR_E_IO, "seek failed");
        const int valN = f.i32(), subN = f.i32();            // dT:290-312
        if (valN != m.refN[k]) throw Error(DSR_E_DIMENSION, "Number of values do not match (%d vs. %d)", valN, m.refN[k]);
        if (subN != 1) throw Error(DSR_E_DIMENSION, "Number of sub-accumulators do not match (%d vs. %d)", subN, 1);
        for (int g = m.off[k]; g < m.off[k + 1]; g++) { double* r = t->row(g); c.dcount(r) += (double) (factor * f.f32()); c.dden(r) += (double) (factor * f.f32()); }
        if (f.i32() != kDsMarker) throw Error(DSR_E_ERROR, "CheckMarker: Marker expected in dump file.");
      }
    } catch (...) { std::swap(work, t->h); throw; }
    t->push();
  });
}

dsr_status dsr_train_update(dsr_train* t, int what, int nParts, int part)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    GmmModel& m = *t->g; const int D = t->D; const Rows c{D};
    int k0, k1; part_range(m.K, nParts, part, k0, k1);
    t->pull();
    if (what & 1)
      for (int g = m.off[k0]; g < m.off[k1]; g++) {        // cT:448-490
        double* r = t->row(g);
        const float cnt = (float) c.count(r); m.count[g] = cnt;
        if ((double) cnt <= t->minCount) continue;
        for (int d = 0; d < D; d++) {
          const float mean = (float) (c.sumO(r)[d] / (double) cnt); m.mean[(size_t) g * D + d] = mean;
          const double mu = (double) mean;
          m.ivar[(size_t) g * D + d] = (float) ((c.sumOsq(r)[d] / (double) cnt) - (mu * mu));
        }
      }
    if (what & 2)
      for (int k = k0; k < k1; k++) {                      // dT:146-156, PaddingValue 1e-4
        double ttl = 0.0;
        for (int g = m.off[k]; g < m.off[k + 1]; g++) ttl += (c.dcount(t->row(g)) + 1.0E-04);
        for (int g = m.off[k]; g < m.off[k + 1]; g++) m.val[g] = (float) -log((c.dcount(t->row(g)) + 1.0E-04) / ttl);
      }
    reupload(m);
  });
}

dsr_status dsr_train_update_mmi(dsr_train* t, int what, double E, int merialdo, int nParts, int part)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    GmmModel& m = *t->g; const int D = t->D; const Rows c{D};
    int k0, k1; part_range(m.K, nParts, part, k0, k1);
    t->pull();
    const double pad = 1.0E-04;
    std::vector<float> val = m.val;                        // a consistency error leaves the model as it was
    if (what & 2)
      for (int k = k0; k < k1; k++) {
        const int a = m.off[k], b = m.off[k + 1];
        if (!merialdo) {                                   // dT:166-190
          double Cc = pad;
          for (int g = a; g < b; g++) { const double deriv = -(1.0 + pad) * ((c.dcount(t->row(g)) - c.dden(t->row(g))) * exp((double) val[g])); if (deriv > Cc) Cc = deriv; }
          double ttl = 0.0;
          for (int g = a; g < b; g++) {
            const double cnt = (c.dcount(t->row(g)) - c.dden(t->row(g))) + Cc * exp(-(double) val[g]);
            if (cnt < 0.0) throw Error(DSR_E_CONSISTENCY, "Count (%g) is negative; C = %g.\n", cnt, Cc);
            ttl += cnt;
          }
          for (int g = a; g < b; g++) {
            const double cnt = (c.dcount(t->row(g)) - c.dden(t->row(g))) + Cc * exp(-(double) val[g]);
            val[g] = (float) -log(cnt / ttl);
            if (std::isnan(val[g])) throw Error(DSR_E_CONSISTENCY, "Weight is NaN : ttlCnt = %g.\n", ttl);
          }
        } else {                                           // dT:192-222
          double tn = 0.0, td = 0.0;
          for (int g = a; g < b; g++) { tn += c.dcount(t->row(g)) + pad; td += c.dden(t->row(g)) + pad; }
          double Cc = 0.0;
          for (int g = a; g < b; g++) { const double deriv = -(1.0 + pad) * (((c.dcount(t->row(g)) + pad) / tn) - ((c.dden(t->row(g)) + pad) / td)); if (deriv > Cc) Cc = deriv; }
          double ttl = 0.0;
          for (int g = a; g < b; g++) {
            const double cnt = (((c.dcount(t->row(g)) + pad) / tn) - ((c.dden(t->row(g)) + pad) / td) + Cc) * exp(-(double) val[g]) + pad;
            if (cnt < 0.0) throw Error(DSR_E_CONSISTENCY, "Count (%g) < 0.0 : C = %g.\n", cnt, Cc);
            ttl += cnt;
          }
          for (int g = a; g < b; g++) {
            const double cnt = (((c.dcount(t->row(g)) + pad) / tn) - ((c.dden(t->row(g)) + pad) / td) + Cc) * exp(-(double) val[g]) + pad;
            val[g] = (float) -log(cnt / ttl);
            if (std::isnan(val[g])) throw Error(DSR_E_CONSISTENCY, "Weight is NaN : ttlCnt = %g.\n", ttl);
          }
        }
      }
    if (what & 1)
      for (int g = m.off[k0]; g < m.off[k1]; g++) {        // cT:448-456, 492-518: the model's covariance slot holds inverse variances on entry
        double* r = t->row(g);
        const float cnt = (float) c.count(r); m.count[g] = cnt;
        float* mean = &m.mean[(size_t) g * D]; float* cv = &m.ivar[(size_t) g * D];
        if ((double) cnt <= t->minCount) { for (int d = 0; d < D; d++) cv[d] = (float) (1.0 / (double) cv[d]); continue; }
        const double Dd = E * c.den(r), denom = c.count(r) - c.den(r) + Dd;
        for (int d = 0; d < D; d++) {
          const float mu = mean[d], sigma = (float) (1.0 / (double) cv[d]);
          const float musum = (float) (c.sumO(r)[d] + (double) mu * Dd);
          const float muhat = (float) ((double) musum / denom);
          const float sigmasum = (float) (c.sumOsq(r)[d] + (double) (sigma + mu * mu) * Dd);
          const float sigmahat = (float) ((double) sigmasum / denom - (double) (muhat * muhat));
          mean[d] = muhat; cv[d] = sigmahat;
        }
      }
    m.val = val;
    reupload(m);
  });
}

dsr_status dsr_train_floor_variances(dsr_train* t, int nParts, int part, unsigned* total, unsigned* floored)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    GmmModel& m = *t->g; int k0, k1; part_range(m.K, nParts, part, k0, k1);
    const float floorV = 1.0E-04f; unsigned n = 0, nf = 0;  // gblVarFloor, cT:732, 786-798
    for (size_t i = (size_t) m.off[k0] * m.D; i < (size_t) m.off[k1] * m.D; i++) { n++; if (m.ivar[i] < floorV) { m.ivar[i] = floorV; nf++; } }
    if (total) *total += n; if (floored) *floored += nf;
    reupload(m);
  });
}

dsr_status dsr_train_fix_gconsts(dsr_train* t, int nParts, int part)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    GmmModel& m = *t->g; int k0, k1; part_range(m.K, nParts, part, k0, k1);
    for (int g = m.off[k0]; g < m.off[k1]; g++) {          // cT:228-241
      double logDet = 0.0;
      for (int d = 0; d < m.D; d++) logDet += log((double) m.ivar[(size_t) g * m.D + d]);
      if (std::isnan(logDet)) throw Error(DSR_E_CONSISTENCY, "Determinant is NaN");
      m.det[g] = (float) logDet;
    }
    reupload(m);
  });
}

dsr_status dsr_train_invert_variances(dsr_train* t, int nParts, int part)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    GmmModel& m = *t->g; int k0, k1; part_range(m.K, nParts, part, k0, k1);
    for (size_t i = (size_t) m.off[k0] * m.D; i < (size_t) m.off[k1] * m.D; i++) m.ivar[i] = (float) (1.0 / (double) m.ivar[i]);   // cT:218-223
    reupload(m);
  });
}

dsr_status dsr_train_split(dsr_train* t, int distX, float minCount, float splitFactor, unsigned* refXOut)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    GmmModel& m = *t->g; const int D = m.D;
    if (distX < 0 || distX >= m.K) throw Error(DSR_E_INDEX, "distribution %d of %d", distX, m.K);
    const int a = m.off[distX], R = m.refN[distX];
    int maxIdx = 0; float maxCount = m.count[a];            // cT:122-142
    for (int r = 1; r < R; r++) if (m.count[a + r] > maxCount) { maxCount = m.count[a + r]; maxIdx = r; }
    if (minCount > 0.0 && maxCount < minCount)
      throw Error(DSR_E_PARAMETER, "Cannot split codebook %s; maxCount (%f) < minCount (%f)\n.", m.cbNames[distX].c_str(), maxCount, minCount);
    if (R >= 256) throw Error(DSR_E_DIMENSION, "codebook %s already has 256 Gaussians (CBX is unsigned char)", m.cbNames[distX].c_str());
    t->pull();
    const int src = a + maxIdx, at = a + R;                // the new Gaussian goes to the end of its codebook (cT:144-198)
    std::vector<float> nm(D), nv(D);
    for (int d = 0; d < D; d++) {
      const float perturb = (float) ((double) splitFactor / sqrt((double) m.ivar[(size_t) src * D + d]));
      nm[d] = m.mean[(size_t) src * D + d] - perturb; m.mean[(size_t) src * D + d] = m.mean[(size_t) src * D + d] + perturb;
      nv[d] = m.ivar[(size_t) src * D + d];
    }
    m.mean.insert(m.mean.begin() + (size_t) at * D, nm.begin(), nm.end());
    m.ivar.insert(m.ivar.begin() + (size_t) at * D, nv.begin(), nv.end());
    m.det.insert(m.det.begin() + at, m.det[src]);
    const float half = (float) ((double) m.count[src] / 2.0);
    m.count[src] = half; m.count.insert(m.count.begin() + at, half);
    const float nval = (float) ((double) m.val[src] + log(2.0));               // dT:99-100
    m.val[src] = nval; m.val.insert(m.val.begin() + at, nval);
    if (!m.regClass.empty()) m.regClass.insert(m.regClass.begin() + at, m.regClass[src]);       // the new Gaussian is of its parent's class
    m.refN[distX] = R + 1;
    reupload(m);                                            // offsets, G, device copies
    // fresh accumulators for this codebook and distribution (cT:183, dT:106), everybody else's rows move up
    std::vector<double> nh((size_t) m.G * t->NA, 0.0);
    memcpy(nh.data(), t->h.data(), (size_t) a * t->NA * sizeof(double));
    memcpy(nh.data() + (size_t) (at + 1) * t->NA, t->h.data() + (size_t) at * t->NA, (size_t) (t->G - at) * t->NA * sizeof(double));
    t->h.swap(nh); t->G = m.G; t->push();
    if (refXOut) *refXOut = (unsigned) maxIdx;
  });
}

dsr_status dsr_gmm_get_params(const dsr_gmm* m, int32_t* refN, float* mean, float* cv, float* det, float* val, float* count)
{
  return guard([&] {
    if (!m) throw Error(DSR_E_PARAMETER, "null argument");
    if (refN) for (int k = 0; k < m->K; k++) refN[k] = m->refN[k];
    if (mean) memcpy(mean, m->mean.data(), m->mean.size() * sizeof(float));
    if (cv) memcpy(cv, m->ivar.data(), m->ivar.size() * sizeof(float));
    if (det) memcpy(det, m->det.data(), m->det.size() * sizeof(float));
    if (val) memcpy(val, m->val.data(), m->val.size() * sizeof(float));
    if (count) memcpy(count, m->count.data(), m->count.size() * sizeof(float));
  });
}

}  // extern "C"
