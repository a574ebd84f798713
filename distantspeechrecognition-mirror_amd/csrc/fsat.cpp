// csrc/fsat.cpp -- the host side of fast speaker-adaptive training: the handle over a dsr_sat, the fast accumulators and their file, the
// update's bookkeeping, the description lengths and the file-driven estimate.
//
// Replaces CodebookFastSAT::FastAccu::save / load (asr/sat/codebookFastSAT.cc:175-253, "cfs"), GaussDensity::descLen (cfs:523-539), AccMap
// (cfs:544-566), CodebookSetFastSAT::saveFastAccus / loadFastAccus / zeroFastAccus / descLength / normFastAccus / setRegClassesToOne
// (cfs:597-717), SATBase::FastAcc::accumulate / update / addFastAcc (asr/sat/sat.cc:1067-1104, "sat"), the bookkeeping of MDLSATMean::update
// (sat:395-462), SATFast<Type>::estimate / addFastAccs (sat.h:825-842) and SATBase::estimate (sat:1802-1839).  The arithmetic over the
// statistics is in fsat_kernels.hip and sat_kernels.hip.  Compiled with -ffp-contract=off.
#include "common.h"
#include "adapt.h"
#include "apt.h"
#include "train.h"
#include "befile.h"
#include "fsat.h"
#include <algorithm>
#include <cmath>

namespace dsr {
namespace {

void need(const FsatHandle* f) { if (!f) throw Error(DSR_E_PARAMETER, "null argument"); }
void check_slot(const FsatHandle& f, int s) { if (s < 0 || s >= f.S) throw Error(DSR_E_INDEX, "slot %d of %d", s, f.S); }
void pass(dsr_status st) { if (st) throw Error(st, "%s", dsr_last_error()); }

void check_model(const FsatHandle& f)
{
  const SatHandle& h = *f.sat;
  if (h.g->G != h.G || h.g->D != h.D || h.tr->G != h.G) throw Error(DSR_E_DIMENSION, "the model changed shape under the SAT handle (%d x %d, now %d x %d)", h.G, h.D, h.g->G, h.g->D);
}

void check_blocks(const FsatHandle& f, int nB)
{
  if (nB < 1 || f.D % nB != 0) throw Error(DSR_E_DIMENSION, "Feature length %d is not compatible with %d blocks.", f.D, nB);
  if (f.D / nB > kSatMaxBlock) throw Error(DSR_E_DIMENSION, "block length %d: SAT is built for blocks of at most %d", f.D / nB, kSatMaxBlock);
}

// GaussDensity::descLen (cfs:523-539): allocated when the block count is first known, every block at 1
void need_desc(FsatHandle& f, int nB)
{
  if (!f.descBlocks) { f.descBlocks = nB; f.descLen.assign((size_t) f.G * nB, 1); }
  else if (f.descBlocks != nB) throw Error(DSR_E_DIMENSION, "description lengths of %d blocks for statistics of %d", f.descBlocks, nB);
}

unsigned desc_length(const FsatHandle& f)                 // cfs:654-673; before the block count is known: nSubFeat blocks at 1
{
  if (!f.descBlocks) return (unsigned) f.G * (unsigned) f.sat->aptSub;
  unsigned dl = 0; for (size_t i = 0; i < f.descLen.size(); i++) dl += f.descLen[i];
  return dl;
}

void alloc_fast(FsatHandle& f, int nB)                    // reallocFastAccu + zeroFastAccu, cfs:688-695
{
  check_blocks(f, nB);
  const size_t G = f.G, D = f.D;
  f.d_fcount.reserve(G); f.d_fden.reserve(G); f.d_fmean.reserve(G * D); f.d_fvar.reserve(G * D); f.d_fscalar.reserve(G * nB);
  DSR_HIP(hipDeviceSynchronize());
  DSR_HIP(hipMemset(f.d_fcount.p, 0, G * sizeof(double))); DSR_HIP(hipMemset(f.d_fden.p, 0, G * sizeof(double)));
  DSR_HIP(hipMemset(f.d_fmean.p, 0, G * D * sizeof(double))); DSR_HIP(hipMemset(f.d_fvar.p, 0, G * D * sizeof(double)));
  DSR_HIP(hipMemset(f.d_fscalar.p, 0, G * nB * sizeof(double)));
  f.fastBlocks = nB;
}

struct FastHost { std::vector<double> count, den, mean, var, scalar; };

void pull_fast(FsatHandle& f, FastHost& a)
{
  if (!f.fastBlocks) throw Error(DSR_E_CONSISTENCY, "no fast accumulators: call dsr_fsat_norm, dsr_fsat_load_fast or dsr_fsat_set_fast first");
  const size_t G = f.G, D = f.D, nB = f.fastBlocks;
  a.count.resize(G); a.den.resize(G); a.mean.resize(G * D); a.var.resize(G * D); a.scalar.resize(G * nB);
  DSR_HIP(hipDeviceSynchronize());
  DSR_HIP(hipMemcpy(a.count.data(), f.d_fcount.p, G * sizeof(double), hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(a.den.data(), f.d_fden.p, G * sizeof(double), hipMemcpyDeviceToHost));
  DSR_HIP(hipMemcpy(a.mean.data(), f.d_fmean.p, G * D * sizeof(double), hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(a.var.data(), f.d_fvar.p, G * D * sizeof(double), hipMemcpyDeviceToHost));
  DSR_HIP(hipMemcpy(a.scalar.data(), f.d_fscalar.p, G * nB * sizeof(double), hipMemcpyDeviceToHost));
}

void push_fast(FsatHandle& f, const FastHost& a)
{
  DSR_HIP(hipDeviceSynchronize());
  f.d_fcount.upload(a.count); f.d_fden.upload(a.den); f.d_fmean.upload(a.mean); f.d_fvar.upload(a.var); f.d_fscalar.upload(a.scalar);
}

bool take_flag(FsatHandle& f)
{
  int flag = 0; DSR_HIP(hipMemcpy(&flag, f.d_flag.p, sizeof(int), hipMemcpyDeviceToHost));
  if (flag) DSR_HIP(hipMemset(f.d_flag.p, 0, sizeof(int)));
  return flag != 0;
}

void set_reg_classes_to_one(FsatHandle& f)                // cfs:708-717
{
  GmmModel& m = *f.sat->g;
  if (m.regClass.empty()) m.regClass.assign(m.G, 1);
  for (size_t g = 0; g < m.regClass.size(); g++) if (m.regClass[g] == 0) m.regClass[g] = 1;
}

void put_counts(FsatHandle& f, int s, const double* num, const double* den)
{
  SatHandle& h = *f.sat; const size_t G = f.G; std::vector<double> c(G);
  for (size_t g = 0; g < G; g++) c[g] = num[g] - den[g];  // postProb(), codebookTrain.h:142-144
  DSR_HIP(hipDeviceSynchronize());
  DSR_HIP(hipMemcpy(f.d_num.p + s * G, num, G * sizeof(double), hipMemcpyHostToDevice)); DSR_HIP(hipMemcpy(f.d_den.p + s * G, den, G * sizeof(double), hipMemcpyHostToDevice));
  DSR_HIP(hipMemcpy(h.d_c.p + s * G, c.data(), G * sizeof(double), hipMemcpyHostToDevice));
}

// the counts of a trainer into slot s: numProb and denProb device to device, count - denCount through the host
void take_counts(FsatHandle& f, int s, const dsr_train& t)
{
  fsat_take_counts(f, s, t);
  const size_t G = f.G; std::vector<double> num(G), den(G);
  DSR_HIP(hipMemcpy(num.data(), f.d_num.p + s * G, G * sizeof(double), hipMemcpyDeviceToHost)); DSR_HIP(hipMemcpy(den.data(), f.d_den.p + s * G, G * sizeof(double), hipMemcpyDeviceToHost));
  put_counts(f, s, num.data(), den.data());
}

void norm(FsatHandle& f, int nSlots, hipStream_t st)      // CodebookSetFastSAT::normFastAccus, cfs:677-705
{
  SatHandle& h = *f.sat;
  if (nSlots < 1 || nSlots > f.S) throw Error(DSR_E_INDEX, "%d slots of %d", nSlots, f.S);
  check_model(f);
  for (int s = 0; s < nSlots; s++) if (!f.full[s]) throw Error(DSR_E_CONSISTENCY, "slot %d holds counts only: the fast accumulators need sumO and sumOsq", s);
  set_reg_classes_to_one(f);
  SatCall c; std::vector<int> gidx, tile;
  sat_tables(h, nSlots, 0, f.G, c, gidx, tile, st);       // every codebook, no parts (cfs:697-702); the refusals come before anything is added
  if (f.fastBlocks && c.nB != f.fastBlocks) throw Error(DSR_E_DIMENSION, "'nblks' does not match (%d vs. %d)", c.nB, f.fastBlocks);
  if (f.descBlocks && c.nB != f.descBlocks) throw Error(DSR_E_DIMENSION, "description lengths of %d blocks for transforms of %d", f.descBlocks, c.nB);
  if (!f.fastBlocks) alloc_fast(f, c.nB);
  need_desc(f, c.nB);
  h.d_gidx.upload(gidx, st); h.d_tile.upload(tile, st); h.d_mean.upload(h.g->mean, st); h.d_ivar.upload(h.g->ivar, st);
  fsat_norm(f, c, st);
  DSR_HIP(hipStreamSynchronize(st));
  if (take_flag(f)) throw Error(DSR_E_NUMERIC, "Scalar is NaN.");                                      // cfs:407-408
}

void add_fast(FsatHandle& f)                              // SATFast::addFastAccs, sat.h:833-842
{
  SatHandle& h = *f.sat;
  if (!f.fastBlocks) throw Error(DSR_E_CONSISTENCY, "no fast accumulators: call dsr_fsat_norm, dsr_fsat_load_fast or dsr_fsat_set_fast first");
  check_model(f);
  const int nB = f.fastBlocks, bl = f.D / nB;
  if (h.nBlocks && h.nBlocks != nB) throw Error(DSR_E_DIMENSION, "Block sizes (%d vs %d) are not equivalent.", nB, h.nBlocks);
  need_desc(f, nB);
  if (!h.nBlocks) {                                       // _checkBlocks(nblks, allocVarVec), sat:533
    const size_t words = (size_t) f.G * nB * ((size_t) bl * bl + bl + 1);
    h.d_macc.reserve(words); DSR_HIP(hipMemset(h.d_macc.p, 0, words * sizeof(double)));
    h.nBlocks = nB; h.bl = bl;
  }
  fsat_add(f, nullptr);
  DSR_HIP(hipDeviceSynchronize());
  if (take_flag(f)) throw Error(DSR_E_NUMERIC, "Scalar is NaN.");                                      // sat:547-548
}

void accumulate(FsatHandle& f, int nSlots, hipStream_t st)   // FastAcc::accumulate, sat:1067-1077
{
  sat_accumulate(*f.sat, kSatMean, true, nSlots, st);
  f.ms[1] = f.sat->ms[0];
  if (f.sat->nBlocks) need_desc(f, f.sat->nBlocks);
}

float inverse(float v) { return (float) (1.0 / (double) v); }          // satVar(n) = 1.0 / satVar(n)

void update(FsatHandle& f, unsigned info[4], unsigned totals[2], double* aux)
{
  SatHandle& h = *f.sat; check_model(f);
  GmmModel& m = *h.g; const int D = h.D, G = h.G, nB = h.nBlocks, bl = h.bl;
  if (nB) need_desc(f, nB);
  int g0, g1; sat_part_gaussians(h, g0, g1);
  DSR_HIP(hipDeviceSynchronize());
  std::vector<double> occ(G), vvec((size_t) G * D); std::vector<int> has(G);
  DSR_HIP(hipMemcpy(occ.data(), h.d_mocc.p, G * sizeof(double), hipMemcpyDeviceToHost));
  DSR_HIP(hipMemcpy(has.data(), h.d_has.p, G * sizeof(int), hipMemcpyDeviceToHost));
  DSR_HIP(hipMemcpy(vvec.data(), h.d_vvec.p, vvec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unsigned inf[4] = {0, 0, 0, 0}, tot[2] = {0, 0}; double auxSum = 0.0;
  h.rec.assign((size_t) G * std::max(nB, 1), SatRecord{0, kSatLeft, 0.0, 0.0}); h.status.assign(G, 0);
  f.recDesc.assign((size_t) G * std::max(nB, 1), 0);
  if (nB) for (size_t i = 0; i < f.descLen.size(); i++) f.recDesc[i] = f.descLen[i];
  std::vector<float> ivar = m.ivar; std::vector<int> solve, zeroed;
  for (int g = g0; g < g1; g++) {                         // FastAcc::update, sat:1079-1099
    tot[0]++;
    if (occ[g] < h.threshold) { for (int d = 0; d < D; d++) ivar[(size_t) g * D + d] = inverse(m.ivar[(size_t) g * D + d]); continue; }    // sat:1088-1093
    tot[1]++;
    if (!has[g] || !nB) continue;                         // no blocks: FastSAT::update walks none, the covariance slot stays as it is
    if (occ[g] == 0.0) zeroed.push_back(g); else solve.push_back(g);
  }
  std::vector<float> newMean = m.mean, newVar; std::vector<int> newDesc; h.sol.assign((size_t) G * D, 0.0);
  if (!solve.empty()) {
    std::vector<SatRecord> rec((size_t) G * nB); std::vector<int> desc(f.descLen.begin(), f.descLen.end());
    newVar.resize((size_t) G * D); newDesc.resize((size_t) G * nB);
    h.d_solve.upload(solve); h.d_mean.upload(m.mean); h.d_newMean.upload(m.mean); h.d_ivar.upload(m.ivar); h.d_rec.reserve(rec.size());
    f.d_desc.upload(desc); f.d_newDesc.reserve(newDesc.size()); f.d_newVar.reserve(newVar.size());
    h.d_sol.reserve(h.sol.size()); DSR_HIP(hipMemset(h.d_sol.p, 0, h.sol.size() * sizeof(double)));
    fsat_solve(f, (int) solve.size(), nullptr);
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(newMean.data(), h.d_newMean.p, newMean.size() * sizeof(float), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(newVar.data(), f.d_newVar.p, newVar.size() * sizeof(float), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(newDesc.data(), f.d_newDesc.p, newDesc.size() * sizeof(int), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(rec.data(), h.d_rec.p, rec.size() * sizeof(SatRecord), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(h.sol.data(), h.d_sol.p, h.sol.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < solve.size(); i++) for (int nb = 0; nb < nB; nb++) h.rec[(size_t) solve[i] * nB + nb] = rec[(size_t) solve[i] * nB + nb];
  }
  for (size_t i = 0; i < zeroed.size(); i++) {            // occ == 0: the variances (sat:555-560), then the mean zeroed (sat:399-407)
    const int g = zeroed[i];
    for (int d = 0; d < D; d++) {
      const size_t k = (size_t) g * D + d; const double var = vvec[k] / occ[g];
      ivar[k] = (f.meanOnly || std::isnan(var)) ? inverse(m.ivar[k]) : (float) var;
      m.mean[k] = 0.0f;
    }
    for (int nb = 0; nb < nB; nb++) h.rec[(size_t) g * nB + nb].decision = kSatZeroed;
  }
  int nFlag = 0, firstFlag = -1, nNaN = 0, firstNaN = -1;
  for (size_t i = 0; i < solve.size(); i++) {             // model order
    const int g = solve[i]; const SatRecord* r = &h.rec[(size_t) g * nB];
    for (int nb = 0; nb < nB; nb++) {
      if (r[nb].decision == kSatFlagged && !h.status[g]) { h.status[g] = DSR_E_CONSISTENCY; if (!nFlag++) firstFlag = g; }
      if (r[nb].decision == kSatNaN && !h.status[g]) { h.status[g] = DSR_E_NUMERIC; if (!nNaN++) firstNaN = g; }
    }
    if (h.status[g]) {                                    // its mean and description lengths stay; the slot holds its old variance
      for (int d = 0; d < D; d++) ivar[(size_t) g * D + d] = inverse(m.ivar[(size_t) g * D + d]);
      continue;
    }
    std::copy(newVar.begin() + (size_t) g * D, newVar.begin() + (size_t) (g + 1) * D, ivar.begin() + (size_t) g * D);
    for (int nb = 0; nb < nB; nb++) {                     // UpdateInfo, sat:411, 439-458, 485, 492
      if (r[nb].decision == kSatKeptOld) { auxSum += r[nb].auxOld; inf[0]++; continue; }
      std::copy(newMean.begin() + (size_t) g * D + nb * bl, newMean.begin() + (size_t) g * D + (nb + 1) * bl, m.mean.begin() + (size_t) g * D + nb * bl);
      f.descLen[(size_t) g * nB + nb] = (uint16_t) newDesc[(size_t) g * nB + nb]; f.recDesc[(size_t) g * nB + nb] = newDesc[(size_t) g * nB + nb];
      auxSum += r[nb].auxNew; inf[0]++; inf[1]++; inf[2] += bl; inf[3] += r[nb].kept;
    }
  }
  m.ivar.swap(ivar);
  gmm_finish(m);
  if (info) std::copy(inf, inf + 4, info); if (totals) std::copy(tot, tot + 2, totals); if (aux) *aux = auxSum;
  if (nFlag) throw Error(DSR_E_CONSISTENCY, "SAT statistics of %d Gaussian(s), the first %d, are not finite or their eigen-decomposition did not converge", nFlag, firstFlag);
  if (nNaN) throw Error(DSR_E_NUMERIC, "Degenerate value in a mean component of %d Gaussian(s), the first %d", nNaN, firstNaN);
}

// the size of one codebook's record: Accu::_size with rv of orgDimN (cT:542-563), orgDimN, nblks and the scalars (cfs:241-254)
long fast_size(const std::string& name, int refN, int D, int nB)
{
  return 2L * refN * 4 + 2L * refN * 4 * D + 2 + (long) name.size() + 1 + 5 * 4 + 4 + 2 * 4 + (long) refN * nB * 4;
}

void save_fast(FsatHandle& f, const char* fileName)       // cfs:597-617, 175-202
{
  FastHost a; pull_fast(f, a);
  const GmmModel& m = *f.sat->g; const int D = f.D, nB = f.fastBlocks;
  std::vector<char> live(m.K, 0); std::map<std::string, long> amap; long offset = 0;
  for (int k = 0; k < m.K; k++) {                         // AccMap(cbs, fastAccusFlag), cfs:544-566
    for (int g = m.off[k]; g < m.off[k + 1]; g++) if (a.count[g] != 0.0 || a.den[g] != 0.0) live[k] = 1;
    if (!live[k]) continue;
    if (amap.count(m.cbNames[k])) throw Error(DSR_E_KEY, "Entry for %s is not unique.", m.cbNames[k].c_str());
    amap[m.cbNames[k]] = offset; offset += fast_size(m.cbNames[k], m.refN[k], D, nB);
  }
  BEFile file(fileName, "wb");
  write_map(file, amap);
  for (int k = 0; k < m.K; k++) {
    if (!live[k]) continue;
    file.wstr(m.cbNames[k]); file.w32(m.refN[k]); file.w32(D); file.w32(1); file.w32(kCovDiagonal); file.w32(0); file.w32(D); file.w32(nB);
    for (int g = m.off[k]; g < m.off[k + 1]; g++) {
      file.wf((float) a.count[g]); file.wf((float) a.den[g]);
      for (int d = 0; d < D; d++) file.wf((float) a.mean[(size_t) g * D + d]);
      for (int d = 0; d < D; d++) file.wf((float) a.var[(size_t) g * D + d]);
    }
    for (int g = m.off[k]; g < m.off[k + 1]; g++) for (int nb = 0; nb < nB; nb++) file.wf((float) a.scalar[(size_t) g * nB + nb]);
    file.w32(kCbMarker);
  }
}

void load_fast(FsatHandle& f, const char* fileName, int nParts, int part)   // cfs:619-644, 204-239: the file is ADDED
{
  const GmmModel& m = *f.sat->g; const int D = f.D;
  int k0, k1; part_range(m.K, nParts, part, k0, k1);
  BEFile file(fileName, "rb");
  const std::map<std::string, long> amap = read_map(file);
  const long startOfAccs = ftell(file.fp);
  FastHost a; int nB = f.fastBlocks;
  if (nB) pull_fast(f, a);
  for (int k = k0; k < k1; k++) {
    std::map<std::string, long>::const_iterator it = amap.find(m.cbNames[k]); if (it == amap.end()) continue;
    if (fseek(file.fp, startOfAccs + it->second, SEEK_SET)) throw Error(DSR_E_IO, "seek failed");
    (void) file.str();
    const int refN = file.i32(), dimN = file.i32(), subN = file.i32(), type = file.i32(); const bool countsOnly = file.i32() != 0;
    if (refN != m.refN[k]) throw Error(DSR_E_DIMENSION, "'refN' does not match (%d vs. %d)", refN, m.refN[k]);
    if (dimN != D) throw Error(DSR_E_DIMENSION, "'dimN' does not match (%d vs. %d)", dimN, D);
    if (subN != 1) throw Error(DSR_E_DIMENSION, "'subN' does not match (%d vs. %d)", subN, 1);
    if (type != kCovDiagonal) throw Error(DSR_E_DIMENSION, "'type' does not match (%d vs. %d)", type, kCovDiagonal);
    if (countsOnly) throw Error(DSR_E_CONSISTENCY, "Mean and variance statistics must be included in fast accumulators.");
    const int orgDimN = file.i32(), nblks = file.i32();
    if (orgDimN != D) throw Error(DSR_E_DIMENSION, "'orgDimN' does not match (%d vs. %d)", orgDimN, D);
    if (!nB) {                                            // a handle without fast accumulators takes the file's block count
      check_blocks(f, nblks); nB = nblks; const size_t G = f.G;
      a.count.assign(G, 0.0); a.den.assign(G, 0.0); a.mean.assign(G * D, 0.0); a.var.assign(G * D, 0.0); a.scalar.assign(G * nB, 0.0);
    }
    if (nblks != nB) throw Error(DSR_E_DIMENSION, "'nblks' does not match (%d vs. %d)", nblks, nB);
    const float factor = 1.0f;
    for (int g = m.off[k]; g < m.off[k + 1]; g++) {       // cT:407-426: float factor x float value, added in double
      a.count[g] += (double) (factor * file.f32()); a.den[g] += (double) (factor * file.f32());
      for (int d = 0; d < D; d++) a.mean[(size_t) g * D + d] += (double) (factor * file.f32());
      for (int d = 0; d < D; d++) a.var[(size_t) g * D + d] += (double) (factor * file.f32());
    }
    for (int g = m.off[k]; g < m.off[k + 1]; g++) for (int nb = 0; nb < nB; nb++) a.scalar[(size_t) g * nB + nb] += (double) (factor * file.f32());
    const int marker = file.i32();
    if (marker != kCbMarker) throw Error(DSR_E_IO, "CheckMarker: Marker expected in accu file (%d vs. %d).", marker, kCbMarker);
  }
  if (!nB) return;                                        // nothing of this part in the file
  if (f.descBlocks && f.descBlocks != nB) throw Error(DSR_E_DIMENSION, "description lengths of %d blocks for a file of %d", f.descBlocks, nB);
  if (!f.fastBlocks) alloc_fast(f, nB);
  need_desc(f, nB);
  push_fast(f, a);                                        // a failed load leaves the accumulators as they were
}

double estimate_files(FsatHandle& f, const char* speakerList, const char* paramPrefix, const char* accuPrefix)
{
  SatHandle& h = *f.sat;
  const std::vector<std::string> list = read_speaker_list(speakerList);
  add_fast(f);                                            // sat.h:829
  int totalT = 0; double totalPr = f.lhoodThreshold * desc_length(f);                                 // sat:1805-1806
  pass(dsr_train_zero(h.tr, 1, h.nParts, h.part));
  int filled = 0;
  for (size_t i = 0; i < list.size(); i++) {              // sat:1816-1834; S speakers a batch, in list order
    float pr = 0.f; unsigned tt = 0;
    const std::string accu = std::string(accuPrefix) + list[i] + ".cbs.accu";
    pass(dsr_train_load_codebook_accus(h.tr, accu.c_str(), &pr, &tt, 1.0f, h.nParts, h.part));       // counts-only or full
    totalPr += (double) pr; totalT += (int) tt;
    sat_read_params(h, filled, std::string(paramPrefix) + list[i]);
    take_counts(f, filled, *h.tr); f.full[filled] = 0;
    pass(dsr_train_zero(h.tr, 1, h.nParts, h.part));
    if (++filled == f.S || i + 1 == list.size()) { accumulate(f, filled, nullptr); filled = 0; }
  }
  update(f, nullptr, nullptr, nullptr);
  return totalPr / totalT;
}

}  // namespace
}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_fsat_check(int meanLen, int featLen, double massThreshold, double mmiMultiplier, int meanOnly, int maxNoRegClass)
{
  return guard([&] {
    (void) meanOnly;
    if (meanLen != 0 && meanLen != featLen) throw Error(DSR_E_DIMENSION, "mean length %d for features of %d: extended means are not implemented", meanLen, featLen);
    if (massThreshold != massThreshold) throw Error(DSR_E_PARAMETER, "mass threshold is not a number");
    if (mmiMultiplier != 1.0) throw Error(DSR_E_PARAMETER, "mmiMultiplier = %g: it acts in the MMI accumulators only, which are not implemented", mmiMultiplier);
    if (maxNoRegClass != 1) throw Error(DSR_E_PARAMETER, "maxNoRegClass = %d: it acts in RegClassAcc only, which is not implemented", maxNoRegClass);
  });
}

dsr_status dsr_fsat_create(dsr_train* t, int S, double lhoodThreshold, double massThreshold, int nParts, int part, int meanOnly, dsr_fsat** out)
{
  return guard([&] {
    if (!t || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (lhoodThreshold != lhoodThreshold) throw Error(DSR_E_PARAMETER, "likelihood threshold is not a number");
    dsr_sat* s = nullptr; pass(dsr_sat_create(t, S, massThreshold, nParts, part, &s));
    dsr_fsat* f = new dsr_fsat();
    try {
      f->sat = s; f->S = s->S; f->D = s->D; f->G = s->G; f->lhoodThreshold = lhoodThreshold; f->meanOnly = meanOnly != 0;
      f->full.assign(f->S, 0);
      const size_t n = (size_t) f->S * f->G;
      f->d_num.reserve(n); f->d_den.reserve(n); f->d_flag.reserve(1);
      DSR_HIP(hipMemset(f->d_num.p, 0, n * sizeof(double))); DSR_HIP(hipMemset(f->d_den.p, 0, n * sizeof(double))); DSR_HIP(hipMemset(f->d_flag.p, 0, sizeof(int)));
    } catch (...) { dsr_sat_destroy(s); f->sat = nullptr; delete f; throw; }
    *out = f;
  });
}
void dsr_fsat_destroy(dsr_fsat* f) { if (f) { dsr_sat_destroy(f->sat); delete f; } }
dsr_sat* dsr_fsat_sat(dsr_fsat* f) { return f ? f->sat : nullptr; }
int dsr_fsat_fast_blocks(const dsr_fsat* f) { return f ? f->fastBlocks : 0; }

dsr_status dsr_fsat_set_stats(dsr_fsat* f, int s, dsr_train* t)
{
  return guard([&] {
    need(f); if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*f, s); pass(dsr_sat_set_stats(f->sat, s, t)); fsat_take_counts(*f, s, *t); f->full[s] = 1;
  });
}

dsr_status dsr_fsat_set_counts(dsr_fsat* f, int s, dsr_train* t)
{ return guard([&] { need(f); if (!t) throw Error(DSR_E_PARAMETER, "null argument"); check_slot(*f, s); take_counts(*f, s, *t); f->full[s] = 0; }); }

dsr_status dsr_fsat_set_stats_arrays(dsr_fsat* f, int s, const double* count, const double* denCount, const double* sumO, const double* sumOsq)
{
  return guard([&] {
    need(f); if (!count || !denCount || (!sumO) != (!sumOsq)) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*f, s);
    if (sumO) {
      std::vector<double> c(f->G); for (int g = 0; g < f->G; g++) c[g] = count[g] - denCount[g];
      pass(dsr_sat_set_stats_arrays(f->sat, s, c.data(), sumO, sumOsq));
    }
    put_counts(*f, s, count, denCount); f->full[s] = sumO != nullptr;
  });
}

dsr_status dsr_fsat_set_tree(dsr_fsat* f, int s, const dsr_param_tree* t) { return guard([&] { need(f); pass(dsr_sat_set_tree(f->sat, s, t)); }); }
dsr_status dsr_fsat_set_apt(dsr_fsat* f, int s, dsr_apt* apt, int aptSlot) { return guard([&] { need(f); pass(dsr_sat_set_apt(f->sat, s, apt, aptSlot)); }); }
dsr_status dsr_fsat_set_transform(dsr_fsat* f, int s, unsigned rc, int kind, int nBlocks, const double* A, const double* b)
{ return guard([&] { need(f); pass(dsr_sat_set_transform(f->sat, s, rc, kind, nBlocks, A, b)); }); }

dsr_status dsr_fsat_clear_slot(dsr_fsat* f, int s)
{
  return guard([&] {
    need(f); pass(dsr_sat_clear_slot(f->sat, s));
    const size_t G = f->G;
    DSR_HIP(hipMemset(f->d_num.p + s * G, 0, G * sizeof(double))); DSR_HIP(hipMemset(f->d_den.p + s * G, 0, G * sizeof(double))); f->full[s] = 0;
  });
}

dsr_status dsr_fsat_set_reg_classes_to_one(dsr_fsat* f) { return guard([&] { need(f); set_reg_classes_to_one(*f); }); }
dsr_status dsr_fsat_norm(dsr_fsat* f, int nSlots, void* stream) { return guard([&] { need(f); norm(*f, nSlots, (hipStream_t) stream); }); }
dsr_status dsr_fsat_zero_fast(dsr_fsat* f) { return guard([&] { need(f); f->fastBlocks = 0; }); }

dsr_status dsr_fsat_save_fast(dsr_fsat* f, const char* fileName)
{ return guard([&] { need(f); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); save_fast(*f, fileName); }); }

dsr_status dsr_fsat_load_fast(dsr_fsat* f, const char* fileName, int nParts, int part)
{ return guard([&] { need(f); if (!fileName) throw Error(DSR_E_PARAMETER, "null argument"); load_fast(*f, fileName, nParts, part); }); }

dsr_status dsr_fsat_get_fast(dsr_fsat* f, double* count, double* denCount, double* fastMean, double* fastVar, double* scalar)
{
  return guard([&] {
    need(f); FastHost a; pull_fast(*f, a);
    if (count) std::copy(a.count.begin(), a.count.end(), count); if (denCount) std::copy(a.den.begin(), a.den.end(), denCount);
    if (fastMean) std::copy(a.mean.begin(), a.mean.end(), fastMean); if (fastVar) std::copy(a.var.begin(), a.var.end(), fastVar);
    if (scalar) std::copy(a.scalar.begin(), a.scalar.end(), scalar);
  });
}

dsr_status dsr_fsat_set_fast(dsr_fsat* f, int nBlocks, const double* count, const double* denCount, const double* fastMean, const double* fastVar, const double* scalar)
{
  return guard([&] {
    need(f); if (!count || !denCount || !fastMean || !fastVar || !scalar) throw Error(DSR_E_PARAMETER, "null argument");
    check_blocks(*f, nBlocks);
    if (f->descBlocks && f->descBlocks != nBlocks) throw Error(DSR_E_DIMENSION, "description lengths of %d blocks for accumulators of %d", f->descBlocks, nBlocks);
    const size_t G = f->G, D = f->D;
    FastHost a; a.count.assign(count, count + G); a.den.assign(denCount, denCount + G); a.mean.assign(fastMean, fastMean + G * D);
    a.var.assign(fastVar, fastVar + G * D); a.scalar.assign(scalar, scalar + G * nBlocks);
    alloc_fast(*f, nBlocks); need_desc(*f, nBlocks); push_fast(*f, a);
  });
}

dsr_status dsr_fsat_add_fast(dsr_fsat* f) { return guard([&] { need(f); add_fast(*f); }); }
dsr_status dsr_fsat_accumulate(dsr_fsat* f, int nSlots, void* stream) { return guard([&] { need(f); accumulate(*f, nSlots, (hipStream_t) stream); }); }
dsr_status dsr_fsat_update(dsr_fsat* f, unsigned info[4], unsigned totals[2], double* aux) { return guard([&] { need(f); update(*f, info, totals, aux); }); }
dsr_status dsr_fsat_zero(dsr_fsat* f) { return guard([&] { need(f); pass(dsr_sat_zero(f->sat)); }); }

dsr_status dsr_fsat_desc_length(const dsr_fsat* f, unsigned* dl)
{ return guard([&] { need(f); if (!dl) throw Error(DSR_E_PARAMETER, "null argument"); *dl = desc_length(*f); }); }

int dsr_fsat_desc_blocks(const dsr_fsat* f) { return f ? f->descBlocks : 0; }

dsr_status dsr_fsat_get_desc_len(const dsr_fsat* f, uint16_t* descLen)
{
  return guard([&] {
    need(f); if (!descLen) throw Error(DSR_E_PARAMETER, "null argument");
    if (!f->descBlocks) throw Error(DSR_E_CONSISTENCY, "no description lengths: the block count is not known yet");
    std::copy(f->descLen.begin(), f->descLen.end(), descLen);
  });
}

dsr_status dsr_fsat_set_desc_len(dsr_fsat* f, int nBlocks, const uint16_t* descLen)
{
  return guard([&] {
    need(f); if (!descLen) throw Error(DSR_E_PARAMETER, "null argument");
    check_blocks(*f, nBlocks);
    if (f->descBlocks && f->descBlocks != nBlocks) throw Error(DSR_E_DIMENSION, "description lengths of %d blocks, the handle keeps %d", nBlocks, f->descBlocks);
    f->descBlocks = nBlocks; f->descLen.assign(descLen, descLen + (size_t) f->G * nBlocks);
  });
}

dsr_status dsr_fsat_estimate_files(dsr_fsat* f, const char* speakerList, const char* paramPrefix, const char* accuPrefix, double* ret)
{
  return guard([&] {
    need(f); if (!speakerList || !paramPrefix || !accuPrefix) throw Error(DSR_E_PARAMETER, "null argument");
    const double r = estimate_files(*f, speakerList, paramPrefix, accuPrefix);
    if (ret) *ret = r;
  });
}

dsr_status dsr_fsat_get_records(const dsr_fsat* f, int32_t* kept, int32_t* decision, double* auxOld, double* auxNew, int32_t* descLen)
{
  return guard([&] {
    need(f); pass(dsr_sat_get_records(f->sat, kept, decision, auxOld, auxNew));
    if (descLen) std::copy(f->recDesc.begin(), f->recDesc.end(), descLen);
  });
}

dsr_status dsr_fsat_kernel_ms(const dsr_fsat* f, float ms[3])
{ return guard([&] { need(f); if (!ms) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 3; i++) ms[i] = f->ms[i]; }); }

}  // extern "C"
