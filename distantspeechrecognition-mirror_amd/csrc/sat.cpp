// csrc/sat.cpp -- the host side of speaker-adaptive training: the handle, the slot tables of transforms, the speaker list, the updates and
// the file-driven estimate.
//
// Replaces SATMean::_checkBlocks / update's bookkeeping (asr/sat/sat.cc:54-110, 288-342, "sat"), SATVariance::update / fixup (sat:731-756),
// SATBase::MeanAcc::update and VarianceAcc::update (sat:1010-1023, 1233-1244), SATBase::SATBase / estimate (sat:1763-1780, 1802-1839),
// TransformerTreeList::getTree (sat:1884-1896), TransformerTree::transformer (asr/adapt/transform.cc:2165-2173, "tr"), BaseTree::_setNodeTypes
// (tr:2082-2100), the TransformMatrix of MLLRTransformer (tr:1746-1768) and of APTTransformerBase (tr:1339-1363), and SpeakerList
// (tr:1989-1998).  The arithmetic over the statistics is in sat_kernels.hip.  Compiled with -ffp-contract=off.
#include "common.h"
#include "adapt.h"
#include "apt.h"
#include "train.h"
#include "sat.h"
#include <algorithm>
#include <cmath>

namespace dsr {

std::vector<std::string> read_speaker_list(const char* fileName)
{
  if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
  FILE* fp = fopen(fileName, "r"); if (!fp) throw Error(DSR_E_IO, "Could not open file %s.", fileName);
  std::vector<std::string> list; char buffer[128];        // MaxListLength: a longer line arrives in pieces, as there
  while (fgets(buffer, sizeof buffer, fp)) {
    const char* tok = strtok(buffer, "\n");
    if (!tok) { fclose(fp); throw Error(DSR_E_PARSE, "empty line %d in speaker list %s", (int) list.size() + 1, fileName); }     // a null String there
    list.push_back(tok);
  }
  fclose(fp);
  return list;
}

void sat_part_gaussians(const SatHandle& h, int& g0, int& g1)
{
  int k0, k1; part_range(h.g->K, h.nParts, h.part, k0, k1);
  g0 = h.g->off[k0]; g1 = h.g->off[k1];
}

namespace {

void check_slot(const SatHandle& h, int s) { if (s < 0 || s >= h.S) throw Error(DSR_E_INDEX, "slot %d of %d", s, h.S); }
void check_gauss(const SatHandle& h, int g) { if (g < 0 || g >= h.G) throw Error(DSR_E_INDEX, "Gaussian %d of %d", g, h.G); }

void check_model(const SatHandle& h)
{
  if (h.g->G != h.G || h.g->D != h.D || h.tr->G != h.G) throw Error(DSR_E_DIMENSION, "the model changed shape under the SAT handle (%d x %d, now %d x %d)", h.G, h.D, h.g->G, h.g->D);
}

void part_gaussians(const SatHandle& h, int& g0, int& g1) { sat_part_gaussians(h, g0, g1); }

void put_xform(SatHandle& h, int s, unsigned rc, SatXform& x)
{
  if (rc == 0) throw Error(DSR_E_INDEX, "Regression class index must be >= 1");                      // BaseTree::_setNode, tr:2021-2022
  if (x.kind != kSatMLLR && x.kind != kSatAPT) throw Error(DSR_E_PARAMETER, "transform kind %d: 1 (MLLR) or 2 (APT)", x.kind);
  if (x.nBlocks < 1 || h.D % x.nBlocks != 0)
    throw Error(DSR_E_DIMENSION, "Transformed feature length %d is not compatible with %d blocks.", h.D, x.nBlocks);     // sat:63-65
  if (h.D / x.nBlocks > kSatMaxBlock) throw Error(DSR_E_DIMENSION, "block length %d: SAT is built for blocks of at most %d", h.D / x.nBlocks, kSatMaxBlock);
  h.slot[s][rc].A.swap(x.A); SatXform& d = h.slot[s][rc]; d.b.swap(x.b); d.kind = x.kind; d.nBlocks = x.nBlocks; d.bSize = x.bSize;
}

void set_tree(SatHandle& h, int s, const ParamTree& t)
{
  std::map<unsigned, SatXform> keep; keep.swap(h.slot[s]);
  try {
    for (std::map<unsigned, MLLRParam>::const_iterator it = t.map.begin(); it != t.map.end(); ++it) {  // TransformerTree(cb, parmFile), tr:2125-2135
      const MLLRParam& p = it->second;
      if (p.size != h.D) throw Error(DSR_E_DIMENSION, "Sizes (%d vs. %d) do not match.", p.size, h.D);                       // tr:1757-1758
      if ((int) p.bias.size() != h.D) throw Error(DSR_E_DIMENSION, "Feature lengths (%d vs. %d) do not match.", (int) p.bias.size(), h.D);
      SatXform x; x.kind = kSatMLLR; x.nBlocks = 1; x.bSize = h.D; x.A = p.matrix; x.b = p.bias;
      put_xform(h, s, it->first, x);
    }
  } catch (...) { h.slot[s].swap(keep); throw; }
}

// the transform matrix of every class of an APT store, made by `make` (the existing matrix kernel), as nSub equal blocks (tr:1339-1363)
template <class Make> void set_apt_store(SatHandle& h, int s, const AptParams& store, int L, int nSub, Make make)
{
  if (L * nSub != h.D) throw Error(DSR_E_DIMENSION, "%d sub-features of %d for a model of dimN = %d", nSub, L, h.D);
  std::map<unsigned, SatXform> keep; keep.swap(h.slot[s]);
  try {
    for (std::map<unsigned, AptParam>::const_iterator it = store.map.begin(); it != store.map.end(); ++it) {
      const AptParam& p = it->second; const int nb = (int) p.bias.size();
      if (nb != 0 && nb != L && nb != h.D) throw Error(DSR_E_CONSISTENCY, "Bias size %d is incompatible with feature length %d.", nb, L);
      std::vector<double> A((size_t) L * L); make(it->first, p, A.data());
      SatXform x; x.kind = kSatAPT; x.nBlocks = nSub; x.bSize = nb; x.b.assign(h.D, 0.0);
      for (int i = 0; i < nb; i++) x.b[i] = (double) p.bias[i];
      for (int k = 0; k < nSub; k++) x.A.insert(x.A.end(), A.begin(), A.end());
      put_xform(h, s, it->first, x);
    }
  } catch (...) { h.slot[s].swap(keep); throw; }
}

void sat_zero(SatHandle& h)
{
  DSR_HIP(hipDeviceSynchronize());
  if (h.nBlocks) DSR_HIP(hipMemset(h.d_macc.p, 0, (size_t) h.G * h.nBlocks * h.stride() * sizeof(double)));
  DSR_HIP(hipMemset(h.d_mocc.p, 0, (size_t) h.G * sizeof(double)));
  DSR_HIP(hipMemset(h.d_vvec.p, 0, (size_t) h.G * h.D * sizeof(double)));
  DSR_HIP(hipMemset(h.d_vocc.p, 0, (size_t) h.G * sizeof(double)));                                   // the blocks stay allocated: d_has is kept (sat:240-253)
}

}  // namespace

void sat_tables(SatHandle& h, int nSlots, int g0, int g1, SatCall& c, std::vector<int>& gidx, std::vector<int>& tile, hipStream_t st)
{
  const GmmModel& m = *h.g; const int D = h.D, G = h.G;
  std::vector<unsigned> classes;
  for (int g = g0; g < g1; g++) {
    const unsigned rc = m.regClass.empty() ? 0u : m.regClass[g];
    if (rc == 0) throw Error(DSR_E_INDEX, "Regression class index must be >= 1");                     // BaseTree::node, tr:2053-2054
    classes.push_back(rc);
  }
  std::sort(classes.begin(), classes.end()); classes.erase(std::unique(classes.begin(), classes.end()), classes.end());
  const int NC = (int) classes.size();
  int nB = 0;
  for (int s = 0; s < nSlots; s++)
    for (int k = 0; k < NC; k++) {                        // TransformerTree::transformer, tr:2165-2173
      const std::map<unsigned, SatXform>& t = h.slot[s]; const unsigned rc = classes[k];
      std::map<unsigned, SatXform>::const_iterator it = t.find(rc);
      if (it == t.end()) throw Error(DSR_E_KEY, "Could not find node %d.", rc);
      for (std::map<unsigned, SatXform>::const_iterator o = t.upper_bound(rc); o != t.end(); ++o)
        if (isAncestor(rc, o->first)) throw Error(DSR_E_CONSISTENCY, "Node for regression class %d is not a leaf", rc);
      if (nB == 0) nB = it->second.nBlocks;
      else if (nB != it->second.nBlocks) throw Error(DSR_E_DIMENSION, "Block sizes (%d vs %d) are not equivalent.", it->second.nBlocks, nB);
    }
  const int bl = D / nB;
  // the tables [slot][class]
  std::vector<double> A((size_t) nSlots * NC * D * bl), b((size_t) nSlots * NC * D); std::vector<int> kind((size_t) nSlots * NC), bsz((size_t) nSlots * NC);
  for (int s = 0; s < nSlots; s++)
    for (int k = 0; k < NC; k++) {
      const SatXform& x = h.slot[s].find(classes[k])->second; const size_t tab = (size_t) s * NC + k;
      std::copy(x.A.begin(), x.A.end(), A.begin() + tab * D * bl); std::copy(x.b.begin(), x.b.end(), b.begin() + tab * D);
      kind[tab] = x.kind; bsz[tab] = x.bSize;
    }
  // the Gaussians sorted by class (stable), cut into tiles that do not cross a class
  std::vector<int> cls(G, 0); std::vector<std::vector<int>> of(NC); gidx.clear(); tile.clear();
  for (int g = g0; g < g1; g++) { cls[g] = (int) (std::lower_bound(classes.begin(), classes.end(), (unsigned) m.regClass[g]) - classes.begin()); of[cls[g]].push_back(g); }
  for (int k = 0; k < NC; k++)
    for (size_t i0 = 0; i0 < of[k].size(); i0 += kSatTileG) {
      tile.push_back(k); tile.push_back((int) gidx.size()); tile.push_back((int) std::min((size_t) kSatTileG, of[k].size() - i0));
      gidx.insert(gidx.end(), of[k].begin() + i0, of[k].begin() + i0 + tile.back());
    }
  c.nSlots = nSlots; c.NC = NC; c.nB = nB; c.bl = bl; c.g0 = g0; c.g1 = g1; c.nTiles = (int) (tile.size() / 3); c.PZ = c.NCp = 0;
  h.d_A.upload(A, st); h.d_b.upload(b, st); h.d_kind.upload(kind, st); h.d_bsz.upload(bsz, st); h.d_cls.upload(cls, st);
}

void sat_accumulate(SatHandle& h, int what, bool matOnly, int nSlots, hipStream_t st)
{
  if (what != kSatMean && what != kSatVariance) throw Error(DSR_E_PARAMETER, "accumulate %d: 1 (means) or 2 (variances)", what);
  if (nSlots < 1 || nSlots > h.S) throw Error(DSR_E_INDEX, "%d slots of %d", nSlots, h.S);
  check_model(h);
  const GmmModel& m = *h.g; const int D = h.D, G = h.G;
  int g0, g1; sat_part_gaussians(h, g0, g1);
  if (g0 == g1) return;
  SatCall c; std::vector<int> gidx, tile;
  sat_tables(h, nSlots, g0, g1, c, gidx, tile, st);
  const int nB = c.nB, bl = c.bl;
  if (what == kSatMean && h.nBlocks && nB != h.nBlocks) throw Error(DSR_E_DIMENSION, "Block sizes (%d vs %d) are not equivalent.", nB, h.nBlocks);   // sat:57-59
  const int P = bl * (bl + 1) / 2; c.PZ = (P + 15) & ~15; c.NCp = matOnly ? c.PZ : (c.PZ + bl + 15) & ~15;
  if (what == kSatMean) {
    if (!h.nBlocks) {                                     // SATMean::_checkBlocks, sat:63-81
      h.d_macc.reserve((size_t) G * nB * ((size_t) bl * bl + bl + 1));
      DSR_HIP(hipMemsetAsync(h.d_macc.p, 0, (size_t) G * nB * ((size_t) bl * bl + bl + 1) * sizeof(double), st));
      h.nBlocks = nB; h.bl = bl;
    }
    std::vector<int> pq(c.NCp, -1);
    { int col = 0; for (int p = 0; p < bl; p++) for (int q = p; q < bl; q++) pq[col++] = p | (q << 16); if (!matOnly) for (int n = 0; n < bl; n++) pq[c.PZ + n] = n; }
    h.d_pq.upload(pq, st); h.d_gidx.upload(gidx, st); h.d_tile.upload(tile, st); h.d_ivar.upload(m.ivar, st);
    sat_mean_acc(h, c, matOnly, st);
  } else {
    h.d_mean.upload(m.mean, st);
    if (h.keepTrn) { h.d_trn.reserve((size_t) nSlots * G * D); DSR_HIP(hipMemsetAsync(h.d_trn.p, 0, (size_t) nSlots * G * D * sizeof(float), st)); h.trnSlots = nSlots; }
    sat_var_acc(h, c, st);
  }
  DSR_HIP(hipStreamSynchronize(st));
}

namespace {

void update_means(SatHandle& h, unsigned info[4], unsigned totals[2], double* aux)
{
  check_model(h);
  GmmModel& m = *h.g; const int D = h.D, G = h.G, nB = h.nBlocks, bl = h.bl;
  int g0, g1; part_gaussians(h, g0, g1);
  DSR_HIP(hipDeviceSynchronize());
  std::vector<double> occ(G); std::vector<int> has(G);
  DSR_HIP(hipMemcpy(occ.data(), h.d_mocc.p, G * sizeof(double), hipMemcpyDeviceToHost));
  DSR_HIP(hipMemcpy(has.data(), h.d_has.p, G * sizeof(int), hipMemcpyDeviceToHost));
  unsigned inf[4] = {0, 0, 0, 0}, tot[2] = {0, 0}; double auxSum = 0.0;
  h.rec.assign((size_t) G * std::max(nB, 1), SatRecord{0, kSatLeft, 0.0, 0.0}); h.status.assign(G, 0);
  std::vector<int> solve, zeroed;
  for (int g = g0; g < g1; g++) {                         // MeanAcc::update, sat:1010-1023
    tot[0]++;
    if (occ[g] < h.threshold) continue;
    tot[1]++;
    if (!has[g] || !nB) continue;                         // no blocks: SATMean::update walks none
    if (occ[g] == 0.0) zeroed.push_back(g); else solve.push_back(g);                                  // sat:292-300
  }
  std::vector<float> newMean = m.mean; h.sol.assign((size_t) G * D, 0.0);
  if (!solve.empty()) {
    std::vector<SatRecord> rec((size_t) G * nB);
    h.d_solve.upload(solve); h.d_mean.upload(m.mean); h.d_newMean.upload(m.mean); h.d_rec.reserve(rec.size());
    h.d_sol.reserve(h.sol.size()); DSR_HIP(hipMemset(h.d_sol.p, 0, h.sol.size() * sizeof(double)));
    sat_solve(h, (int) solve.size(), nullptr);
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(newMean.data(), h.d_newMean.p, newMean.size() * sizeof(float), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(rec.data(), h.d_rec.p, rec.size() * sizeof(SatRecord), hipMemcpyDeviceToHost));
    DSR_HIP(hipMemcpy(h.sol.data(), h.d_sol.p, h.sol.size() * sizeof(double), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < solve.size(); i++) for (int nb = 0; nb < nB; nb++) h.rec[(size_t) solve[i] * nB + nb] = rec[(size_t) solve[i] * nB + nb];
  }
  for (size_t i = 0; i < zeroed.size(); i++) {
    for (int d = 0; d < D; d++) m.mean[(size_t) zeroed[i] * D + d] = 0.0f;
    for (int nb = 0; nb < nB; nb++) h.rec[(size_t) zeroed[i] * nB + nb].decision = kSatZeroed;
  }
  int nFlag = 0, firstFlag = -1, nNaN = 0, firstNaN = -1;
  for (size_t i = 0; i < solve.size(); i++) {             // model order
    const int g = solve[i]; const SatRecord* r = &h.rec[(size_t) g * nB];
    for (int nb = 0; nb < nB; nb++) {
      if (r[nb].decision == kSatFlagged && !h.status[g]) { h.status[g] = DSR_E_CONSISTENCY; if (!nFlag++) firstFlag = g; }
      if (r[nb].decision == kSatNaN && !h.status[g]) { h.status[g] = DSR_E_NUMERIC; if (!nNaN++) firstNaN = g; }
    }
    if (h.status[g]) continue;                            // its mean stays
    for (int nb = 0; nb < nB; nb++) {                     // UpdateInfo, sat:304, 324, 339, 267, 273
      if (r[nb].decision == kSatKeptOld) { auxSum += r[nb].auxOld; inf[0]++; continue; }
      std::copy(newMean.begin() + (size_t) g * D + nb * bl, newMean.begin() + (size_t) g * D + (nb + 1) * bl, m.mean.begin() + (size_t) g * D + nb * bl);
      auxSum += r[nb].auxNew; inf[0]++; inf[1]++; inf[2] += bl; inf[3] += r[nb].kept;
    }
  }
  gmm_finish(m);
  if (info) std::copy(inf, inf + 4, info); if (totals) std::copy(tot, tot + 2, totals); if (aux) *aux = auxSum;
  if (nFlag) throw Error(DSR_E_CONSISTENCY, "SAT statistics of %d Gaussian(s), the first %d, are not finite or their eigen-decomposition did not converge", nFlag, firstFlag);
  if (nNaN) throw Error(DSR_E_NUMERIC, "Degenerate value in a mean component of %d Gaussian(s), the first %d", nNaN, firstNaN);
}

void update_variances(SatHandle& h, unsigned totals[2])
{
  check_model(h);
  GmmModel& m = *h.g; const int D = h.D, G = h.G;
  int g0, g1; part_gaussians(h, g0, g1);
  DSR_HIP(hipDeviceSynchronize());
  std::vector<double> occ(G), vec((size_t) G * D);
  DSR_HIP(hipMemcpy(occ.data(), h.d_vocc.p, G * sizeof(double), hipMemcpyDeviceToHost));
  DSR_HIP(hipMemcpy(vec.data(), h.d_vvec.p, vec.size() * sizeof(double), hipMemcpyDeviceToHost));
  unsigned tot[2] = {0, 0}; int nNaN = 0, firstNaN = -1;
  h.status.assign(G, 0);
  for (int g = g0; g < g1; g++) {                         // VarianceAcc::update, sat:1233-1244
    float* var = &m.ivar[(size_t) g * D];
    tot[0]++;
    if (occ[g] < h.threshold) { for (int d = 0; d < D; d++) var[d] = (float) (1.0 / var[d]); continue; }    // fixup, sat:753-756
    tot[1]++;
    if (occ[g] == 0.0) { for (int d = 0; d < D; d++) var[d] = 0.0f; continue; }                              // sat:735-739
    bool nan = false;
    for (int d = 0; d < D; d++) if (std::isnan(vec[(size_t) g * D + d] / occ[g])) nan = true;
    if (nan) { h.status[g] = DSR_E_NUMERIC; if (!nNaN++) firstNaN = g; continue; }
    for (int d = 0; d < D; d++) var[d] = (float) (vec[(size_t) g * D + d] / occ[g]);                         // sat:741-748
  }
  gmm_finish(m);
  if (totals) std::copy(tot, tot + 2, totals);
  if (nNaN) throw Error(DSR_E_NUMERIC, "updateSATVar: degenerate variance value in %d Gaussian(s), the first %d", nNaN, firstNaN);
}

void sat_update(SatHandle& h, int what, unsigned info[4], unsigned totals[2], double* aux)
{
  if (what != kSatMean && what != kSatVariance) throw Error(DSR_E_PARAMETER, "update %d: 1 (means) or 2 (variances)", what);
  if (what == kSatMean) update_means(h, info, totals, aux);
  else { if (info) std::fill(info, info + 4, 0u); if (aux) *aux = 0.0; update_variances(h, totals); }
}

void take_into_slot(SatHandle& h, int s, dsr_train& t)
{
  take_stats_sq(t, h.G, h.D, h.d_c.p + (size_t) s * h.G, h.d_sumO.p + (size_t) s * h.G * h.D, h.d_sumOsq.p + (size_t) s * h.G * h.D);
}

// the parameter file of one speaker into a slot: an MLLR tree, or RAPT / SLAPT parameters through the APT matrix kernel
void read_params(SatHandle& h, int s, const std::string& fileName) { sat_read_params(h, s, fileName); }

}  // namespace

void sat_read_params(SatHandle& h, int s, const std::string& fileName)
{
  { FILE* fp = fopen(fileName.c_str(), "r"); if (!fp) throw Error(DSR_E_IO, "Could not open file %s.", fileName.c_str()); fclose(fp); }
  ParamTree t; bool mllr = true;
  try { t.read(fileName.c_str()); } catch (const Error& e) { if (e.code != DSR_E_TYPE) throw; mllr = false; }
  if (mllr) { set_tree(h, s, t); return; }
  AptParams store; store.read(fileName.c_str());
  const int L = h.D / h.aptSub;
  set_apt_store(h, s, store, L, h.aptSub, [&](unsigned, const AptParam& p, double* A) {
    const dsr_status st = dsr_apt_transform_rows(store.type, L, h.aptSub, (int) p.conf.size(), p.conf.data(), (int) p.bias.size(), p.bias.data(), nullptr, 0, A, nullptr);
    if (st) throw Error(st, "%s", dsr_last_error());
  });
}

namespace {

double estimate_files(SatHandle& h, int what, const char* speakerList, const char* paramPrefix, const char* accuPrefix)
{
  if (what != kSatMean && what != kSatVariance) throw Error(DSR_E_PARAMETER, "estimate %d: 1 (means) or 2 (variances)", what);
  const std::vector<std::string> list = read_speaker_list(speakerList);
  int totalT = 0; double totalPr = 0.0;                   // LogLhoodThreshhold descLength() = 0, sat:1806
  dsr_status st = dsr_train_zero(h.tr, 1, h.nParts, h.part); if (st) throw Error(st, "%s", dsr_last_error());
  int filled = 0;
  for (size_t i = 0; i < list.size(); i++) {              // sat:1816-1834; S speakers a batch, in list order
    float pr = 0.f; unsigned tt = 0;
    const std::string accu = std::string(accuPrefix) + list[i] + ".cbs.accu";
    st = dsr_train_load_codebook_accus(h.tr, accu.c_str(), &pr, &tt, 1.0f, h.nParts, h.part); if (st) throw Error(st, "%s", dsr_last_error());
    totalPr += (double) pr; totalT += (int) tt;
    read_params(h, filled, std::string(paramPrefix) + list[i]);                                       // no separator, sat:1890
    take_into_slot(h, filled, *h.tr);
    st = dsr_train_zero(h.tr, 1, h.nParts, h.part); if (st) throw Error(st, "%s", dsr_last_error());
    if (++filled == h.S || i + 1 == list.size()) { sat_accumulate(h, what, false, filled, nullptr); filled = 0; }
  }
  sat_update(h, what, nullptr, nullptr, nullptr);
  return totalPr / totalT;
}

}  // namespace
}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_sat_check(int meanLen, int featLen, double lhoodThreshold, int accKind)
{
  return guard([&] {
    if (accKind != 0 && accKind != 1)
      throw Error(DSR_E_PARAMETER, "SAT accumulator kind %d: MeanAcc (0) and VarianceAcc (1) are implemented; FastAcc, RegClassAcc and the MMI kinds are not", accKind);
    if (lhoodThreshold != 0.0) throw Error(DSR_E_PARAMETER, "likelihood threshold %g: MDLSATMean is not implemented", lhoodThreshold);
    if (meanLen != 0 && meanLen != featLen) throw Error(DSR_E_DIMENSION, "mean length %d for features of %d: extended means are not implemented", meanLen, featLen);
  });
}

dsr_status dsr_speaker_list_read(const char* fileName, char* labels, int cap, int* n, int* bytes)
{
  return guard([&] {
    if (!n || !bytes) throw Error(DSR_E_PARAMETER, "null argument");
    const std::vector<std::string> l = read_speaker_list(fileName); std::string all;
    for (size_t i = 0; i < l.size(); i++) { all += l[i]; all += '\n'; }
    *n = (int) l.size(); *bytes = (int) all.size();
    if (labels && cap >= (int) all.size()) memcpy(labels, all.data(), all.size());
  });
}

dsr_status dsr_sat_create(dsr_train* t, int S, double massThreshold, int nParts, int part, dsr_sat** out)
{
  return guard([&] {
    if (!t || !out) throw Error(DSR_E_PARAMETER, "null argument");
    if (S < 1 || S > 65535) throw Error(DSR_E_PARAMETER, "%d speaker slots", S);
    int k0, k1; part_range(t->g->K, nParts, part, k0, k1);
    require_device();
    dsr_sat* h = new dsr_sat();
    try {
      h->tr = t; h->g = t->g; h->S = S; h->D = t->D; h->G = t->G; h->nParts = nParts; h->part = part;
      h->threshold = massThreshold == 0.0 ? 10.0 : massThreshold;                                     // sat:1768
      h->slot.resize(S); h->status.assign(h->G, 0);
      const size_t G = h->G, D = h->D;
      h->d_c.reserve(S * G); h->d_sumO.reserve(S * G * D); h->d_sumOsq.reserve(S * G * D);
      DSR_HIP(hipMemset(h->d_c.p, 0, S * G * sizeof(double))); DSR_HIP(hipMemset(h->d_sumO.p, 0, S * G * D * sizeof(double)));
      DSR_HIP(hipMemset(h->d_sumOsq.p, 0, S * G * D * sizeof(double)));
      h->d_mocc.reserve(G); h->d_vocc.reserve(G); h->d_vvec.reserve(G * D); h->d_has.reserve(G);
      DSR_HIP(hipMemset(h->d_has.p, 0, G * sizeof(int)));
      sat_zero(*h);
    } catch (...) { delete h; throw; }
    *out = h;
  });
}
void dsr_sat_destroy(dsr_sat* h) { delete h; }
int dsr_sat_num_slots(const dsr_sat* h) { return h ? h->S : 0; }
int dsr_sat_num_blocks(const dsr_sat* h) { return h ? h->nBlocks : 0; }

dsr_status dsr_sat_set_apt_sub_features(dsr_sat* h, int nSubFeat)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    if (nSubFeat < 1 || nSubFeat > 3 || h->D % nSubFeat) throw Error(DSR_E_DIMENSION, "Mean length %d is inconsistent with %d sub-features", h->D, nSubFeat);   // sat:1789-1791
    h->aptSub = nSubFeat;
  });
}

dsr_status dsr_sat_zero(dsr_sat* h) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); sat_zero(*h); }); }

dsr_status dsr_sat_set_stats(dsr_sat* h, int s, dsr_train* t)
{ return guard([&] { if (!h || !t) throw Error(DSR_E_PARAMETER, "null argument"); check_slot(*h, s); take_into_slot(*h, s, *t); }); }

dsr_status dsr_sat_set_stats_arrays(dsr_sat* h, int s, const double* c, const double* sumO, const double* sumOsq)
{
  return guard([&] {
    if (!h || !c || !sumO || !sumOsq) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    const size_t G = h->G, D = h->D;
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(h->d_c.p + s * G, c, G * sizeof(double), hipMemcpyHostToDevice));
    DSR_HIP(hipMemcpy(h->d_sumO.p + s * G * D, sumO, G * D * sizeof(double), hipMemcpyHostToDevice));
    DSR_HIP(hipMemcpy(h->d_sumOsq.p + s * G * D, sumOsq, G * D * sizeof(double), hipMemcpyHostToDevice));
  });
}

dsr_status dsr_sat_set_tree(dsr_sat* h, int s, const dsr_param_tree* t)
{ return guard([&] { if (!h || !t) throw Error(DSR_E_PARAMETER, "null argument"); check_slot(*h, s); set_tree(*h, s, *t); }); }

dsr_status dsr_sat_set_apt(dsr_sat* h, int s, dsr_apt* apt, int aptSlot)
{
  return guard([&] {
    if (!h || !apt) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    if (aptSlot < 0 || aptSlot >= apt->S) throw Error(DSR_E_INDEX, "speaker %d of %d", aptSlot, apt->S);
    if (apt->D != h->D) throw Error(DSR_E_DIMENSION, "transforms of dimN = %d for a model of %d", apt->D, h->D);
    set_apt_store(*h, s, apt->store[aptSlot], apt->L, apt->nSub, [&](unsigned rc, const AptParam&, double* A) {
      const dsr_status st = dsr_apt_get_matrix(apt, aptSlot, rc, A); if (st) throw Error(st, "%s", dsr_last_error());
    });
  });
}

dsr_status dsr_sat_set_transform(dsr_sat* h, int s, unsigned rc, int kind, int nBlocks, const double* A, const double* b)
{
  return guard([&] {
    if (!h || !A) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    if (nBlocks < 1 || h->D % nBlocks != 0) throw Error(DSR_E_DIMENSION, "Transformed feature length %d is not compatible with %d blocks.", h->D, nBlocks);
    const int bl = h->D / nBlocks;
    SatXform x; x.kind = kind; x.nBlocks = nBlocks; x.bSize = b ? h->D : 0; x.A.assign(A, A + (size_t) nBlocks * bl * bl);
    if (b) x.b.assign(b, b + h->D); else x.b.assign(h->D, 0.0);
    put_xform(*h, s, rc, x);
  });
}

dsr_status dsr_sat_get_transform(const dsr_sat* h, int s, unsigned rc, int* kind, int* nBlocks, int* bSize, double* A, double* b)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s);
    std::map<unsigned, SatXform>::const_iterator it = h->slot[s].find(rc);
    if (it == h->slot[s].end()) throw Error(DSR_E_KEY, "Could not find node %d.", rc);
    const SatXform& x = it->second;
    if (kind) *kind = x.kind; if (nBlocks) *nBlocks = x.nBlocks; if (bSize) *bSize = x.bSize;
    if (A) std::copy(x.A.begin(), x.A.end(), A); if (b) std::copy(x.b.begin(), x.b.end(), b);
  });
}

int dsr_sat_slot_classes(const dsr_sat* h, int s, unsigned* classes, int cap)
{
  if (!h || s < 0 || s >= h->S) return 0;
  int n = 0;
  for (std::map<unsigned, SatXform>::const_iterator it = h->slot[s].begin(); it != h->slot[s].end(); ++it, ++n) if (classes && n < cap) classes[n] = it->first;
  return n;
}

dsr_status dsr_sat_clear_slot(dsr_sat* h, int s)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_slot(*h, s); h->slot[s].clear();
    const size_t G = h->G, D = h->D;
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemset(h->d_c.p + s * G, 0, G * sizeof(double))); DSR_HIP(hipMemset(h->d_sumO.p + s * G * D, 0, G * D * sizeof(double)));
    DSR_HIP(hipMemset(h->d_sumOsq.p + s * G * D, 0, G * D * sizeof(double)));
  });
}

dsr_status dsr_sat_accumulate(dsr_sat* h, int what, int nSlots, void* stream)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); sat_accumulate(*h, what, false, nSlots, (hipStream_t) stream); }); }

dsr_status dsr_sat_update(dsr_sat* h, int what, unsigned info[4], unsigned totals[2], double* aux)
{ return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); sat_update(*h, what, info, totals, aux); }); }

dsr_status dsr_sat_estimate_files(dsr_sat* h, int what, const char* speakerList, const char* paramPrefix, const char* accuPrefix, double* ret)
{
  return guard([&] {
    if (!h || !speakerList || !paramPrefix || !accuPrefix) throw Error(DSR_E_PARAMETER, "null argument");
    const double r = estimate_files(*h, what, speakerList, paramPrefix, accuPrefix);
    if (ret) *ret = r;
  });
}

dsr_status dsr_sat_get_mean_accu(dsr_sat* h, int g, int block, double* mat, double* vec, double* scalar, double* occ)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_gauss(*h, g);
    if (!h->nBlocks) throw Error(DSR_E_CONSISTENCY, "no mean statistics: call dsr_sat_accumulate first");
    if (block < 0 || block >= h->nBlocks) throw Error(DSR_E_INDEX, "block %d of %d", block, h->nBlocks);
    const int bl = h->bl; std::vector<double> r(h->stride());
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(r.data(), h->d_macc.p + ((size_t) g * h->nBlocks + block) * h->stride(), r.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (mat) std::copy(r.begin(), r.begin() + bl * bl, mat); if (vec) std::copy(r.begin() + bl * bl, r.begin() + bl * bl + bl, vec);
    if (scalar) *scalar = r[bl * bl + bl];
    if (occ) DSR_HIP(hipMemcpy(occ, h->d_mocc.p + g, sizeof(double), hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_sat_get_mean_accus(dsr_sat* h, double* acc, double* occ, int32_t* has)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    if (!h->nBlocks) throw Error(DSR_E_CONSISTENCY, "no mean statistics: call dsr_sat_accumulate first");
    DSR_HIP(hipDeviceSynchronize());
    if (acc) DSR_HIP(hipMemcpy(acc, h->d_macc.p, (size_t) h->G * h->nBlocks * h->stride() * sizeof(double), hipMemcpyDeviceToHost));
    if (occ) DSR_HIP(hipMemcpy(occ, h->d_mocc.p, (size_t) h->G * sizeof(double), hipMemcpyDeviceToHost));
    if (has) DSR_HIP(hipMemcpy(has, h->d_has.p, (size_t) h->G * sizeof(int), hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_sat_get_var_accu(dsr_sat* h, int g, double* vec, double* occ)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    check_gauss(*h, g);
    DSR_HIP(hipDeviceSynchronize());
    if (vec) DSR_HIP(hipMemcpy(vec, h->d_vvec.p + (size_t) g * h->D, h->D * sizeof(double), hipMemcpyDeviceToHost));
    if (occ) DSR_HIP(hipMemcpy(occ, h->d_vocc.p + g, sizeof(double), hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_sat_get_var_accus(dsr_sat* h, double* vec, double* occ)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    DSR_HIP(hipDeviceSynchronize());
    if (vec) DSR_HIP(hipMemcpy(vec, h->d_vvec.p, (size_t) h->G * h->D * sizeof(double), hipMemcpyDeviceToHost));
    if (occ) DSR_HIP(hipMemcpy(occ, h->d_vocc.p, (size_t) h->G * sizeof(double), hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_sat_keep_transformed(dsr_sat* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->keepTrn = on != 0; }); }

dsr_status dsr_sat_get_transformed(dsr_sat* h, int s, float* means)
{
  return guard([&] {
    if (!h || !means) throw Error(DSR_E_PARAMETER, "null argument");
    if (s < 0 || s >= h->trnSlots) throw Error(DSR_E_INDEX, "slot %d of the %d kept by the last variance accumulation", s, h->trnSlots);
    DSR_HIP(hipDeviceSynchronize());
    DSR_HIP(hipMemcpy(means, h->d_trn.p + (size_t) s * h->G * h->D, (size_t) h->G * h->D * sizeof(float), hipMemcpyDeviceToHost));
  });
}

dsr_status dsr_sat_get_records(const dsr_sat* h, int32_t* kept, int32_t* decision, double* auxOld, double* auxNew)
{
  return guard([&] {
    if (!h) throw Error(DSR_E_PARAMETER, "null argument");
    for (size_t i = 0; i < h->rec.size(); i++) {
      if (kept) kept[i] = h->rec[i].kept; if (decision) decision[i] = h->rec[i].decision;
      if (auxOld) auxOld[i] = h->rec[i].auxOld; if (auxNew) auxNew[i] = h->rec[i].auxNew;
    }
  });
}

dsr_status dsr_sat_get_solution(const dsr_sat* h, double* means)
{
  return guard([&] {
    if (!h || !means) throw Error(DSR_E_PARAMETER, "null argument");
    if (h->sol.empty()) throw Error(DSR_E_CONSISTENCY, "no solution: call dsr_sat_update first");
    std::copy(h->sol.begin(), h->sol.end(), means);
  });
}

int dsr_sat_gaussian_status(const dsr_sat* h, int g) { return (h && g >= 0 && g < h->G) ? h->status[g] : DSR_E_INDEX; }

dsr_status dsr_sat_set_timing(dsr_sat* h, int on) { return guard([&] { if (!h) throw Error(DSR_E_PARAMETER, "null argument"); h->timing = on != 0; }); }
dsr_status dsr_sat_kernel_ms(const dsr_sat* h, float ms[3])
{ return guard([&] { if (!h || !ms) throw Error(DSR_E_PARAMETER, "null argument"); for (int i = 0; i < 3; i++) ms[i] = h->ms[i]; }); }

}  // extern "C"
