// csrc/apt.cpp -- the host side of all-pass transform adaptation: RAPT / SLAPT parameters, their text files, and the line search.
//
// Replaces APTParamBase / RAPTParam / SLAPTParam (asr/adapt/transform.cc:410-551, "tr"), ParamTree::findAPT (tr:862-896), the APT branches of
// ParamBase::param / _readParams (tr:339-407), and EstimatorBase::bracket / brentsMethod (asr/train/estimateAdapt.cc:94-240, "eA") with the
// start points of BLTEstimatorAdapt::estimate (eA:1659-1665) and of the one-parameter branch of APTEstimatorBase::optimize (eA:821-830).
// The search is written against a function that replays the values it was given and stops at the first point it has no value for: the
// caller evaluates that point on the device -- for every (slot, node) of a round in one launch -- and runs the search again.  It is
// deterministic in those values, so every run visits the same points.  Compiled with -ffp-contract=off.
#include "common.h"
#include "adapt.h"
#include "apt.h"
#include <cmath>

namespace dsr {

AptParam& AptParams::findAPT(unsigned initRC, int typ, bool useAncestor)
{
  if (type == kAptUnspecified) type = typ;
  else if (type != typ) throw Error(DSR_E_CONSISTENCY, "Tree not instantiated with %s parameters.", typ == kAptRAPT ? "RAPT" : "SLAPT");
  if (initRC == 0) throw Error(DSR_E_INDEX, "Regression class index is zero");
  std::map<unsigned, AptParam>::iterator itr = map.find(initRC);
  if (itr != map.end()) return itr->second;
  if (!useAncestor) throw Error(DSR_E_INDEX, "Could not find parameters for regression class %d.", initRC);
  unsigned reg = initRC / 2;
  while (reg > 0 && (itr = map.find(reg)) == map.end()) reg /= 2;
  AptParam par = reg == 0 ? AptParam() : itr->second;
  par.regClass = initRC;
  return map.insert(std::make_pair(initRC, par)).first->second;
}

namespace {

struct File {
  FILE* fp;
  File(const char* name, const char* mode) : fp(fopen(name, mode)) { if (!fp) throw Error(DSR_E_IO, "Could not open file %s.", name); }
  ~File() { if (fp) fclose(fp); }
};

void getConf(FILE* fp, AptParam& par)                     // APTParamBase::_getParams tr:430-441
{
  int n = 0; if (fscanf(fp, "%d", &n) != 1 || n < 0) n = 0;
  par.conf.assign((size_t) n, 0.0);
  for (int i = 0; i < n; i++) { double v = 0.0; if (fscanf(fp, "%lf", &v) == 1) par.conf[i] = v; }
}

void readParams(FILE* fp, AptParam& par, int typ)         // ParamBase::_readParams tr:374-407 for _type() == RAPT or SLAPT
{
  Symbol sym;
  while ((sym = getSymbol(fp)) != SymEndClass) {
    switch (sym) {
    case SymAdaptType:
      if (getAdaptType(fp) + 1 != typ) throw Error(DSR_E_PARAMETER, "Attempted to read parameters of wrong type.");
      break;
    case SymRegClass:
      if (fscanf(fp, "%u", &par.regClass) != 1) { /* the reference does not look at the count */ }
      break;
    case SymRAPT:
      if (typ == kAptSLAPT) throw Error(DSR_E_PARAMETER, "Attempted to read SLAPT parameters.");
      getConf(fp, par); break;
    case SymSLAPT:
      if (typ == kAptRAPT) throw Error(DSR_E_PARAMETER, "Attempted to read RAPT parameters.");
      getConf(fp, par); break;
    case SymMLLR:                                         // only the RAPT type refuses it there (tr:397-400)
      if (typ == kAptRAPT) throw Error(DSR_E_PARAMETER, "Attempted to read RAPT parameters.");
      getConf(fp, par); break;
    case SymBias: {                                       // tr:288-299: a double read into a float
      int n = 0; if (fscanf(fp, "%d", &n) != 1 || n < 0) n = 0;
      par.bias.assign((size_t) n, 0.0f);
      for (int i = 0; i < n; i++) { double v = 0.0; if (fscanf(fp, "%lf", &v) == 1) par.bias[i] = (float) v; }
      break;
    }
    default:
      throw Error(DSR_E_PARAMETER, "Unexpected symbol %s in conformal parameter file.", kSymMap[sym]);
    }
  }
}

bool readParam(FILE* fp, AptParam& par, int& typ)         // ParamBase::param(FILE*) tr:339-363
{
  int c = getc(fp); if (c == EOF) return false;
  ungetc(c, fp);
  if (getSymbol(fp) != SymAdaptType) throw Error(DSR_E_TYPE, "Unable to determine adaptation type.");
  const int t = getAdaptType(fp) + 1;
  if (t != kAptRAPT && t != kAptSLAPT) throw Error(DSR_E_PARAMETER, "Attempted to read parameters of wrong type.");     // an MLLR block: dsr_param_tree reads those
  typ = t; par = AptParam(); readParams(fp, par, t);
  return true;
}

}  // namespace

void AptParams::read(const char* fileName)
{
  clear();
  if (!fileName || !*fileName) return;
  File f(fileName, "r");
  std::map<unsigned, AptParam> m; AptParam par; int t = kAptUnspecified, typ = kAptUnspecified;
  while (readParam(f.fp, par, t)) {
    m.insert(std::make_pair(par.regClass, par));          // map::insert: the first class of an index stays
    if (typ == kAptUnspecified) typ = t;
    else if (typ != t) throw Error(DSR_E_CONSISTENCY, "Incorrect adaptation type for regression class %d.", par.regClass);
  }
  if (typ == kAptUnspecified) throw Error(DSR_E_CONSISTENCY, "Unable to determine adaptation type.");
  map.swap(m); type = typ;
}

void AptParams::write(const char* fileName) const
{
  if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
  File f(fileName, "w");
  const bool rapt = type == kAptRAPT;
  for (std::map<unsigned, AptParam>::const_iterator it = map.begin(); it != map.end(); ++it) {        // ParamBase::write tr:365-372, index order
    const AptParam& p = it->second;
    fprintf(f.fp, "<AdaptType> %s\n", rapt ? "RAPT" : "SLAPT");
    fprintf(f.fp, "<RegClass> %d\n", p.regClass == 0 ? 1 : p.regClass);                               // tr:301-307
    fprintf(f.fp, "<%s> %d\n", rapt ? "RAPTParam" : "SLAPTParam", (int) p.conf.size());               // tr:490-501, 542-551
    for (size_t i = 0; i < p.conf.size(); i++)
      fprintf(f.fp, " %g", (rapt && i >= 2 && i % 2 == 0) ? fabs(p.conf[i]) : p.conf[i]);             // an empty RAPT parameter is not written there (it reads _conf[0])
    fprintf(f.fp, "\n");
    if (!p.bias.empty()) {                                                                            // tr:309-319
      fprintf(f.fp, "<BiasOffset> %d\n", (int) p.bias.size());
      for (size_t i = 0; i < p.bias.size(); i++) fprintf(f.fp, " %g", p.bias[i]);
      fprintf(f.fp, "\n");
    }
    fprintf(f.fp, "<EndClass>\n");
  }
}

// ---- the line search -----------------------------------------------------------------------------------------------------------------------
namespace {

// EstimatorBase's constants (eA:81-91)
const unsigned MaxItns = 100;
const double Tolerance = 1.0e-02, ConstGold = 0.3819660, Gold = 1.618034, GoldLimit = 10.0, Tiny = 1.0e-20, ZEpsilon = 1.0e-10;
const double RhoEpsilon = 1.0e-03, MaximumRho = 0.90;

struct Pending { double x; };                             // thrown at the first point without a value
struct TooLong {};

struct Search {
  int kind; const std::vector<double>& vals; std::vector<double> pts;
  Search(int k, const std::vector<double>& v) : kind(k), vals(v) {}
  double calcLogLhood(double x)
  {
    if (pts.size() >= (size_t) kSearchEvalCap) throw TooLong();
    if (pts.size() == vals.size()) throw Pending{x};
    pts.push_back(x); return vals[pts.size() - 1];
  }
  void findRange(double rho, double& mn, double& mx)      // eA:252-255, 1544-1548
  { if (kind == kAptRAPT) { mn = -rho; mx = rho; } else { mn = -100.0; mx = 100.0; } }
  static void swap_(double& a, double& b) { double t = a; a = b; b = t; }
  static void shift_(double& a, double& b, double& c, double d) { a = b; b = c; c = d; }
  static double sign_(double a, double b) { return (b > 0.0) ? fabs(a) : -fabs(a); }
  static void bound(double mn, double mx, double& q) { if (q > mx) q = mx; if (q < mn) q = mn; }     // eA:94-106

  bool bracket(double& ax, double& bx, double& cx)        // eA:109-180
  {
    double fa, fb, fc, ulim, u, r, q, fu, minim, maxim;
    findRange(MaximumRho - RhoEpsilon, minim, maxim);
    bound(minim, maxim, ax);
    fa = -calcLogLhood(ax); if (std::isnan(fa)) return false;
    fb = -calcLogLhood(bx); if (std::isnan(fb)) return false;
    if (fb > fa) { swap_(ax, bx); swap_(fb, fa); }
    cx = bx + Gold * (bx - ax);
    bound(minim, maxim, cx);
    fc = -calcLogLhood(cx); if (std::isnan(fc)) return false;
    while (fb > fc) {
      r = (bx - ax) * (fb - fc);
      q = (bx - cx) * (fb - fa);
      u = bx - ((bx - cx) * q - (bx - ax) * r) / (2.0 * sign_(std::max(fabs(q - r), Tiny), q - r));
      bound(minim, maxim, u);
      ulim = bx + GoldLimit * (cx - bx);
      bound(minim, maxim, ulim);
      if ((bx - u) * (u - cx) > 0.0) {
        fu = -calcLogLhood(u);
        if (fu < fc) { ax = bx; bx = u; fa = fb; fb = fu; return true; }
        else if (fu > fb) { cx = u; fc = fu; return true; }
        u = cx + Gold * (cx - bx);
        bound(minim, maxim, u);
        fu = -calcLogLhood(u);
      } else if ((cx - u) * (u - ulim) > 0.0) {
        fu = -calcLogLhood(u);
        if (fu < fc) {
          shift_(bx, cx, u, cx + Gold * (cx - bx));
          bound(minim, maxim, u);
          shift_(fb, fc, fu, -calcLogLhood(u));
        }
      } else if ((u - ulim) * (ulim - cx) >= 0.0) {
        u = ulim;
        fu = -calcLogLhood(u);
      } else {
        u = cx + Gold * (cx - bx);
        bound(minim, maxim, u);
        fu = -calcLogLhood(u);
      }
      shift_(ax, bx, cx, u);
      shift_(fa, fb, fc, fu);
    }
    return true;
  }

  bool brentsMethod(double ax, double bx, double cx, double& xmin)       // eA:183-240; false: "Too many iterations of Brent's method"
  {
    double a, b, d = 0.0, etemp, fu, fv, fw, fx, p, q, r, tol1, tol2, u, v, w, x, xm, e = 0.0;
    a = std::min(ax, cx);
    b = std::max(ax, cx);
    x = w = v = bx;
    fw = fv = fx = -calcLogLhood(x);
    for (unsigned iter = 0; iter < MaxItns; iter++) {
      xm = 0.5 * (a + b);
      tol2 = 2.0 * (tol1 = Tolerance * fabs(x) + ZEpsilon);
      if (fabs(x - xm) <= (tol2 - 0.5 * (b - a))) { xmin = x; return true; }
      if (fabs(e) > tol1) {
        r = (x - w) * (fx - fv);
        q = (x - v) * (fx - fw);
        p = (x - v) * q - (x - w) * r;
        q = 2.0 * (q - r);
        if (q > 0.0) p = -p;
        q = fabs(q);
        etemp = e;
        e = d;
        if (fabs(p) >= fabs(0.5 * q * etemp) || p <= q * (a - x) || p >= q * (b - x))
          d = ConstGold * (e = (x >= xm ? a - x : b - x));
        else {
          d = p / q;
          u = x + d;
          if (u - a < tol2 || b - u < tol2) d = sign_(tol1, xm - x);
        }
      } else {
        d = ConstGold * (e = (x >= xm ? a - x : b - x));
      }
      u = (fabs(d) >= tol1 ? x + d : x + sign_(tol1, d));
      fu = -calcLogLhood(u);
      if (fu <= fx) {
        if (u >= x) a = x; else b = x;
        shift_(v, w, x, u);
        shift_(fv, fw, fx, fu);
      } else {
        if (u < x) a = u; else b = u;
        if (fu <= fw || w == x) { v = w; w = u; fv = fw; fw = fu; }
        else if (fu <= fv || v == x || v == w) { v = u; fv = fu; }
      }
    }
    return false;
  }
};

}  // namespace

int apt_line_search(int kind, const std::vector<double>& lhood, double* point, std::vector<double>* points)
{
  Search s(kind, lhood); int result;
  try {
    double a, b, c = 0.0, xmin = 0.0;
    if (kind == kAptRAPT) { b = 0.0; a = b + 0.10; } else { a = -0.05; b = 0.0; }
    // the reference does not look at what bracket returns and goes on with an unset cx; here a NaN ends the search
    if (!s.bracket(a, b, c) || !s.brentsMethod(a, b, c, xmin)) result = kSearchFailed;
    else { result = kSearchDone; if (point) *point = xmin; }
  }
  catch (const Pending& p) { result = kSearchNeeds; if (point) *point = p.x; }
  catch (const TooLong&) { result = kSearchFailed; }
  if (points) points->swap(s.pts);
  return result;
}

}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_apt_params_create(const char* fileName, dsr_apt_params** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    dsr_apt_params* t = new dsr_apt_params();
    try { t->read(fileName); } catch (...) { delete t; throw; }
    *out = t;
  });
}
void dsr_apt_params_destroy(dsr_apt_params* t) { delete t; }
dsr_status dsr_apt_params_clear(dsr_apt_params* t) { return guard([&] { if (!t) throw Error(DSR_E_PARAMETER, "null argument"); t->clear(); }); }
dsr_status dsr_apt_params_read(dsr_apt_params* t, const char* fileName)
{ return guard([&] { if (!t) throw Error(DSR_E_PARAMETER, "null argument"); t->read(fileName); }); }
dsr_status dsr_apt_params_write(const dsr_apt_params* t, const char* fileName)
{ return guard([&] { if (!t) throw Error(DSR_E_PARAMETER, "null argument"); t->write(fileName); }); }
dsr_status dsr_apt_params_copy(dsr_apt_params* dst, const dsr_apt_params* src)
{ return guard([&] { if (!dst || !src) throw Error(DSR_E_PARAMETER, "null argument"); if (dst != src) { dst->map = src->map; dst->type = src->type; } }); }
int dsr_apt_params_type(const dsr_apt_params* t) { return t ? t->type : 0; }
int dsr_apt_params_indices(const dsr_apt_params* t, unsigned* indices, int cap)
{
  if (!t) return 0;
  int n = 0;
  for (std::map<unsigned, AptParam>::const_iterator it = t->map.begin(); it != t->map.end(); ++it, ++n) if (indices && n < cap) indices[n] = it->first;
  return n;
}
dsr_status dsr_apt_params_find(dsr_apt_params* t, unsigned rc, int type, int useAncestor, int* nConf, int* nBias)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    if (type != kAptRAPT && type != kAptSLAPT) throw Error(DSR_E_PARAMETER, "adaptation type %d", type);
    const AptParam& p = t->findAPT(rc, type, useAncestor != 0);
    if (nConf) *nConf = (int) p.conf.size();
    if (nBias) *nBias = (int) p.bias.size();
  });
}
dsr_status dsr_apt_params_get(const dsr_apt_params* t, unsigned rc, double* conf, float* bias)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    std::map<unsigned, AptParam>::const_iterator it = t->map.find(rc);
    if (it == t->map.end()) throw Error(DSR_E_INDEX, "Could not find parameters for regression class %d.", rc);
    if (conf) for (size_t i = 0; i < it->second.conf.size(); i++) conf[i] = it->second.conf[i];
    if (bias) for (size_t i = 0; i < it->second.bias.size(); i++) bias[i] = it->second.bias[i];
  });
}
dsr_status dsr_apt_params_set(dsr_apt_params* t, unsigned rc, int type, int nConf, const double* conf, int nBias, const float* bias)
{
  return guard([&] {
    if (!t || nConf < 0 || nBias < 0 || (nConf && !conf) || (nBias && !bias)) throw Error(DSR_E_PARAMETER, "null argument");
    if (type != kAptRAPT && type != kAptSLAPT) throw Error(DSR_E_PARAMETER, "adaptation type %d", type);
    AptParam& p = t->findAPT(rc, type, true);
    p.conf.assign(conf, conf + nConf); p.bias.assign(bias, bias + nBias);
  });
}

dsr_status dsr_apt_line_search(int kind, const double* lhood, int n, int* state, double* point, int* nPoints, double* points)
{
  return guard([&] {
    if (!state || !point || n < 0 || (n && !lhood)) throw Error(DSR_E_PARAMETER, "null argument");
    if (kind != kAptRAPT && kind != kAptSLAPT) throw Error(DSR_E_PARAMETER, "adaptation type %d", kind);
    std::vector<double> v(lhood, lhood + n), pts;
    *state = apt_line_search(kind, v, point, &pts);
    if (nPoints) *nPoints = (int) pts.size();
    if (points) for (size_t i = 0; i < pts.size(); i++) points[i] = pts[i];
  });
}

}  // extern "C"
