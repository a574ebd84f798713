// csrc/adapt.cpp -- the host side of MLLR speaker adaptation: the speaker parameter tree and its text files.
//
// Replaces isAncestor (asr/adapt/transform.cc:133-145, "tr"), ParamBase's symbol reader and writer (tr:203-407), MLLRParam (tr:556-650) and
// ParamTree (tr:789-950).  Only the MLLR type is implemented: a file of RAPT or SLAPT parameters is refused with the reference's
// jtype_error, RAPT / SLAPT symbols inside an MLLR class with its jparameter_error.  The reference reads numbers with fscanf; so does this
// file, so that what it accepts and what it stops at are the same.  Compiled with -ffp-contract=off.
#include "common.h"
#include "adapt.h"
#include <cctype>

namespace dsr {

bool isAncestor(unsigned ancestor, unsigned child)
{
  if (ancestor == 0) throw Error(DSR_E_INDEX, "Ancestor index is zero.");
  if (child == 0) throw Error(DSR_E_INDEX, "Child index zero.");
  for (; child >= ancestor; child /= 2) if (child == ancestor) return true;
  return false;
}

void MLLRParam::assign(int D, const double* W)
{
  if (size != D) { size = D; matrix.assign((size_t) D * D, 0.0); }
  if (bias.empty()) bias.resize(D);
  else if ((int) bias.size() != size) throw Error(DSR_E_DIMENSION, "Bias sizes (%d vs. %d) do not match.", (int) bias.size(), size);
  for (int m = 0; m < D; m++) {
    bias[m] = W[(size_t) m * (D + 1) + D];
    for (int n = 0; n < D; n++) matrix[(size_t) m * D + n] = W[(size_t) m * (D + 1) + n];
  }
}

// ParamBase::_symMap / _adaptMap (tr:203-208)
const char* kSymMap[] = { "RegClass", "RAPTParam", "SLAPTParam", "MLLRParam", "STCParam", "LDAParam", "BiasOffset", "EndClass", "AdaptType", "EOF", "" };
static const char* kAdaptMap[] = { "RAPT", "SLAPT", "MLLR", "STC", "LDA", "" };
static const unsigned kMaxSymbolLength = 16;

Symbol getSymbol(FILE* fp)                                // tr:219-242
{
  int c; char buf[kMaxSymbolLength];
  while (isspace(c = getc(fp)));
  if (c == EOF) return SymEOF;
  if (c != '<') throw Error(DSR_E_ERROR, "Symbol expected");
  unsigned i = 0;
  while ((c = getc(fp)) != '>' && c != EOF && i < (kMaxSymbolLength - 1)) buf[i++] = (char) c;
  buf[i] = '\0';
  if (c != '>') throw Error(DSR_E_ERROR, "_getSymbol: > missing in symbol");
  while (isspace(c = getc(fp)));
  if (c != EOF) ungetc(c, fp);
  for (int s = SymRegClass; s <= SymEOF; s++) if (strcmp(kSymMap[s], buf) == 0) return (Symbol) s;
  throw Error(DSR_E_ERROR, "Invalid symbol %s", buf);
}

int getAdaptType(FILE* fp)                                // tr:244-267: 0 RAPT, 1 SLAPT, 2 MLLR
{
  int c; char buf[kMaxSymbolLength];
  while (isspace(c = getc(fp)));
  if (c == EOF) throw Error(DSR_E_ERROR, "No adaptation type specified.");
  ungetc(c, fp);
  unsigned i = 0;
  while ((c = getc(fp)) != EOF && !isspace(c) && i < (kMaxSymbolLength - 1)) buf[i++] = (char) c;
  buf[i] = '\0';
  if (i == (kMaxSymbolLength - 1)) throw Error(DSR_E_ERROR, "Adaptation type %s is not valid.", buf);
  for (int as = 0; as <= 2; as++) if (strcmp(kAdaptMap[as], buf) == 0) return as;
  throw Error(DSR_E_ERROR, "Invalid adaptation type %s", buf);
}

namespace {

void readParams(FILE* fp, MLLRParam& par)                 // ParamBase::_readParams tr:374-407 for _type() == MLLR
{
  Symbol sym;
  while ((sym = getSymbol(fp)) != SymEndClass) {
    switch (sym) {
    case SymAdaptType:
      if (getAdaptType(fp) != 2) throw Error(DSR_E_PARAMETER, "Attempted to read parameters of wrong type.");
      break;
    case SymRegClass:
      if (fscanf(fp, "%u", &par.regClass) != 1) { /* the reference does not look at the count */ }
      break;
    case SymRAPT: case SymSLAPT:
      throw Error(DSR_E_PARAMETER, "Attempted to read MLLR parameters.");
    case SymMLLR: {                                       // MLLRParam::_getParams tr:589-607
      unsigned short sz = 0; if (fscanf(fp, "%hu", &sz) != 1) sz = 0;
      par.size = sz; par.matrix.assign((size_t) sz * sz, 0.0);
      for (size_t e = 0; e < par.matrix.size(); e++) { double v = 0.0; if (fscanf(fp, "%lf", &v) == 1) par.matrix[e] = v; }
      break;
    }
    case SymBias: {                                       // tr:288-299
      int n = 0; if (fscanf(fp, "%d", &n) != 1 || n < 0) n = 0;
      par.bias.assign((size_t) n, 0.0);
      for (int i = 0; i < n; i++) { double v = 0.0; if (fscanf(fp, "%lf", &v) == 1) par.bias[i] = v; }
      break;
    }
    default:
      throw Error(DSR_E_PARAMETER, "Unexpected symbol %s in conformal parameter file.", kSymMap[sym]);
    }
  }
}

bool readParam(FILE* fp, MLLRParam& par)                  // ParamBase::param(FILE*) tr:339-363
{
  int c = getc(fp); if (c == EOF) return false;
  ungetc(c, fp);
  if (getSymbol(fp) != SymAdaptType) throw Error(DSR_E_TYPE, "Unable to determine adaptation type.");
  if (getAdaptType(fp) != 2) throw Error(DSR_E_TYPE, "Unknown adaptation type.");       // RAPT and SLAPT parameters are not implemented
  par = MLLRParam(); readParams(fp, par);
  return true;
}

struct File {
  FILE* fp;
  File(const char* name, const char* mode) : fp(fopen(name, mode)) { if (!fp) throw Error(DSR_E_IO, "Could not open file %s.", name); }
  ~File() { if (fp) fclose(fp); }
};

MLLRParam& nearest(ParamTree& t, unsigned initRC, bool useAncestor, bool mllr)
{
  if (mllr) {
    if (t.type == kAdaptUnspecified) t.type = kAdaptMLLR;
    else if (t.type != kAdaptMLLR) throw Error(DSR_E_CONSISTENCY, "Tree not instantiated with MLLR parameters.");
  }
  if (initRC == 0) throw Error(DSR_E_INDEX, "Regression class index is zero");
  std::map<unsigned, MLLRParam>::iterator itr = t.map.find(initRC);
  if (itr != t.map.end()) return itr->second;
  if (!useAncestor)
    throw Error(DSR_E_INDEX, mllr ? "Could not find parameters for regression class %d." : "No parameters for index %d.", initRC);
  unsigned reg = initRC / 2;
  while (reg > 0 && (itr = t.map.find(reg)) == t.map.end()) reg /= 2;
  if (reg == 0 && !mllr) throw Error(DSR_E_INDEX, "No ancestor for node %d.", initRC);
  MLLRParam par = reg == 0 ? MLLRParam() : itr->second;   // the copy of the nearest ancestor (findMLLR: an empty parameter without one)
  par.regClass = initRC;
  return t.map.insert(std::make_pair(initRC, par)).first->second;
}

}  // namespace

MLLRParam& ParamTree::find(unsigned rc, bool useAncestor) { return nearest(*this, rc, useAncestor, false); }
MLLRParam& ParamTree::findMLLR(unsigned rc, bool useAncestor) { return nearest(*this, rc, useAncestor, true); }

void ParamTree::read(const char* fileName)
{
  clear();
  if (!fileName || !*fileName) return;
  File f(fileName, "r");
  std::map<unsigned, MLLRParam> m; MLLRParam par;
  while (readParam(f.fp, par)) m.insert(std::make_pair(par.regClass, par));     // map::insert: the first class of an index stays
  if (m.empty()) throw Error(DSR_E_CONSISTENCY, "Unable to determine adaptation type.");
  map.swap(m); type = kAdaptMLLR;
}

void ParamTree::write(const char* fileName) const
{
  if (!fileName) throw Error(DSR_E_PARAMETER, "null argument");
  File f(fileName, "w");
  for (std::map<unsigned, MLLRParam>::const_iterator it = map.begin(); it != map.end(); ++it) {      // ParamBase::write tr:365-372, index order
    const MLLRParam& p = it->second;
    fprintf(f.fp, "<AdaptType> MLLR\n");
    fprintf(f.fp, "<RegClass> %d\n", p.regClass == 0 ? 1 : p.regClass);                              // tr:301-307
    fprintf(f.fp, "<MLLRParam> %d\n", p.size);                                                        // tr:576-587
    for (int m = 0; m < p.size; m++) {
      for (int n = 0; n < p.size; n++) fprintf(f.fp, " %g", p.matrix[(size_t) m * p.size + n]);
      fprintf(f.fp, "\n");
    }
    if (!p.bias.empty()) {                                                                            // tr:309-319
      fprintf(f.fp, "<BiasOffset> %d\n", (int) p.bias.size());
      for (size_t i = 0; i < p.bias.size(); i++) fprintf(f.fp, " %g", p.bias[i]);
      fprintf(f.fp, "\n");
    }
    fprintf(f.fp, "<EndClass>\n");
  }
}

}  // namespace dsr

using namespace dsr;

extern "C" {

dsr_status dsr_is_ancestor(unsigned ancestor, unsigned child, int* result)
{ return guard([&] { if (!result) throw Error(DSR_E_PARAMETER, "null argument"); *result = isAncestor(ancestor, child) ? 1 : 0; }); }

dsr_status dsr_param_tree_create(const char* fileName, dsr_param_tree** out)
{
  return guard([&] {
    if (!out) throw Error(DSR_E_PARAMETER, "null argument");
    dsr_param_tree* t = new dsr_param_tree();
    try { t->read(fileName); } catch (...) { delete t; throw; }
    *out = t;
  });
}
void dsr_param_tree_destroy(dsr_param_tree* t) { delete t; }
dsr_status dsr_param_tree_clear(dsr_param_tree* t) { return guard([&] { if (!t) throw Error(DSR_E_PARAMETER, "null argument"); t->clear(); }); }
dsr_status dsr_param_tree_read(dsr_param_tree* t, const char* fileName)
{ return guard([&] { if (!t) throw Error(DSR_E_PARAMETER, "null argument"); t->read(fileName); }); }
dsr_status dsr_param_tree_write(const dsr_param_tree* t, const char* fileName)
{ return guard([&] { if (!t) throw Error(DSR_E_PARAMETER, "null argument"); t->write(fileName); }); }
dsr_status dsr_param_tree_copy(dsr_param_tree* dst, const dsr_param_tree* src)
{ return guard([&] { if (!dst || !src) throw Error(DSR_E_PARAMETER, "null argument"); if (dst != src) { dst->map = src->map; dst->type = src->type; } }); }
int dsr_param_tree_type(const dsr_param_tree* t) { return t ? t->type : 0; }
int dsr_param_tree_has_index(const dsr_param_tree* t, unsigned rc) { return t && t->hasIndex(rc) ? 1 : 0; }
int dsr_param_tree_indices(const dsr_param_tree* t, unsigned* indices, int cap)
{
  if (!t) return 0;
  int n = 0;
  for (std::map<unsigned, MLLRParam>::const_iterator it = t->map.begin(); it != t->map.end(); ++it, ++n) if (indices && n < cap) indices[n] = it->first;
  return n;
}
dsr_status dsr_param_tree_find(dsr_param_tree* t, unsigned rc, int useAncestor, int mllr, int* size)
{
  return guard([&] {
    if (!t) throw Error(DSR_E_PARAMETER, "null argument");
    const MLLRParam& p = mllr ? t->findMLLR(rc, useAncestor != 0) : t->find(rc, useAncestor != 0);
    if (size) *size = p.size;
  });
}
dsr_status dsr_param_tree_get(const dsr_param_tree* t, unsigned rc, double* W)
{
  return guard([&] {
    if (!t || !W) throw Error(DSR_E_PARAMETER, "null argument");
    std::map<unsigned, MLLRParam>::const_iterator it = t->map.find(rc);
    if (it == t->map.end()) throw Error(DSR_E_INDEX, "No parameters for index %d.", rc);
    const MLLRParam& p = it->second; const int D = p.size;
    for (int m = 0; m < D; m++) {
      for (int n = 0; n < D; n++) W[(size_t) m * (D + 1) + n] = p.matrix[(size_t) m * D + n];
      W[(size_t) m * (D + 1) + D] = m < (int) p.bias.size() ? p.bias[m] : 0.0;
    }
  });
}
dsr_status dsr_param_tree_set(dsr_param_tree* t, unsigned rc, int D, const double* W)
{
  return guard([&] {
    if (!t || !W || D < 1) throw Error(DSR_E_PARAMETER, "null argument");
    t->findMLLR(rc, true).assign(D, W);
  });
}

}  // extern "C"
