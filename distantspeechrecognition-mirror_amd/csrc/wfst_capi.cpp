// csrc/wfst_capi.cpp -- the dsr_wfst_* entries of the C-ABI over WfstGraph (wfst_graph.h; the handle type dsr_wfst is declared there)
#include "common.h"
#include "wfst_graph.h"
#include "lexicon.h"

using namespace dsr;

extern "C" {

dsr_status dsr_wfst_create(dsr_wfst** out) { return guard([&] { if (!out) throw Error(DSR_E_PARAMETER, "null argument"); *out = new dsr_wfst(); }); }
// WFSTFlyWeightSortedOutput(statelex, inlex, outlex) (decoder.i; wfstFlyWeight.h:403-424): the same container with every node's arcs kept ordered by
// (output, input); call on an empty transducer
dsr_status dsr_wfst_set_sorted_output(dsr_wfst* g, int on)
{ return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); if (!g->arcs.empty()) throw Error(DSR_E_CONSISTENCY, "the transducer already has arcs"); g->sortedOutput = on != 0; }); }
void dsr_wfst_destroy(dsr_wfst* g) { delete g; }
dsr_status dsr_wfst_read(dsr_wfst* g, const char* f, int binary) { return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->read(f, binary != 0); }); }
dsr_status dsr_wfst_read_dynamic(dsr_wfst* g, const char* f, int noSelfLoops) { return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->readEx(f, false, noSelfLoops != 0); }); }
dsr_status dsr_wfst_write(const dsr_wfst* g, const char* f, int binary) { return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->write(f, binary != 0); }); }
// WFSTFlyWeight::write(fileName, binary, useSymbols) (wfstFlyWeight.cc:415-463): with useSymbols every arc line carries the lexica's strings (Edge::write
// :499-516: states too when the state lexicon is non-empty, costs below 1e-4 left out); final-state lines and -- with binary -- the end marker stay numeric
dsr_status dsr_wfst_write_symbols(const dsr_wfst* g, const char* f, int binary, int useSymbols)
{ return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->write(f, binary != 0, useSymbols != 0); }); }
// WFSTFlyWeight::reverse(wfst) (:141-213) and reverseRead(fileName) (:215-297)
dsr_status dsr_wfst_reverse(dsr_wfst* g, const dsr_wfst* src)
{ return guard([&] { if (!g || !src) throw Error(DSR_E_PARAMETER, "null argument"); g->reverse(*src); }); }
dsr_status dsr_wfst_reverse_read(dsr_wfst* g, const char* f)
{ return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->reverseRead(f); }); }
dsr_status dsr_wfst_add_arc(dsr_wfst* g, unsigned s1, unsigned s2, unsigned in, unsigned out, float cost)
{ return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->addArc(s1, s2, in, out, cost, true); }); }
dsr_status dsr_wfst_add_final(dsr_wfst* g, unsigned s, float cost) { return guard([&] { if (!g) throw Error(DSR_E_PARAMETER, "null argument"); g->addFinal(s, cost); }); }
int dsr_wfst_num_nodes(const dsr_wfst* g) { return (int) g->nodes.size(); }
int dsr_wfst_num_arcs(const dsr_wfst* g) { return (int) g->arcs.size(); }
dsr_status dsr_wfst_export(const dsr_wfst* g, uint32_t* nodeState, int32_t* nodeFinal, float* nodeCost, int32_t* arcOff,
                           int32_t* arcDst, uint32_t* arcIn, uint32_t* arcOut, float* arcCost)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null argument");
    const WfstGraph::Csr c = g->csr(); const size_t n = g->nodes.size();
    for (size_t i = 0; i < n; i++) { if (nodeState) nodeState[i] = g->nodes[i].state; if (nodeFinal) nodeFinal[i] = g->nodes[i].final_; if (nodeCost) nodeCost[i] = g->nodes[i].cost; }
    if (arcOff) for (size_t i = 0; i <= n; i++) arcOff[i] = c.off[i];
    for (size_t a = 0; a < c.dst.size(); a++) { if (arcDst) arcDst[a] = c.dst[a]; if (arcIn) arcIn[a] = c.in[a]; if (arcOut) arcOut[a] = c.out[a]; if (arcCost) arcCost[a] = c.cost[a]; }
  });
}

// WFSTFlyWeight(statelex, inlex, outlex) (decoder.i:52-70): the lexica are borrowed (the reference holds reference-counted pointers); the text reader
// looks non-numeric fields up in them (wfstFlyWeight.cc:311-347)
dsr_status dsr_wfst_set_lexicons(dsr_wfst* g, dsr_lexicon* stateLex, dsr_lexicon* inputLex, dsr_lexicon* outputLex)
{
  return guard([&] {
    if (!g) throw Error(DSR_E_PARAMETER, "null argument");
    g->lexState = stateLex; g->lexIn = inputLex; g->lexOut = outputLex;
    g->symbolOf = [g](int which, const char* t) -> uint32_t {
      dsr_lexicon* l = which == 0 ? g->lexState : which == 1 ? g->lexIn : g->lexOut;
      if (!l) throw Error(DSR_E_KEY, "field '%s' is not a number and the transducer has no %s lexicon", t, which == 0 ? "state" : which == 1 ? "input" : "output");
      return l->index(t);
    };
    g->nameOf = [g](int which, uint32_t i) -> std::string {
      const dsr_lexicon* l = which == 0 ? g->lexState : which == 1 ? g->lexIn : g->lexOut;
      if (!l) throw Error(DSR_E_KEY, "the transducer has no %s lexicon", which == 0 ? "state" : which == 1 ? "input" : "output");
      return l->symbol(i);
    };
    g->stateLexSize = [g]() -> size_t { return g->lexState ? g->lexState->syms.size() : 0; };
  });
}
dsr_lexicon* dsr_wfst_state_lexicon(const dsr_wfst* g) { return g ? g->lexState : nullptr; }
dsr_lexicon* dsr_wfst_input_lexicon(const dsr_wfst* g) { return g ? g->lexIn : nullptr; }
dsr_lexicon* dsr_wfst_output_lexicon(const dsr_wfst* g) { return g ? g->lexOut : nullptr; }
int dsr_wfst_has_final_state(const dsr_wfst* g) { if (!g) return 0; for (size_t i = 0; i < g->nodes.size(); i++) if (g->nodes[i].final_) return 1; return 0; }

}  // extern "C"
