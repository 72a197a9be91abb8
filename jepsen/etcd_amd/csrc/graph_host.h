// graph_host.h — what the two Elle checkers (lc_append_check, lc_wr_check)
// share on the host once a transaction graph's edges stand: the real-time
// ranges (rule 6 of include/lincheck_append.h) and the cycles (its rule 7:
// SCCs, classes, witness cycles).  Plain inputs, no checker's own structs but
// the txn, edge and step records, which the two checkers have in common.
// g++, no GPU (graph_host.cpp).
#pragma once
#include <stdint.h>

#include <functional>

#include "../../../include/lincheck_append.h"

namespace lcgraph {

// Rule 6 on the host: byc (the OK txns by comp_pos; as many as there are) and
// per txn [rt_lo, rt_hi).
void real_time_host(const lc_ap_txn *txns, int64_t n_txns, int32_t *byc, int32_t *rt_lo, int32_t *rt_hi);

struct CycleCounts {
  int64_t n_class[8];  // nontrivial SCCs per class
  int64_t n_scc, n_cycles_returned;
};

// Rule 7.  The nodes are the txns whose type is not FAIL (n_nodes of them);
// edges are sorted by (from, to, type, key) and unique, both ends nodes; byc
// and the ranges are real_time_host's.  Written: scc and scc_class (n_txns
// each), steps (room for n_txns), cycle_off (LC_AP_MAX_CYCLES + 1), cycle_scc
// (LC_AP_MAX_CYCLES), *counts.
void cycles_host(const lc_ap_txn *txns, int64_t n_txns, int64_t n_nodes, const lc_ap_edge *edges, int64_t n_edges,
                 const int32_t *byc, const int32_t *rt_lo, const int32_t *rt_hi, int32_t *scc, int32_t *scc_class,
                 lc_ap_step *steps, int64_t *cycle_off, int32_t *cycle_scc, CycleCounts *counts);

// What cycles_host writes for a graph without a nontrivial SCC, for a caller
// that knows there is none (lc_cycle_screen's clean = 1): scc and scc_class
// all -1, cycle_off all 0, cycle_scc all -1, no counts.
void no_cycles(int64_t n_txns, int32_t *scc, int32_t *scc_class, int64_t *cycle_off, int32_t *cycle_scc,
               CycleCounts *counts);

// One search of the class loop, on a graph of its own (the nodes are an SCC's
// members in member order): which is the least query whose source some head of
// it reaches?  The arrays are include/lincheck_cycles.h's.
struct ReachProblem {
  int64_t n_nodes;
  const int64_t *pred_off;
  const int32_t *pred;
  int64_t n_queries;
  const int32_t *q_node;
  const int64_t *q_head_off;
  const int32_t *q_heads;
};
// 0 with *first_hit, or an errno: -E2BIG sends the search to the host loop
// (counted as a fallback), any other ends cycles_host_marked with it.
using ReachHook = std::function<int(const ReachProblem &, int64_t *first_hit)>;

// What cycles_host_marked reads beside cycles_host's arguments, and what it
// counts (the fields of lc_cycle_search_summary).
struct MarkedPass {
  const int32_t *mark;  // n_txns: non-zero for at least every member of a nontrivial SCC
  ReachHook hook;       // empty: every search takes the host loop
  int64_t min_work = 0, max_nodes = INT64_MAX;
  int64_t n_marked = 0, n_device_searches = 0, n_device_queries = 0, n_host_fallbacks = 0;
  double search_ms = 0;
};

// cycles_host over the marked txns alone: the CSR, the Tarjan and their
// scratch cover the marked txns and the edges with both ends marked, real
// time's predecessors filtered by the mark.  It writes exactly what
// cycles_host writes where every member of a nontrivial SCC is marked
// (lc_cycle_screen's clean == 0).  0, or the hook's error.
int cycles_host_marked(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
                       const int32_t *byc, int64_t n_ok, const int32_t *rt_lo, const int32_t *rt_hi, MarkedPass *mp,
                       int32_t *scc, int32_t *scc_class, lc_ap_step *steps, int64_t *cycle_off, int32_t *cycle_scc,
                       CycleCounts *counts);

}  // namespace lcgraph
