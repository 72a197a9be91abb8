// graph_host.h — what the two Elle checkers (lc_append_check, lc_wr_check)
// share on the host once a transaction graph's edges stand: the real-time
// ranges (rule 6 of include/lincheck_append.h) and the cycles (its rule 7:
// SCCs, classes, witness cycles).  Plain inputs, no checker's own structs but
// the txn, edge and step records, which the two checkers have in common.
// g++, no GPU (graph_host.cpp).
#pragma once
#include <stdint.h>

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

}  // namespace lcgraph
