/*
 * lincheck_cycles.h — the search for the txn that closes a G-single cycle on
 * the device, and the Elle checkers' host pass restricted to the txns the
 * cycle screen marked (include/lincheck_screen.h).  Included by lincheck.h;
 * additive to ABI 5 (callers detect the feature by looking up lc_cycle_reach
 * and lc_append_check_restricted).
 *
 * 1. lc_cycle_reach: batched backward reachability, first hit.
 *
 * A graph of n_nodes nodes is given by its predecessor lists (a CSR: the
 * predecessors of node b are pred[pred_off[b] .. pred_off[b + 1])), and
 * n_queries queries by a source node q_node[q] each and a list of heads
 * q_heads[q_head_off[q] .. q_head_off[q + 1]).  Query q hits iff some head of
 * q reaches q_node[q] along the graph's edges, that is, iff a breadth-first
 * search from q_node[q] along pred meets a head.  The source is not a head of
 * its own query.  first_hit is the least hitting query, or -1.
 *
 * With LC_REACH_ALL every query is searched to exhaustion (no early exit
 * inside a query or between queries): hit[q] is written for every query, and
 * nodes_visited is the sum over the queries of the nodes the search marked,
 * the source included, a function of the input alone and so equal on host
 * and device.  Without the flag hit is not written (it may be NULL), a query
 * above a known hit may be skipped, a search ends at its first head, and
 * n_queries_run and nodes_visited say what happened to be done.
 *
 * 2. lc_append_check_restricted / lc_wr_check_restricted: the screened calls
 * with rule 7 / rule 9 run over the marked txns only where the screen did not
 * prove the graph clean, the quadratic part of the class loop (which member
 * of an SCC closes a G-single cycle) asked of lc_cycle_reach's kernel.
 */
#ifndef LINCHECK_CYCLES_H
#define LINCHECK_CYCLES_H

#include "lincheck.h"
#include "lincheck_append.h"
#include "lincheck_screen.h"
#include "lincheck_wr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_REACH_ALL 1u /* flags: decide every query; write hit[] */

typedef struct lc_reach_summary {
  int64_t first_hit;      /* the least hitting query, or -1 */
  int64_t n_queries_run;  /* queries whose search began */
  int64_t nodes_visited;  /* LC_REACH_ALL: exact (see above); otherwise informational */
  double  h2d_ms;         /* lc_cycle_reach: the inputs' copies (HIP events); host: 0 */
  double  kernel_ms;      /* lc_cycle_reach: the kernel (HIP events); host: 0 */
  double  total_ms;       /* host wall time of the call */
} lc_reach_summary;

/*
 * Contract of both functions: n_nodes and n_queries in [0, 2^31 - 1);
 * pred_off (n_nodes + 1 entries) starts at 0, does not decrease and ends at
 * n_pred; q_head_off (n_queries + 1 entries) the same, ending at n_heads;
 * every entry of pred, q_node and q_heads is a node; q_node is strictly
 * ascending; no head equals its query's source (the graphs this serves have
 * no edge from a txn to itself).  A violation returns -EINVAL and writes
 * nothing.  n_queries == 0 or n_nodes == 0 is legal (first_hit -1).  sum may
 * be NULL; hit may be NULL without LC_REACH_ALL.
 */

/* The definition on one host thread: the fallback, the device path's oracle
 * and the probe's baseline.  No GPU needed.  0, -EINVAL or -ENOMEM. */
int lc_cycle_reach_host(int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred,
                        int64_t n_queries, const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads,
                        int64_t n_heads, uint32_t flags, int32_t *hit, lc_reach_summary *sum);

/* The same on the context's first GPU.  Every array is host memory; the call
 * is synchronous.  0, -EINVAL (text in lc_last_error; the context stays
 * usable), -E2BIG (n_nodes above lc_cycle_reach_limits' max_nodes; nothing is
 * written), -ENOMEM or -EIO.  A call without nodes or queries is answered by
 * the host code. */
int lc_cycle_reach(lc_ctx *ctx, int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred,
                   int64_t n_queries, const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads,
                   int64_t n_heads, uint32_t flags, int32_t *hit, lc_reach_summary *sum);

typedef struct lc_reach_limit_info {
  int64_t max_nodes;          /* the nodes whose two bitmaps fit one workgroup's LDS */
  int64_t min_work;           /* candidates x (nodes + preds) from which the restricted calls ask the device:
                                 default_min_work unless the environment variable LC_CYCLE_MIN_WORK holds a
                                 non-negative number, read at every call */
  int64_t default_min_work;
  int32_t max_workgroups;     /* a launch starts min(n_queries, max_workgroups, what the queues' room allows) */
  int32_t pad;
} lc_reach_limit_info;

int lc_cycle_reach_limits(lc_reach_limit_info *out);

typedef struct lc_cycle_search_summary {
  int32_t restricted;          /* 1: rule 7 / 9 ran over the marked txns only */
  int32_t pad;
  int64_t n_marked;            /* txns with a mark bit (restricted == 1) */
  int64_t n_device_searches;   /* (SCC, class) pairs whose first closing member the device named */
  int64_t n_device_queries;    /* the candidates of those searches */
  int64_t n_host_fallbacks;    /* searches above min_work that the host loop ran: more than max_nodes, or -E2BIG */
  double  search_ms;           /* the device searches' share of host_graph_ms (host wall time) */
} lc_cycle_search_summary;

/*
 * The screened calls (include/lincheck_screen.h) with the host pass
 * restricted.  By the screen's result:
 *   clean ==  1  as the screened call (nothing runs on the host);
 *   clean ==  0  every member of a nontrivial SCC has a mark bit, so the CSR,
 *                the Tarjan and the class loop cover the marked txns and the
 *                edges between them; restricted = 1;
 *   clean == -1  the whole-graph pass; restricted = 0.
 * Every output array and every count of the summary equals the unscreened
 * call's: the device names only which member of an SCC is the first from
 * which the host's breadth-first search succeeds, and the witness steps are
 * that search's.  Arguments, errors and limits are the screened call's; an
 * error leaves *scr and *srch unwritten.  scr and srch may be NULL.
 */
int lc_append_check_restricted(lc_ctx *ctx, const struct lc_ap_txn *txns, int64_t n_txns,
                               const struct lc_ap_mop *mops, int64_t n_mops, const int64_t *values, int64_t n_values,
                               const struct lc_ap_out *out, struct lc_ap_summary *sum, struct lc_screen_summary *scr,
                               lc_cycle_search_summary *srch);
int lc_wr_check_restricted(lc_ctx *ctx, const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_wr_mop *mops,
                           int64_t n_mops, uint32_t flags, const struct lc_wr_out *out, struct lc_wr_summary *sum,
                           struct lc_screen_summary *scr, lc_cycle_search_summary *srch);

/*
 * Rule 7 alone on the host, for tests and tools: real time's ranges, then the
 * cycles over the whole graph (mark NULL) or over the marked txns (mark:
 * n_txns words, non-zero for at least every member of a nontrivial SCC).
 * reach, where given, answers a class-loop search whose work is at least
 * min_work (first_hit as lc_cycle_reach's; a return other than 0 sends the
 * search to the host loop, counted in n_host_fallbacks, as is a search over
 * more than max_nodes nodes where max_nodes > 0); NULL: the host loop.  The txns and edges obey
 * lc_cycle_screen's contract (not checked).  Written: scc, scc_class (n_txns
 * each), steps (room for n_txns), cycle_off (LC_AP_MAX_CYCLES + 1), cycle_scc
 * (LC_AP_MAX_CYCLES), n_class (8), *n_scc; srch may be NULL.  0 or -ENOMEM.
 */
typedef int (*lc_reach_fn)(void *user, int64_t n_nodes, const int64_t *pred_off, const int32_t *pred,
                           int64_t n_queries, const int32_t *q_node, const int64_t *q_head_off,
                           const int32_t *q_heads, int64_t *first_hit);
int lc_cycles_host(const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_ap_edge *edges, int64_t n_edges,
                   const int32_t *mark, lc_reach_fn reach, void *user, int64_t min_work, int64_t max_nodes, int32_t *scc,
                   int32_t *scc_class, struct lc_ap_step *steps, int64_t *cycle_off, int32_t *cycle_scc,
                   int64_t *n_class, int64_t *n_scc, lc_cycle_search_summary *srch);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_CYCLES_H */
