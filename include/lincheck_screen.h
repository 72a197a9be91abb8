/*
 * lincheck_screen.h — lc_cycle_screen: an exact screen that proves a
 * transaction graph free of nontrivial SCCs on the device, so that the host's
 * graph pass (rule 7 of include/lincheck_append.h, rule 9 of
 * include/lincheck_wr.h) can be skipped for the histories that have none.
 * Included by lincheck.h; additive to ABI 5 (callers detect the feature by
 * looking up lc_cycle_screen).
 *
 * The graph.  Nodes are the txns whose type is not FAIL.  Edges are the data
 * edges handed in (ww, wr, rw) and real time, unreduced: u => v iff u is OK
 * and comp_pos(u) < inv_pos(v).  (Its closure is that of rule 6's reduced
 * relation, so the SCCs are the same.)
 *
 * Two labels per node, over paths of >= 0 edges of any kind:
 *   H(u)  the least comp_pos of an OK node reachable from u; INT32_MAX if none
 *   K(u)  the greatest inv_pos of a node that reaches u
 *
 *  1. u lies in a nontrivial SCC with a real-time edge inside it iff
 *     H(u) < K(u).
 *  2. H and K are constant on an SCC, so a nontrivial SCC of nodes with
 *     H >= K has data edges only, between nodes of one (H, K).  Restrict to
 *     those nodes and to the data edges whose ends have equal (H, K), and drop,
 *     again and again, every node without such an in-edge or such an out-edge:
 *     what is left is non-empty iff such an SCC exists and holds every member
 *     of one.
 * The history has no nontrivial SCC iff no node has H < K and the trim leaves
 * nothing (DESIGN.md §9 has the proofs).
 *
 * Both labels are computed by Jacobi rounds (round r reads only round r - 1's
 * labels, so the number of rounds is a function of the graph):
 *   H0(u) = comp_pos(u) if OK else INT32_MAX;  K0(u) = inv_pos(u)
 *   H'(u) = min(H(u), min over data edges u -> v of H(v), [u OK] S[first(u)])
 *   K'(v) = max(K(v), max over data edges u -> v of K(u), P[rt_hi(v)])
 * S[i] being the least H among txns of index >= i, first(u) the least index
 * whose inv_pos is above comp_pos(u), P[i] the greatest K among byc[0 .. i)
 * and rt_hi(v) the number of OK txns completed before v's invoke (rule 6).
 * The labels have converged in the first round that changes nothing;
 * label_rounds counts the rounds up to and including that one, and
 * trim_rounds counts the trim's the same way.  A phase gives up when round
 * max_rounds still changed something: then clean is -1, the labels are those
 * of that round (still sound: H is an upper and K a lower bound, so a set
 * bit 0 is right, a clear one proves nothing), and the trim, if it is the
 * labels that gave up, did not run (trim_rounds 0, no bit 1).  Where the trim
 * gave up, bit 1 marks what its last round left: a superset.
 */
#ifndef LINCHECK_SCREEN_H
#define LINCHECK_SCREEN_H

#include "lincheck.h"
#include "lincheck_append.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_SCREEN_RT   1  /* mark: H < K, the txn is in an SCC with a real-time edge inside */
#define LC_SCREEN_TRIM 2  /* mark: the txn survives the trim */

/* Where the results go; every array is the caller's, n_txns entries each. */
typedef struct lc_screen_out {
  int32_t *reach_lo;  /* H; INT32_MAX for a FAIL txn */
  int32_t *reach_hi;  /* K; -1 for a FAIL txn */
  int32_t *mark;      /* LC_SCREEN_*; 0 for a FAIL txn */
} lc_screen_out;

typedef struct lc_screen_summary {
  int32_t clean;         /* 1: no nontrivial SCC (proved); 0: not proved; -1: gave up */
  int32_t label_rounds, trim_rounds, max_rounds;
  int64_t n_rt_members;      /* txns with LC_SCREEN_RT */
  int64_t n_trim_survivors;  /* txns with LC_SCREEN_TRIM */
  double  h2d_ms;     /* lc_cycle_screen: the inputs' copies (HIP events) */
  double  kernel_ms;  /* lc_cycle_screen: from the first kernel to the last, the host's waits for a
                         batch of rounds included (HIP events) */
  double  total_ms;   /* host wall time of the call */
} lc_screen_summary;

/*
 * Contract of both functions: txns strictly ascending by inv_pos; positions
 * in [0, 2^31 - 1); type OK or FAIL with comp_pos > inv_pos, or INFO with
 * comp_pos -1 (mop_off and mop_len are not read); edges strictly ascending by
 * (from, to, type, key), both ends txns in range that are not FAIL and differ.
 * A violation returns -EINVAL and writes nothing to out or sum.  n_txns == 0
 * is legal (clean, no rounds).  sum may be NULL; out and its arrays may not.
 * Positions are taken to be distinct, as history positions are.
 * The txn and edge records are list-append's (include/lincheck_append.h).
 * An edge from a txn to itself is refused because it would be a cycle the
 * two labels cannot see; no caller in this library can hand one in: rule 5 of
 * both checkers drops an edge whose two ends are one txn, on the device and in
 * the host functions alike.
 */

/* The definition on one host thread: the fallback, the device path's oracle
 * and the probe's baseline.  No GPU needed.  0, -EINVAL or -ENOMEM. */
int lc_cycle_screen_host(const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_ap_edge *edges,
                         int64_t n_edges, const lc_screen_out *out, lc_screen_summary *sum);

/* The same on the context's first GPU.  Every array is host memory; the call
 * is synchronous.  0, -EINVAL (text in lc_last_error; the context stays
 * usable), -ENOMEM or -EIO.  A call without txns is answered by the host
 * code. */
int lc_cycle_screen(lc_ctx *ctx, const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_ap_edge *edges,
                    int64_t n_edges, const lc_screen_out *out, lc_screen_summary *sum);

/* max_rounds is default_max_rounds unless the environment variable
 * LC_SCREEN_MAX_ROUNDS holds a positive number, read at every call. */
typedef struct lc_screen_limit_info {
  int32_t max_rounds;
  int32_t default_max_rounds;
} lc_screen_limit_info;

int lc_screen_limits(lc_screen_limit_info *out);

/*
 * lc_append_check and lc_wr_check (include/lincheck_append.h,
 * include/lincheck_wr.h) with the screen run on the edges and the real-time
 * ranges while they still stand on the device, before the edges are copied
 * out.  Where the screen proves the graph clean (scr->clean == 1), rule 7 /
 * rule 9 is not run on the host: scc and scc_class are filled with -1,
 * cycle_off with zeros, cycle_scc with -1, the counts are zero, and
 * host_graph_ms is the time of that fill.  Otherwise (clean 0 or -1) the host
 * pass runs on the whole graph as in the unscreened call.  Every output array
 * and every count of the summary equals the unscreened call's in both cases;
 * arguments, errors and limits are the unscreened call's, and an error leaves
 * *scr unwritten.  scr may be NULL.  scr->h2d_ms is 0 (nothing is copied in
 * for the screen); its kernel_ms and total_ms are the screen's share of the
 * call.  A call without txns is answered by the host code (clean, no rounds).
 */
int lc_append_check_screened(lc_ctx *ctx, const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_ap_mop *mops,
                             int64_t n_mops, const int64_t *values, int64_t n_values, const struct lc_ap_out *out,
                             struct lc_ap_summary *sum, lc_screen_summary *scr);
int lc_wr_check_screened(lc_ctx *ctx, const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_wr_mop *mops,
                         int64_t n_mops, uint32_t flags, const struct lc_wr_out *out, struct lc_wr_summary *sum,
                         lc_screen_summary *scr);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_SCREEN_H */
