/*
 * lincheck_append.h — lc_append_check: Elle's list-append checker under
 * :consistency-models [:strict-serializable], with the dependency graph built
 * on the device.  The caller hands over the transactions, their micro-ops and
 * the reads' payloads as flat arrays; the library flags every read, derives
 * every key's version order, builds the ww / wr / rw edges and the real-time
 * predecessor ranges, finds the cycles and gives the verdict.
 * Included by lincheck.h; additive to ABI 5 (callers detect the feature by
 * looking up lc_append_check).
 *
 * The rules below are a re-derivation of elle.list-append (elle 0.2.x, as
 * jepsen.tests.cycle.append calls it).  They are this feature's
 * specification; parity with Elle itself is unpinned.
 *
 * Positions are history positions (the order of the op maps), below 2^31 - 1.
 * Only client ops with :f :txn matter.  Keys and elements are int64 (the
 * binding interns anything else); INT64_MIN is reserved.
 *
 *  1. Writers.  Each append mop makes (key, element) -> (its txn, whether it
 *     is the txn's last append to that key, the txn's type).  Two appends of
 *     one (key, element) are not expressible: -EINVAL.
 *  2. Version order of a key: the longest len >= 0 read of the key; among
 *     equal lengths the read of least index (mops are numbered as they lie in
 *     the array).  A read is a prefix read iff it equals the first len
 *     entries of that order.  A key with any non-prefix read is
 *     incompatible-order (LC_AP_K_INCOMPATIBLE on the key, LC_AP_R_NONPREFIX
 *     on those reads).  Per key, -1 where there is none:
 *       first_dup      the least index whose element occurred earlier in the order
 *       first_failed   the least index whose writer is a FAIL txn
 *       first_phantom  the least index with no writer
 *     A key that is incompatible, or has a first_dup or a first_phantom, has
 *     no version order and contributes no edges.
 *  3. Per read of an OK txn:
 *       duplicate-elements  iff some element occurs twice in it
 *       G1a                 iff it holds an element whose writer is FAIL
 *       phantom             iff it holds an element with no writer (not one of
 *                           Elle's names: Elle is written for histories that
 *                           never read an unwritten value; counted, and it
 *                           makes the history invalid)
 *     — for a prefix read these three are len > first_* of its key —
 *       G1b                 iff its last element's writer is another txn and
 *                           that append is not the writer's last append to the key.
 *  4. Internal.  Walk a txn's mops in order, per key.  A read with an earlier
 *     read of the same key in the txn must equal the latest such read followed
 *     by the txn's own appends since.  A read preceded only by own appends
 *     a1..aj must end with them.  Otherwise the read is the txn's external
 *     read of the key (LC_AP_R_EXTERNAL).  A violation flags the read
 *     (LC_AP_R_INTERNAL) and the txn.
 *  5. Nodes and edges.  Graph nodes are the OK and INFO txns.  For a key with
 *     a version order o[0..n):  ww: writer(o[i]) -> writer(o[i+1]);  for each
 *     external prefix read of length L by an OK txn t:  wr: writer(o[L-1]) -> t
 *     when L > 0;  rw: t -> writer(o[L]) when L < n.  An edge exists only when
 *     both ends are nodes and differ.  The edges come back sorted by (from,
 *     to, type, key) and unique; there are at most 2 * reads + appends.
 *  6. Real time: Elle's frontier walk, transitively reduced.  A -> B iff
 *     comp(A) < inv(B) and no OK txn C has comp(A) < inv(C) and comp(C) <
 *     inv(B).  INFO txns never complete: successors, never predecessors.
 *     Equivalently: with byc the OK txns sorted by comp_pos and m(B) the
 *     largest inv_pos among OK txns with comp < inv(B), B's predecessors are
 *     the contiguous run of byc with m(B) < comp < inv(B).  byc and per txn
 *     [rt_lo, rt_hi) are returned; nothing else is materialised.  Process
 *     edges are not built: a process's ops are sequential, real time has them.
 *  7. Cycles.  SCCs of the whole graph (ww + wr + rw + rt).  Each nontrivial
 *     SCC gets the first class that holds inside it:
 *       G0        a cycle of ww edges alone
 *       G1c       a wr edge inside an SCC of {ww, wr}
 *       G-single  an rw edge u -> v with v reaching u through {ww, wr}
 *       G2-item   {ww, wr, rw} is cyclic
 *     then the same four with rt added to each edge set (…-realtime).  Elle
 *     may report more than one class for such an SCC; this rule is ours and
 *     the verdict does not depend on it.  For the first LC_AP_MAX_CYCLES
 *     nontrivial SCCs, in order of their least txn, one witness cycle found by
 *     breadth-first search under the class's edge set is returned: each step
 *     is {txn, edge type to the next step, key}; the last step leads back to
 *     the first.
 *  8. Verdict.  No OK txn: unknown (Elle's empty transaction graph).  Any
 *     flag of rules 2-4, or any nontrivial SCC: invalid.  Otherwise valid.
 */
#ifndef LINCHECK_APPEND_H
#define LINCHECK_APPEND_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_AP_OK   0  /* lc_ap_txn.type */
#define LC_AP_INFO 1
#define LC_AP_FAIL 2
#define LC_AP_APPEND 0  /* lc_ap_mop.f */
#define LC_AP_READ   1
#define LC_AP_WW 0  /* edge types */
#define LC_AP_WR 1
#define LC_AP_RW 2
#define LC_AP_RT 3  /* in witness steps only */
#define LC_AP_MAX_CYCLES 16

/* per-read flags (mop_flags; 0 for appends and ignored reads) */
#define LC_AP_R_NONPREFIX 1   /* incompatible-order */
#define LC_AP_R_DUPLICATE 2
#define LC_AP_R_G1A       4
#define LC_AP_R_PHANTOM   8
#define LC_AP_R_G1B       16
#define LC_AP_R_INTERNAL  32
#define LC_AP_R_EXTERNAL  64  /* not an anomaly: the txn's external read of its key */
#define LC_AP_R_ANOMALY   63
/* per-txn flags: the OR of its reads' anomaly flags */
/* per-key flags */
#define LC_AP_K_INCOMPATIBLE 1
#define LC_AP_K_NO_ORDER     2  /* incompatible, or first_dup / first_phantom >= 0 */

/* classes of rule 7, in its order */
#define LC_AP_G0       0
#define LC_AP_G1C      1
#define LC_AP_G_SINGLE 2
#define LC_AP_G2_ITEM  3
#define LC_AP_REALTIME 4  /* added to the four above */

typedef struct lc_ap_txn {
  int64_t mop_off;   /* its mops are mops[mop_off .. mop_off + mop_len) */
  int32_t inv_pos;
  int32_t comp_pos;  /* OK, FAIL: the completion, above inv_pos; INFO: -1 */
  int32_t type;      /* LC_AP_OK / INFO / FAIL */
  int32_t mop_len;
} lc_ap_txn;         /* 24 bytes */

typedef struct lc_ap_mop {
  int64_t key;
  int64_t value;     /* APPEND: the element; READ: the payload's offset in values */
  int32_t f;         /* LC_AP_APPEND / LC_AP_READ */
  int32_t len;       /* READ: the list's length; -1 in an INFO or FAIL txn (ignored) */
} lc_ap_mop;         /* 24 bytes */

typedef struct lc_ap_edge {
  int32_t from, to;  /* txns */
  int32_t type;      /* LC_AP_WW / WR / RW */
  int32_t pad;
  int64_t key;
} lc_ap_edge;        /* 24 bytes */

typedef struct lc_ap_key {
  int64_t key;
  int64_t longest;   /* the mop that is the key's longest read; -1: never read */
  int32_t len;       /* its length (0 without one) */
  int32_t flags;     /* LC_AP_K_* */
  int32_t first_dup, first_failed, first_phantom;
  int32_t pad;
} lc_ap_key;         /* 40 bytes */

typedef struct lc_ap_step {
  int32_t txn;
  int32_t type;      /* of the edge to the next step: LC_AP_WW / WR / RW / RT */
  int64_t key;       /* 0 for LC_AP_RT */
} lc_ap_step;        /* 16 bytes */

/* Where the results go; every array is the caller's, n_reads being the number
 * of READ mops and n_appends that of APPEND mops. */
typedef struct lc_ap_out {
  int32_t *mop_flags;     /* n_mops */
  int32_t *txn_flags;     /* n_txns */
  lc_ap_key *keys;        /* room for n_mops; sum->n_keys written, ascending by key */
  lc_ap_edge *edges;      /* room for 2 * n_reads + n_appends; sum->n_edges written */
  int32_t *byc;           /* room for n_txns; sum->n_ok written */
  int32_t *rt_lo, *rt_hi; /* n_txns: the txn's predecessors are byc[rt_lo .. rt_hi) */
  int32_t *scc;           /* n_txns: the txn's nontrivial SCC (numbered by least txn), else -1 */
  int32_t *scc_class;     /* n_txns: that SCC's class, else -1 */
  lc_ap_step *steps;      /* room for n_txns (the SCCs are disjoint) */
  int64_t *cycle_off;     /* LC_AP_MAX_CYCLES + 1: cycle c is steps[cycle_off[c] .. cycle_off[c+1]) */
  int32_t *cycle_scc;     /* LC_AP_MAX_CYCLES: its SCC */
} lc_ap_out;

typedef struct lc_ap_summary {
  int32_t valid;          /* 1 / 0 / -1 (unknown) */
  int32_t pad;
  int64_t n_incompatible_order;  /* keys */
  int64_t n_nonprefix, n_duplicate, n_g1a, n_phantom, n_g1b, n_internal;  /* reads of OK txns */
  int64_t n_class[8];     /* nontrivial SCCs per class */
  int64_t n_keys, n_ok, n_nodes, n_edges, n_scc, n_cycles_returned;
  int64_t n_slow_reads;   /* lc_append_check: reads whose rules 3 and 4 the host recomputed: those of
                             txns with a non-prefix read or a read of an order with two phantoms
                             (0 from the host function) */
  double  h2d_ms;         /* lc_append_check: the inputs' copies (HIP events) */
  double  kernel_ms;      /* lc_append_check: the kernels' two runs, a HIP-event interval each (before and
                             after the call's first synchronisation); the per-call memsets, the copies
                             out and the host's wait between the runs are outside */
  double  host_graph_ms;  /* rule 7 (SCCs, classes, witness cycles), host wall time */
  double  total_ms;       /* host wall time of the call */
} lc_ap_summary;

/*
 * Contract of both functions: txns strictly ascending by inv_pos; positions
 * in [0, 2^31 - 1); type OK or FAIL with comp_pos > inv_pos, or INFO with
 * comp_pos -1; the txns' mop ranges tile [0, n_mops) in txn order, without
 * gaps; f APPEND or READ; no key and no appended element INT64_MIN; a
 * READ of an OK txn has 0 <= value, 0 <= len, value + len <= n_values (ranges
 * may overlap), a READ of another txn len -1; n_mops and the payload's total
 * length below 2^31.  A violation, or two appends of one (key, element),
 * returns -EINVAL and writes nothing to out or sum.  n_txns == 0 is legal
 * (unknown).  sum may be NULL; out and its arrays may not.  Positions are
 * taken to be distinct, as history positions are; that is not checked.
 * A txn's mops are walked per mop of the txn: the work is quadratic in a
 * txn's own length, which the workload keeps to a handful.
 */

/* The rules on the host, single-threaded: the fallback, the device path's
 * oracle and the probe's baseline.  No GPU needed.  0, -EINVAL or -ENOMEM. */
int lc_append_check_host(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops,
                         const int64_t *values, int64_t n_values, const lc_ap_out *out, lc_ap_summary *sum);

/* The same with rules 1-6 on the context's first GPU and rule 7 by the host
 * code over the device's edges.  Every array is host memory; the call is
 * synchronous.  0, -EINVAL (text in lc_last_error; the context stays usable),
 * -E2BIG (a payload or a mop count above lc_append_limits), -ENOMEM or -EIO.  A call without txns is
 * answered by the host code. */
int lc_append_check(lc_ctx *ctx, const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops,
                    const int64_t *values, int64_t n_values, const lc_ap_out *out, lc_ap_summary *sum);

/*
 * Limits.  The device call keeps everything resident (there are no tiles):
 * a call whose payload (n_values) or whose reads' total length exceeds
 * max_payload entries is refused with -E2BIG.  Device memory per call: 8 B
 * per payload entry, 28 B per entry of a read (its writer and its ww edge
 * slot), about 150 B per read (wr / rw slots and the edge sort's buffers),
 * and 170 to 300 B per mop (the input, both hash tables at 2 to 4 slots per
 * entry, the key records, the flags): about 36 B per payload entry where the
 * reads are long, so about 39 GB at the default max_payload of 2^30 — a
 * size that was not measured; the largest measured call held 1.9 x 10^7
 * payload entries and 2.5 x 10^6 mops.  max_payload is
 * default_max_payload unless the environment variable LC_AP_MAX_PAYLOAD
 * holds a positive number, read at every call.  The device call also refuses
 * more than max_mops mops with -E2BIG: the key table has the least power of
 * two of slots that is at least twice the mops, and a slot index is an int32.
 * max_mops is 2^29, or a positive number below that in the environment
 * variable LC_AP_MAX_MOPS.  (The host function takes any n_mops below
 * 2^31 - 1.)  Host-only.
 */
typedef struct lc_ap_limit_info {
  int64_t max_payload;
  int64_t default_max_payload;
  int64_t max_position;   /* positions are below this */
  int64_t max_mops;       /* lc_append_check: n_mops is at most this */
} lc_ap_limit_info;

int lc_append_limits(lc_ap_limit_info *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_APPEND_H */
