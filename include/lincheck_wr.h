/*
 * lincheck_wr.h — lc_wr_check: Elle's rw-register checker for the :wr
 * workload (jepsen.tests.cycle.wr with :consistency-models
 * [:strict-serializable] and, optionally, :wfr-keys), with the version graphs
 * and the dependency graph built on the device.  The caller hands over the
 * transactions and their micro-ops as flat arrays; the library flags every
 * read, infers every key's version graph, builds the ww / wr / rw edges and the
 * real-time predecessor ranges, finds the cycles and gives the verdict.
 * Included by lincheck.h; additive to ABI 5 (callers detect the feature by
 * looking up lc_wr_check).
 *
 * The rules below are a re-derivation of elle.rw-register (elle 0.2.x, as
 * jepsen.tests.cycle.wr calls it).  They are this feature's specification;
 * parity with Elle itself is unpinned.  Elle's
 * :linearizable-keys? inference is lc_wr_check_lin's (lincheck_wrlin.h: a
 * call of its own, these calls take no flag for it); :sequential-keys? is out
 * of scope (the workload this stands for leaves it unset).
 *
 * Positions are history positions, below 2^31 - 1.  Only client ops with
 * :f :txn matter.  Keys and values are int64 (the binding interns anything
 * else); INT64_MIN is no key, and as a value it is nil (LC_WR_NIL).
 *
 *  1. Writers.  Each write mop of any txn makes (key, value) -> (the mop, its
 *     txn, the txn's type, whether it is the txn's last write to that key).
 *     Two writes of one (key, value) are not expressible (Elle requires unique
 *     writes): -EINVAL.
 *  2. Internal.  Walk an OK txn's mops in order, per key.  The expected value
 *     of a key is the value of the latest earlier mop on that key in the txn,
 *     a write or a known read.  A read whose expected value exists and differs
 *     is LC_WR_R_INTERNAL.  A read with no earlier mop on its key in the txn is
 *     the txn's external read of the key (LC_WR_R_EXTERNAL; not an anomaly).
 *     A txn's external write of a key is its last write to it.
 *  3. Every known read of an OK txn with value v != nil:
 *       phantom  (key, v) has no writer (not one of Elle's names, as in
 *                lincheck_append.h; counted, and it makes the history invalid)
 *       G1a      the writer is a FAIL txn
 *       G1b      the writer is another txn and that write is not its last
 *                write to the key.
 *  4. Versions and the version graph of a key.  A key's versions are nil plus
 *     every value written to it or read from it by a known read.  Edges a -> b
 *     with a != b mean "a precedes b":
 *       initial  always: nil -> v for every v written to the key by a node txn
 *                (OK or INFO);
 *       wfr      only with LC_WR_WFR_KEYS: for every OK txn with an external
 *                read a of the key (nil included) and at least one write to
 *                it, a -> b with b the txn's external write.
 *     Where a = b the txn read externally the value it goes on to write: that
 *     edge is a self-loop (rule 6).  The graph is a set: nil -> b arising both
 *     ways is one edge.
 *  5. Lost update, whatever the flag.  A version (key, a) is a lost update iff
 *     at least two OK txns each read it externally and write the key.  It is
 *     flagged on the key (LC_WR_K_LOST_UPDATE), counted per version
 *     (n_lost_update) and makes the history invalid.  With LC_WR_WFR_KEYS it
 *     always coincides with an rw-rw cycle between those txns (each reads a
 *     and the other's write follows a), so the verdict does not depend on
 *     this rule then; without the flag it decides alone.
 *  6. Cyclic versions.  A key whose wfr graph has a cycle, self-loops
 *     counting, is LC_WR_K_CYCLIC.  (nil has no incoming edge, so the initial
 *     edges never close one.)  A cyclic key makes the history invalid and
 *     contributes no ww or rw edges.  Its record's cyc_value is the least
 *     value lying on a version cycle of the key — on one, not merely below
 *     one; LC_WR_NIL for every other key.
 *  7. Nodes and edges.  Graph nodes are the OK and INFO txns.  An edge exists
 *     only when both ends are nodes and differ.
 *       wr, every key: writer(v) -> t for each OK txn t with an external read
 *           of (key, v), v != nil.
 *       For every non-cyclic key and every version edge a -> b of rule 4,
 *       with w = writer(b):
 *       ww: writer(a) -> w;
 *       rw: t -> w for every OK txn t with an external read of (key, a).
 *     The version graph is used as it stands, neither transitively reduced nor
 *     closed: that choice is ours (a nil reader gets an rw edge to every
 *     writer of the key, not only to the first ones).  The edges come back
 *     sorted by (from, to, type, key) and unique.  There is no linear bound on
 *     them: the rw edges number readers(a) x children(a) per version.  So the
 *     caller states its room (out->edge_cap) and sum->n_edges_raw reports the
 *     count before unique: one per external read with a wr edge, and per
 *     version edge of a non-cyclic key one per ww edge and per reader's rw edge.
 *  8. Real time: Elle's frontier walk, transitively reduced.  A -> B iff
 *     comp(A) < inv(B) and no OK txn C has comp(A) < inv(C) and comp(C) <
 *     inv(B).  INFO txns never complete: successors, never predecessors.
 *     Equivalently: with byc the OK txns sorted by comp_pos and m(B) the
 *     largest inv_pos among OK txns with comp < inv(B), B's predecessors are
 *     the contiguous run of byc with m(B) < comp < inv(B).  byc and per txn
 *     [rt_lo, rt_hi) are returned; nothing else is materialised.  Process
 *     edges are not built: a process's ops are sequential, real time has them.
 *     (Rule 6 of lincheck_append.h, and its code.)
 *  9. Cycles: rule 7 of lincheck_append.h, and its code.  SCCs of the whole
 *     graph (ww + wr + rw + rt); each nontrivial SCC gets the first of G0,
 *     G1c, G-single, G2-item and then their -realtime twins that holds inside
 *     it; the first LC_AP_MAX_CYCLES SCCs, in order of their least txn, get
 *     one witness cycle.
 * 10. Verdict.  No OK txn: unknown.  Any flag of rules 2 and 3, any cyclic or
 *     lost-update key, or any nontrivial SCC: invalid.  Otherwise valid.
 */
#ifndef LINCHECK_WR_H
#define LINCHECK_WR_H

#include "lincheck_append.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_WR_OK   LC_AP_OK    /* lc_wr_txn.type */
#define LC_WR_INFO LC_AP_INFO
#define LC_WR_FAIL LC_AP_FAIL
#define LC_WR_WRITE 0          /* lc_wr_mop.f */
#define LC_WR_READ  1
#define LC_WR_NIL INT64_MIN    /* a read's value: nil */
#define LC_WR_WFR_KEYS 1u      /* flags: infer the wfr edges of rule 4 */

/* per-read flags (mop_flags; 0 for writes and ignored reads) */
#define LC_WR_R_INTERNAL 1
#define LC_WR_R_PHANTOM  2
#define LC_WR_R_G1A      4
#define LC_WR_R_G1B      8
#define LC_WR_R_EXTERNAL 16  /* not an anomaly: the txn's external read of its key */
#define LC_WR_R_ANOMALY  15
/* per-txn flags: the OR of its reads' anomaly flags */
/* per-key flags */
#define LC_WR_K_CYCLIC      1
#define LC_WR_K_LOST_UPDATE 2

/* The txn, edge and step records are list-append's: the edge types LC_AP_WW /
 * WR / RW (/ RT in steps) and the classes LC_AP_G0 .. apply. */
typedef struct lc_ap_txn lc_wr_txn;    /* mop_off, inv_pos, comp_pos, type, mop_len; 24 bytes */
typedef struct lc_ap_edge lc_wr_edge;  /* from, to, type, pad, key; 24 bytes */
typedef struct lc_ap_step lc_wr_step;  /* txn, type, key; 16 bytes */

typedef struct lc_wr_mop {
  int64_t key;
  int64_t value;  /* WRITE: the value; READ: the value read, LC_WR_NIL for nil (known reads only) */
  int32_t f;      /* LC_WR_WRITE / LC_WR_READ */
  int32_t known;  /* READ of an OK txn: 1; READ of an INFO or FAIL txn: 0 (ignored); WRITE: 0 */
} lc_wr_mop;      /* 24 bytes */

typedef struct lc_wr_key {
  int64_t key;
  int64_t cyc_value;    /* rule 6; LC_WR_NIL unless LC_WR_K_CYCLIC */
  int32_t flags;        /* LC_WR_K_* */
  int32_t n_writes;     /* write mops on the key, of any txn */
  int32_t n_versions;   /* nil and the distinct values written or read (known reads) */
  int32_t n_ext_reads;  /* external reads of the key (rule 2) */
} lc_wr_key;            /* 32 bytes */

/* Where the results go; every array is the caller's. */
typedef struct lc_wr_out {
  int32_t *mop_flags;     /* n_mops */
  int32_t *txn_flags;     /* n_txns */
  lc_wr_key *keys;        /* room for n_mops; sum->n_keys written, ascending by key */
  lc_wr_edge *edges;      /* room for edge_cap; sum->n_edges written */
  int64_t edge_cap;
  int32_t *byc;           /* room for n_txns; sum->n_ok written */
  int32_t *rt_lo, *rt_hi; /* n_txns: the txn's predecessors are byc[rt_lo .. rt_hi) */
  int32_t *scc;           /* n_txns: the txn's nontrivial SCC (numbered by least txn), else -1 */
  int32_t *scc_class;     /* n_txns: that SCC's class, else -1 */
  lc_wr_step *steps;      /* room for n_txns */
  int64_t *cycle_off;     /* LC_AP_MAX_CYCLES + 1 */
  int32_t *cycle_scc;     /* LC_AP_MAX_CYCLES */
} lc_wr_out;

typedef struct lc_wr_summary {
  int32_t valid;          /* 1 / 0 / -1 (unknown) */
  int32_t pad;
  int64_t n_internal, n_phantom, n_g1a, n_g1b;  /* reads of OK txns */
  int64_t n_cyclic_keys;  /* keys */
  int64_t n_lost_update;  /* versions */
  int64_t n_class[8];     /* nontrivial SCCs per class */
  int64_t n_keys, n_versions /* the keys' n_versions summed */, n_ok, n_nodes, n_edges, n_edges_raw, n_scc,
      n_cycles_returned;
  double  h2d_ms;         /* lc_wr_check: the inputs' copies (HIP events) */
  double  kernel_ms;      /* lc_wr_check: the kernels' two runs, a HIP-event interval each (before and after
                             the synchronisation that brings the status and the rw edges' count) */
  double  host_graph_ms;  /* rule 9, host wall time */
  double  total_ms;       /* host wall time of the call */
} lc_wr_summary;

/*
 * Contract of both functions: txns strictly ascending by inv_pos; positions
 * in [0, 2^31 - 1); type OK or FAIL with comp_pos > inv_pos, or INFO with
 * comp_pos -1; the txns' mop ranges tile [0, n_mops) in txn order, without
 * gaps; f WRITE or READ; no key INT64_MIN; no write's value LC_WR_NIL; known
 * 1 on the reads of OK txns and 0 on every other mop; n_mops below 2^31 - 1;
 * flags LC_WR_WFR_KEYS or 0; edge_cap >= 0.  A violation, or two writes of one
 * (key, value), returns -EINVAL and writes nothing to out or sum.  A call
 * whose unique edges exceed out->edge_cap returns -ENOSPC: nothing is written
 * to out's arrays, and sum (which should not be NULL then) is zero but for
 * n_edges and n_edges_raw, so that the caller can come again with room.
 * n_txns == 0 is legal (unknown).  sum may be NULL; out and its arrays may
 * not.  Positions are taken to be distinct; that is not checked.  A txn's
 * mops are walked per mop of the txn: quadratic in a txn's own length, which
 * the workload keeps to four.
 */

/* The rules on the host, single-threaded: the fallback, the device path's
 * oracle and the probe's baseline.  No GPU needed.  0, -EINVAL, -ENOSPC or
 * -ENOMEM. */
int lc_wr_check_host(const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops, uint32_t flags,
                     const lc_wr_out *out, lc_wr_summary *sum);

/* The same with rules 1-8 on the context's first GPU and rule 9 by the host
 * code over the device's edges.  Every array is host memory; the call is
 * synchronous.  0, -EINVAL, -ENOSPC (texts in lc_last_error, -ENOSPC's naming
 * n_edges and edge_cap; the context stays usable), -E2BIG (more mops or
 * candidate edges than lc_wr_limits allows), -ENOMEM or -EIO.  A call without
 * txns is answered by the host code. */
int lc_wr_check(lc_ctx *ctx, const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops,
                uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum);

/*
 * Limits.  The device call keeps everything resident.  It refuses with
 * -E2BIG a call with more than max_mops mops (the tables have the least power
 * of two of slots that is at least twice the mops, and a slot index is an
 * int32), and one whose candidate edges — a wr / ww slot per mop and the sum
 * of readers(a) x children(a) over the versions of the non-cyclic keys, that
 * is n_edges_raw before the both-ends-are-nodes-and-differ filter — exceed
 * max_edges.  max_edges is default_max_edges (2^27: two buffers of 24-byte
 * records that the select, the sort and the unique pass between them, 6.4
 * GB — a size that was not measured) unless the environment variable
 * LC_WR_MAX_EDGES holds a positive number, read at every call.  max_mops is
 * 2^29, or a positive number below that in LC_WR_MAX_MOPS.  Device memory
 * beside the edges: 100 B per table slot (2 to 4 slots per mop) and about
 * 100 B per mop; the largest measured call held 2.5 x 10^6 mops and 2.1 x
 * 10^6 candidate edges.  (The host function takes any
 * n_mops below 2^31 - 1.)  Host-only.
 */
typedef struct lc_wr_limit_info {
  int64_t max_edges;
  int64_t default_max_edges;
  int64_t max_position;   /* positions are below this */
  int64_t max_mops;       /* lc_wr_check: n_mops is at most this */
} lc_wr_limit_info;

int lc_wr_limits(lc_wr_limit_info *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_WR_H */
