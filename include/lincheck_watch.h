/*
 * lincheck_watch.h — lc_watch_check: the :watch workload's log-convergence
 * checker (the checker of jepsen.etcd's watch.clj: every thread's watch log
 * must be the same sequence), with the logs hashed, compared and diffed on the
 * device.  The caller hands over the threads and their concatenated logs as
 * flat arrays; the library groups equal logs into classes, picks the canonical
 * log, gives every differing thread its edit distance and, up to a cap, its
 * edit script against the canonical log, and gives the verdict.  Included by
 * lincheck.h; additive to ABI 5 (callers detect the feature by looking up
 * lc_watch_check).
 *
 * The rules below re-derive the checker of watch.clj and what is known of
 * clj-diff's edit distance and diff.  They are this feature's specification.
 * No JVM, jepsen or clj-diff was at hand when they were written: parity with
 * them is unpinned, as for the other side checkers.
 *
 *  1. Threads.  Only op maps with :type :ok and :f :watch or :final-watch
 *     matter; a :final-watch that carries :error [:converge-timeout] is still
 *     :ok and counts.  An op's thread is process mod concurrency.  A thread's
 *     log is the concatenation, in history order, of its ops' :value :log; its
 *     revision is the maximum of its ops' :value :revision, and 0.  A thread
 *     without such an op does not exist.  (The encoder applies this rule; the
 *     functions below take threads as flat arrays.)
 *  2. Classes.  Two threads are in one class iff their logs are equal, element
 *     for element.  A class's representative is its thread with the lowest
 *     position in the input array.
 *  3. Canonical log.  If some class has more than one thread, the log of the
 *     largest class; otherwise the longest log.  Ties go to the representative
 *     with the lowest input position.  (The reference breaks ties by hash-map
 *     iteration order: this tie-break is ours.  The verdict does not depend on
 *     it; which log is called canonical, and hence the deltas, do.)
 *  4. Deltas.  For every thread whose log B differs from the canonical log A:
 *     p is the longest common prefix of A and B; s is the longest common
 *     suffix of A[p:] and B[p:] (so the two never overlap: p + s <= min(len A,
 *     len B)); a = A[p : len A - s] and b = B[p : len B - s] are the middles;
 *     edit_distance = len a + len b - 2 LCS(a, b), insertions plus deletions.
 *     It is unique.
 *  5. Edit script.  When edit_distance <= max_d, the delta carries the script
 *     that Myers' greedy forward algorithm gives on (a, b), with this choice
 *     rule.  Forward: V_{-1}[1] = 0; round d visits the diagonals k = -d,
 *     -d + 2, .., d; on diagonal k the path comes down (an insertion, x =
 *     V_{d-1}[k+1]) if k == -d, or if k != d and V_{d-1}[k-1] < V_{d-1}[k+1];
 *     otherwise it comes right (a deletion, x = V_{d-1}[k-1] + 1); then the
 *     snake is followed while x < len a, x - k < len b and a[x] == b[x-k].
 *     The first d at which diagonal len a - len b reaches x >= len a is the
 *     distance D.  The backtrack applies the same test to the saved V_{d-1}
 *     from d = D down to 1.  The script is in path order, each edit with its
 *     position in A: a deletion is (LC_WT_DELETE, at, A[at]); an insertion is
 *     (LC_WT_INSERT, at, value), value going in before A[at], 0 <= at <=
 *     len A.  The script has exactly D entries, `at` never decreases, and
 *     applying it to A gives B.
 *  6. Above the cap.  A delta with edit_distance > max_d keeps its exact
 *     distance and has no script: LC_WT_NO_SCRIPT, script_len 0.  (The host
 *     code computes the distance by the same forward pass without a trace, in
 *     O(D) memory.)
 *  7. Order of deltas: descending edit_distance, then ascending input
 *     position.  (The reference's tie order is a map's: this one is ours.)
 *  8. Nonmonotonic errors: the op maps, of any type, whose :error is a
 *     sequence starting with :nonmonotonic-watch.  The encoder counts them;
 *     the functions take the count.
 *  9. Verdict, in this order: any nonmonotonic error: invalid; else threads
 *     with unequal revisions: unknown; else any delta: invalid; else valid.
 *     No threads at all: unknown (the reference's (apply = []) throws, and
 *     check-safe turns that into :unknown).
 * 10. Refusals (-EINVAL, nothing written): a log of 2^31 - 1 entries or more;
 *     a thread id repeated; a negative off or len, or a log that runs past
 *     n_values; an unknown flag (none is defined: flags must be 0).
 */
#ifndef LINCHECK_WATCH_H
#define LINCHECK_WATCH_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_WT_DELETE 0           /* lc_wt_edit.op */
#define LC_WT_INSERT 1
#define LC_WT_NO_SCRIPT 1u       /* lc_wt_delta.flags: rule 6 */
#define LC_WT_MAX_D_LIMIT 4096   /* max_d is at most this (a V row lives in the LDS) */

typedef struct lc_wt_thread {
  int64_t off, len;   /* the log is values[off .. off + len) */
  int64_t revision;
  int64_t thread;     /* rule 1's thread id: distinct */
} lc_wt_thread;       /* 32 bytes */

typedef struct lc_wt_delta {
  int32_t thread;         /* the thread's position in the input array */
  uint32_t flags;         /* LC_WT_NO_SCRIPT or 0 */
  int64_t edit_distance;
  int64_t prefix, suffix; /* rule 4's p and s */
  int64_t script_off;     /* into edits; script_len is edit_distance, or 0 with LC_WT_NO_SCRIPT */
  int64_t script_len;
} lc_wt_delta;            /* 48 bytes */

typedef struct lc_wt_edit {
  int64_t at;     /* position in the canonical log */
  int64_t value;  /* the element deleted or inserted */
  int32_t op;     /* LC_WT_DELETE / LC_WT_INSERT */
  int32_t pad;    /* 0 */
} lc_wt_edit;     /* 24 bytes */

/* Where the results go; every array is the caller's. */
typedef struct lc_wt_out {
  int32_t *cls;         /* n_threads: the input position of the thread's class representative */
  int64_t *distance;    /* n_threads: edit distance to the canonical log, 0 when equal to it */
  lc_wt_delta *deltas;  /* room for n_threads; sum->n_deltas written, in rule 7's order */
  lc_wt_edit *edits;    /* room for edit_cap; sum->n_edits written, the scripts in the deltas' order */
  int64_t edit_cap;
} lc_wt_out;

typedef struct lc_wt_summary {
  int32_t valid;            /* 1 / 0 / -1 (unknown) */
  int32_t canonical;        /* input position of the canonical thread, -1 without threads */
  int64_t canonical_size;   /* threads in its class */
  int64_t n_threads, n_classes, n_deltas, n_edits;
  int64_t n_no_script;      /* deltas above the cap (rule 6) */
  int64_t n_by_host;        /* lc_watch_check: deltas whose distance the host code finished; host: 0 */
  int64_t n_collisions;     /* exact compares of two logs of one length and one hash that were unequal */
  int32_t revisions_equal;  /* 1 / 0 */
  int32_t pad;
  double h2d_ms;            /* lc_watch_check: the inputs' copies (HIP events) */
  double kernel_ms;         /* lc_watch_check: the kernels' runs, a HIP-event interval each */
  double total_ms;          /* host wall time of the call */
} lc_wt_summary;

/*
 * Contract of both functions: rule 10; n_values >= 0; 0 <= n_threads < 2^31 -
 * 1; n_nonmonotonic >= 0; edit_cap >= 0.  A violation returns
 * -EINVAL and writes nothing to out or sum.  Logs may overlap or leave gaps in
 * values.  A call whose scripts exceed out->edit_cap returns -ENOSPC: nothing
 * is written to out's arrays, and sum (which should not be NULL then) is zero
 * but for n_edits, so that the caller can come again with room.  n_threads ==
 * 0 is legal (unknown).  sum may be NULL; out and its arrays may not.
 */

/* The rules on the host, single-threaded: the fallback, the device path's
 * oracle and the probe's baseline.  No GPU needed.  0, -EINVAL, -ENOSPC or
 * -ENOMEM. */
int lc_watch_check_host(const lc_wt_thread *threads, int64_t n_threads, const int64_t *values, int64_t n_values,
                        int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out, lc_wt_summary *sum);

/* The same with the hashes, the compares, Myers' forward pass and the
 * backtrack on the context's first GPU.  Every array is host memory; the call
 * is synchronous.  0, -EINVAL, -ENOSPC (texts in lc_last_error; the context
 * stays usable), -E2BIG (a log longer than lc_watch_limits' max_device_len),
 * -ENOMEM or -EIO.  A call with fewer than two threads is answered by the
 * host code. */
int lc_watch_check(lc_ctx *ctx, const lc_wt_thread *threads, int64_t n_threads, const int64_t *values,
                   int64_t n_values, int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out,
                   lc_wt_summary *sum);

/*
 * Limits, and the environment's overrides, read at every call.  max_d is rule
 * 5's cap: default_max_d (4,096) unless LC_WT_MAX_D holds a number in [0,
 * LC_WT_MAX_D_LIMIT] (a larger one counts as the limit).  trace_bytes bounds
 * the forward pass's traces on the device — a differing thread's trace has
 * (c + 1)(c + 2) / 2 int32 entries with c = min(max_d, len a + len b) — and
 * the threads are taken in batches whose traces fit it (a batch has at least
 * one thread, whatever the budget): default_trace_bytes (1 GiB) unless
 * LC_WT_TRACE_BYTES holds a positive number.  Where LC_WT_HASH_MASK holds a
 * number (decimal or 0x..), that 64-bit number is ANDed onto every log's
 * 128-bit hash, so the high word is gone and hash_mask is what is left of the
 * low one (mask 1: two hashes in all); unset, hash_mask is all ones and
 * nothing is masked.  It is a test's way to force collisions; the results do
 * not depend on it but for n_collisions.  max_len: logs are shorter than this
 * (rule 10).  max_device_len: lc_watch_check's own bound on a log's length
 * (positions and the overshoot of a pass are int32 there).  Host-only.
 */
typedef struct lc_wt_limit_info {
  int64_t max_d, default_max_d;
  int64_t trace_bytes, default_trace_bytes;
  int64_t max_len;
  int64_t max_device_len;
  uint64_t hash_mask;
} lc_wt_limit_info;

int lc_watch_limits(lc_wt_limit_info *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_WATCH_H */
