/*
 * lincheck_perf.h — lc_perf_stats: the :stats and :perf keys of the composed
 * checker (jepsen.checker/stats and the data behind jepsen.checker.perf's
 * three graphs: the latency points, the latency quantiles per time bucket and
 * the completion rate per time bucket), computed on the device from one
 * 16-byte record per op map.  Included by lincheck.h; additive to ABI 5
 * (callers detect the feature by looking up lc_perf_stats).
 *
 * The rules below re-derive jepsen.checker/stats and jepsen.checker.perf
 * (jepsen 0.3.x) from memory.  They are this feature's specification.  No JVM
 * and no jepsen source was at hand when they were written: parity with jepsen
 * itself is unpinned, as for the other side checkers.
 *
 *  1. Only client events count (process >= 0).  Every other record (a nemesis
 *     op) occupies its position and is otherwise ignored, but for rule 8's
 *     test of its time and type.
 *  2. Stats.  Per f, over client events whose type is not INVOKE: count, ok,
 *     fail, info.  An f with count > 0 is valid iff ok > 0; an f with count ==
 *     0 is absent.  valid is 1 iff every present f is valid (also when none is
 *     present).  The totals over all f are returned as well.
 *  3. Pairing is rule 2 of lincheck_events.h with "process" in place of "(key,
 *     process)": within one process's subsequence of the history, an invoke is
 *     paired with the event that immediately follows it iff that event is a
 *     completion.  An invoke followed by an invoke or by nothing is pending
 *     (n_pending).  A completion whose predecessor is not an invoke is ignored
 *     for latencies (n_ignored_completions) but still counts in rules 2 and 5.
 *     A pair whose completion's f differs from the invoke's is counted
 *     (n_mismatched_f); it stands, with the invoke's f.
 *  4. Latency.  A pair's latency is completion.time - invoke.time, signed: a
 *     clock that stepped back gives a negative one, which is kept.
 *  5. Rate.  Every client non-invoke event adds 1 to rate[f][type - 1][time /
 *     rate_dt_ns] (integer division; f and time are the completion's own).
 *     Dividing by dt and the buckets' midpoints are the binding's business.
 *  6. Quantiles.  A pair puts its latency into the group (invoke.f,
 *     invoke.time / quant_dt_ns), whatever the completion's type.  For a group
 *     of n latencies sorted ascending s, quantile q is s[min(n - 1,
 *     (int64)floor(q * (double)n))]: one IEEE double multiply, written so that
 *     host and device evaluate the same expression (no fused form).
 *     quant_n[f][b] = n.  An empty group's entries are INT64_MIN.
 *  7. Bucket counts.  t_max is the largest time of a client event, 0 if there
 *     is none.  The rate table has t_max / rate_dt_ns + 1 buckets per row, the
 *     quantile tables t_max / quant_dt_ns + 1.
 *  8. Refusals.  -EINVAL, text in lc_last_error, nothing written, the context
 *     still usable: a record (client or not) with a negative time or a type
 *     above 3; a client event's f >= n_f; n_events >= 2^31 (or negative); n_f
 *     < 1; n_q outside [0, 8]; a q outside [0, 1] or NaN; a dt of 0 or less;
 *     a NULL array that may not be NULL.  -E2BIG: n_f above
 *     lc_perf_stats_limits' max_f, or a table of rule 7's counts (n_f * 3 *
 *     n_rate_buckets; n_f * n_quant_buckets * max(n_q, 1)) above
 *     max_table_entries.  -ENOSPC: rate_cap or quant_cap below rule 7's
 *     counts; the summary (which should not be NULL then) is zero but for
 *     n_events, n_client, t_max, n_rate_buckets and n_quant_buckets, so that
 *     the caller sizes its tables and calls again (lc_wr_check's edge_cap
 *     convention).  The checks are made in this order.
 */
#ifndef LINCHECK_PERF_H
#define LINCHECK_PERF_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_PS_MAX_Q 8
#define LC_PS_NONE INT64_MIN /* latency_ns of an unpaired position; quant of an empty group */

/* One op map of the history; its position in the array is the history position. */
typedef struct lc_ps_event {
  int64_t time;    /* the op map's :time, ns, >= 0 */
  int32_t process; /* >= 0: a client's :process; < 0: not a client op (nemesis): ignored, occupies a position */
  uint16_t f;      /* dense id of :f, 0 .. n_f-1, interned by the caller */
  uint8_t type;    /* LC_EV_INVOKE / OK / FAIL / INFO (lincheck_events.h's values) */
  uint8_t pad;
} lc_ps_event;     /* 16 bytes */

typedef struct lc_ps_params {
  int32_t n_f;
  int32_t n_q;              /* 0 .. LC_PS_MAX_Q */
  double q[LC_PS_MAX_Q];    /* the first n_q count, each in [0, 1] */
  int64_t rate_dt_ns;       /* rule 5's bucket, > 0 */
  int64_t quant_dt_ns;      /* rule 6's bucket, > 0 */
} lc_ps_params;

/* Where the results go; every array is the caller's host memory. */
typedef struct lc_ps_out {
  int64_t *by_f;        /* n_f x {count, ok, fail, info} */
  int32_t *comp_pos;    /* n_events: a paired invoke's completion position, else -1.  comp_pos and */
  int64_t *latency_ns;  /* n_events: its latency, else LC_PS_NONE.  ... latency_ns may both be NULL */
  int64_t *rate;        /* [n_f][3][rate_cap] */
  int64_t rate_cap;
  int64_t *quant;       /* [n_f][quant_cap][n_q]; may be NULL when n_q == 0 */
  int64_t *quant_n;     /* [n_f][quant_cap] */
  int64_t quant_cap;
} lc_ps_out;
/* Of a table's row, the buckets from rule 7's count up to the cap are written
 * too: 0 in rate and quant_n, LC_PS_NONE in quant. */

typedef struct lc_ps_summary {
  int32_t valid;        /* 1 / 0 (rule 2) */
  int32_t pad;
  int64_t n_events, n_client, n_pairs, n_pending, n_ignored_completions, n_mismatched_f;
  int64_t count, ok, fail, info;  /* rule 2's totals */
  int64_t t_max, n_rate_buckets, n_quant_buckets;
  double h2d_ms;        /* lc_perf_stats: the records' copy (HIP events) */
  double kernel_ms;     /* lc_perf_stats: the kernels and sorts (HIP events) */
  double total_ms;      /* host wall time of the call */
} lc_ps_summary;

/* The rules on the host, single-threaded: the fallback, the device path's
 * oracle and the probe's baseline.  No GPU needed.  0, -EINVAL, -E2BIG,
 * -ENOSPC or -ENOMEM.  sum may be NULL. */
int lc_perf_stats_host(const lc_ps_event *ev, int64_t n_events, const lc_ps_params *params, const lc_ps_out *out,
                       lc_ps_summary *sum);

/* The same on the context's first GPU.  Every array is host memory; the call
 * is synchronous.  The codes above (texts in lc_last_error; the context stays
 * usable) or -EIO.  A call with fewer than two events or without client
 * events is answered by the host code. */
int lc_perf_stats(lc_ctx *ctx, const lc_ps_event *ev, int64_t n_events, const lc_ps_params *params,
                  const lc_ps_out *out, lc_ps_summary *sum);

/*
 * Limits, and the kernels' geometry for those who plant inputs at its edges.
 * The pair pass counts rules 5 and 6 in one table of n_f * 3 * n_rate_buckets
 * + n_f * n_quant_buckets entries; up to lds_entries it is a histogram in each
 * workgroup's LDS, flushed with atomics at the workgroup's end, above it the
 * counts go to global memory directly.  lds_entries is default_lds_entries
 * unless the environment variable LC_PS_LDS_ENTRIES holds a number in [0,
 * default_lds_entries], read at every call (0: always global memory).  The
 * results do not depend on it.  Host-only.
 */
typedef struct lc_ps_limit_info {
  int64_t max_f;              /* n_f is at most this */
  int64_t max_table_entries;  /* rule 8's bound on each table */
  int64_t lds_entries, default_lds_entries;
  int32_t wave;               /* 64 */
  int32_t block;              /* threads of a workgroup, in every kernel */
  int32_t chunk;              /* process-sorted slots a workgroup of the pair pass takes at a time */
  int32_t max_grid;           /* workgroups of a launch; the rest is a grid stride */
} lc_ps_limit_info;

int lc_perf_stats_limits(lc_ps_limit_info *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_PERF_H */
