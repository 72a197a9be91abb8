/*
 * lincheck_setfull.h — lc_set_full: jepsen.checker/set-full on the device.
 * The caller hands over the adds, the :ok reads and the reads' payloads as
 * flat arrays; the library decides for every element whether it is stable,
 * lost or never read, with jepsen's latencies, and gives the verdict.
 * Included by lincheck.h; additive to ABI 5 (callers detect the feature by
 * looking up lc_set_full).
 *
 * The rules below are a re-derivation of jepsen.checker/set-full (jepsen
 * 0.3.x).  They are this feature's specification; parity with jepsen itself
 * is unpinned.
 *
 * Positions are history positions (the order of the op maps); times are the
 * op maps' :time in ns.  Only client ops with :f :add or :f :read matter.
 *
 *  1. Elements.  Every :add invoke creates an element (its :value), whatever
 *     its completion.  An :add :ok of that value gives the element ok_pos /
 *     ok_time; :fail, :info or no completion give nothing (ok_pos = -1).
 *  2. Reads.  An :ok read by process p is paired with p's pending read invoke:
 *     p's latest :read invoke before it with no :read :fail of p in between
 *     (:info leaves the invoke pending; an :ok does not clear it).  The read
 *     is (inv_pos, inv_time, ok_pos, ok_time, payload).  Only :ok reads count.
 *  3. Eligibility.  Read r concerns element e iff ok_pos(r) > inv_pos(e): the
 *     element existed when the read completed.  r then observes e if e occurs
 *     in r's payload, and misses it otherwise.  A payload entry that names no
 *     element, or an element r does not concern, is ignored and counted
 *     (n_phantom).
 *  4. Per element: first_seen = the observing read with the least ok_pos;
 *     known = whichever of the add's :ok and first_seen's :ok has the smaller
 *     position, or none; last_present = the largest inv_pos over observing
 *     reads; last_absent = the largest inv_pos over missing reads; each with
 *     that op's time, each -1 when there is none.  (Among reads of one
 *     inv_pos the one with the largest ok_pos gives the time.)
 *  5. Outcome (-1 compares below everything):
 *       stable  iff last_present >= 0 && last_absent < last_present
 *       lost    iff known_pos >= 0 && last_absent >= 0 &&
 *                   last_present < last_absent && known_pos < last_absent
 *       never-read otherwise.  Stable and lost exclude each other.
 *  6. Latencies.  stable_time = time(last_absent) + 1 if there is a
 *     last_absent, else 0; lost_time = time(last_present) + 1 if there is a
 *     last_present, else 0; a latency in ms is max(0, t - known_time) /
 *     1,000,000, truncated; -1 where the outcome does not define it (stable:
 *     stable_latency_ms, lost: lost_latency_ms).  An element is stale iff it
 *     is stable with stable_latency_ms > 0.
 *  7. Duplicates.  An element occurring n > 1 times in one concerning read's
 *     payload is duplicated; dup_max is the largest such n, 0 if none.
 *  8. Verdict.  Any duplicated element: invalid.  Else any lost: invalid.
 *     Else no stable element: unknown.  Else linearizable and any stale:
 *     invalid.  Else valid.
 *  9. Differences from jepsen, which would throw or silently rebind (it writes
 *     no such history): an add completion of a value with no earlier add
 *     invoke is ignored; an :ok read with no pending invoke is ignored and
 *     counted; two add invokes of one value are not expressible (-EINVAL); an
 *     op map without :time is not expressible.  (Rules 1, 2 and 9 are applied
 *     by whoever makes the arrays: jepsen/etcd_amd/setfull.py's encode.)
 */
#ifndef LINCHECK_SETFULL_H
#define LINCHECK_SETFULL_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_SF_NEVER_READ 0
#define LC_SF_STABLE     1
#define LC_SF_LOST       2
#define LC_SF_STALE      1  /* lc_sf_element.flags */
#define LC_SF_DUPLICATED 2

/* One element: its add invoke and, where there is one, the add's :ok. */
typedef struct lc_sf_add {
  int64_t value;    /* the element; INT64_MIN is reserved */
  int64_t ok_time;  /* ignored when ok_pos is -1 */
  int32_t inv_pos;
  int32_t ok_pos;   /* -1: no :ok */
} lc_sf_add;        /* 24 bytes */

/* One :ok read; its payload is read_values[off .. off + len). */
typedef struct lc_sf_read {
  int64_t inv_time, ok_time, off;
  int32_t inv_pos, ok_pos, len, pad;
} lc_sf_read;       /* 40 bytes */

typedef struct lc_sf_element {
  int32_t outcome;       /* LC_SF_NEVER_READ / STABLE / LOST */
  int32_t flags;         /* LC_SF_STALE | LC_SF_DUPLICATED */
  int32_t known_pos;     /* positions; -1: none */
  int32_t last_present;
  int32_t last_absent;
  int32_t dup_max;
  int64_t stable_latency_ms, lost_latency_ms;  /* -1: not defined */
} lc_sf_element;    /* 40 bytes */

typedef struct lc_sf_summary {
  int32_t valid;         /* 1 / 0 / -1 (unknown) */
  int32_t linearizable;  /* as passed */
  int64_t n_elements, n_stable, n_lost, n_never_read, n_stale, n_duplicated;
  int64_t n_phantom;     /* payload entries ignored by rule 3 */
  int64_t n_tiles;       /* lc_set_full: element ranges processed (0 from the host function) */
  double  h2d_ms;        /* lc_set_full: the inputs' copies (HIP events) */
  double  kernel_ms;     /* lc_set_full: every kernel of the call (HIP events) */
  double  total_ms;      /* host wall time of the call */
} lc_sf_summary;

/*
 * Contract of both functions: adds strictly ascending by inv_pos; reads
 * strictly ascending by ok_pos, each with inv_pos < ok_pos; for each read
 * 0 <= off, 0 <= len, off + len <= n_values (ranges may overlap); positions
 * in [0, 2^31 - 1), an add's ok_pos -1 or above its inv_pos; no add value
 * INT64_MIN.  A violation, or two adds of one value, returns -EINVAL and
 * writes nothing to out or sum.  out has n_adds entries: out[e] belongs to
 * adds[e].  n_adds == 0 or n_reads == 0 are legal (every element is never
 * read, the verdict is unknown).  sum may be NULL.
 */

/* The rules on the host, single-threaded: the fallback, and the device
 * path's oracle.  No GPU needed.  Returns 0, -EINVAL or -ENOMEM. */
int lc_set_full_host(const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads, int64_t n_reads,
                     const int64_t *read_values, int64_t n_values, int32_t linearizable,
                     lc_sf_element *out, lc_sf_summary *sum);

/* The same on the context's first GPU.  Every array is host memory; the call
 * is synchronous.  Returns 0, -EINVAL (text in lc_last_error; the context
 * stays usable), -ENOMEM or -EIO.  A call without adds or without reads has
 * nothing for the device to do and is answered by the host code. */
int lc_set_full(lc_ctx *ctx, const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads,
                int64_t n_reads, const int64_t *read_values, int64_t n_values, int32_t linearizable,
                lc_sf_element *out, lc_sf_summary *sum);

/*
 * Limits.  The device keeps one bit per (element, read); a bitmap above
 * tile_bytes is processed in element ranges of max(1, tile_bytes / (4 *
 * ceil(n_reads / 32))) elements, each a pass of its own over the payload
 * (lc_sf_summary.n_tiles; results do not depend on it).  tile_bytes
 * is default_tile_bytes unless the environment variable LC_SF_TILE_BYTES
 * holds a positive number, read at every call.  Host-only.
 */
typedef struct lc_sf_limit_info {
  int64_t tile_bytes;
  int64_t default_tile_bytes;
  int64_t max_position;   /* positions are below this */
  int64_t value_bytes;    /* one payload entry */
} lc_sf_limit_info;

int lc_set_full_limits(lc_sf_limit_info *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_SETFULL_H */
