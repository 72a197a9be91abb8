/*
 * lincheck_events.h — lc_check_events: jepsen.independent's per-key split and
 * knossos's history completion on the device.  The caller hands over the
 * history as one flat array of 24-byte event records, one per op map in
 * history order; the library splits it by key, pairs invokes with their
 * completions, packs lc_op32 records and checks them, all on the GPU.
 * Included by lincheck.h; additive to ABI 5 (callers detect the feature by
 * looking up lc_check_events).
 */
#ifndef LINCHECK_EVENTS_H
#define LINCHECK_EVENTS_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_EV_SKIP   (-1)  /* lc_event.key: not a client op (ignored; it occupies a position) */
#define LC_EV_INVOKE 0
#define LC_EV_OK     1
#define LC_EV_FAIL   2
#define LC_EV_INFO   3
#define LC_EV_F_UNKNOWN 3  /* fkw: an :f the model has no step for */

/*
 * One op map of the history, 24 bytes.  The event's position in the array is
 * its history position.
 *
 *  key      dense key number 0 .. n_keys-1 (which key gets which number is the
 *           caller's business), or LC_EV_SKIP
 *  process  the op's :process (any int32)
 *  tf       type | fkw << 8 | bad_shape << 16.  type: LC_EV_INVOKE / OK / FAIL
 *           / INFO; fkw: LC_F_READ / WRITE / CAS or LC_EV_F_UNKNOWN; bad_shape:
 *           this op map's value does not have the model's shape
 *  value, expected, version
 *           this op map's own value, encoded as lc_op32 encodes it (LC_NIL =
 *           -1); ids are the caller's and pass through unchanged
 *
 * Rules (they restate history.py's split_by_key / complete / _record):
 *  1. Key k's subhistory is the events with key == k, in position order.
 *  2. Within one (key, process) subsequence an invoke is paired with the event
 *     that immediately follows it iff that event is a completion (OK / FAIL /
 *     INFO).  An invoke followed by another invoke, or by nothing, stays
 *     pending forever; a completion whose predecessor is not an invoke is
 *     ignored.
 *  3. A FAIL pair produces no record.  An OK pair gives ret = the completion's
 *     position, and value / expected / version / bad_shape come from the
 *     completion.  INFO, or no completion, gives ret = LC_INF32 and the
 *     invoke's fields.
 *  4. The record's f is the invoke's fkw; it is 3, with all three fields
 *     LC_NIL, when that fkw is 3, when the source event's bad_shape bit is
 *     set, or when an OK completion's fkw differs from the invoke's.  (The
 *     last is the one difference from history.py, which would take the
 *     invoke's :f with the completion's value; Jepsen writes no such history.)
 *  5. call / ret are relative to key_base[k], the position of the key's first
 *     record's invoke (lc_pack32's rule; 0 for a key without records).
 *     Records are ordered by call.
 *  6. A key without records is an empty key.
 *  7. A key outside [-1, n_keys), a type above 3, or n_events >= 2^31: -EINVAL
 *     (the context stays usable).
 *  8. A client op that belongs to every key (a non-tuple value under
 *     jepsen.independent) is not expressible; such a history takes the host
 *     path.
 */
typedef struct lc_event {
  int32_t  key;
  int32_t  process;
  uint32_t tf;
  int32_t  value, expected, version;
} lc_event;

/*
 * The packed records, in caller-allocated host memory.  cap: the capacity of
 * ops32 and completion in records; at least the number of INVOKE events of
 * the call (-EINVAL otherwise).  key_off: n_keys + 1 entries, key_off[0] = 0;
 * key_base: n_keys entries.  completion[r]: the position of record r's
 * completion event (OK or INFO), or -1 when it has none.  n_ops is written.
 */
typedef struct lc_events_out {
  lc_op32 *ops32;
  int32_t *completion;
  int64_t *key_off;
  int64_t *key_base;
  int64_t cap;
  int64_t n_ops;
} lc_events_out;

/* The rules on the host: the fallback, and the device path's oracle.  No GPU
 * needed.  Returns 0, -EINVAL (null buffers, rule 7, cap too small) or
 * -ENOMEM. */
int lc_events_pack_host(const lc_event *ev, int64_t n_events, int64_t n_keys, lc_events_out *out);

/* Split and completion on the context's first GPU; the records are copied
 * back into `out`.  ev is host memory; synchronous.  Returns 0, -EINVAL (text
 * in lc_last_error), -ENOMEM or -EIO. */
int lc_events_pack(lc_ctx *ctx, const lc_event *ev, int64_t n_events, int64_t n_keys,
                   lc_events_out *out);

/*
 * Split, completion and check on the context's first GPU: the packed records
 * stay in device memory and are decided as lc_check_device32 decides them, so
 * every tier and every LC_FLAG_* applies; out[k] is what lc_check32 returns
 * for the records lc_events_pack_host makes (fail_prefix_end is a position).
 * ev, out, aux's arrays and packed are host memory; aux's per-record members
 * (witness, certificate_set) are indexed like the packed records and hold at
 * least as many entries as the call has INVOKE events (n_events always
 * suffices).  aux and packed may be NULL.  Synchronous.
 */
int lc_check_events(lc_ctx *ctx, const lc_event *ev, int64_t n_events, int64_t n_keys,
                    const lc_opts *opts, lc_key_result *out, const lc_aux *aux,
                    lc_events_out *packed);

/* The most recent lc_events_pack / lc_check_events call. */
typedef struct lc_events_stats {
  double  h2d_ms;       /* the events' host-to-device copy (HIP events) */
  double  split_ms;     /* the split / completion / packing kernels (HIP events) */
  double  check_ms;     /* lc_check_events: host wall time of the check that follows */
  double  total_ms;     /* host wall time of the call */
  int64_t n_events;
  int64_t n_client;     /* events with key >= 0 */
  int64_t n_ops;        /* records packed */
  int64_t n_fail_pairs; /* invokes dropped with their FAIL completion */
  int64_t n_ignored_completions; /* completions whose predecessor is not an invoke */
  int64_t n_big_keys;   /* keys larger than max_lds_events: sorted in global memory */
} lc_events_stats;

int lc_last_events_stats(lc_ctx *ctx, lc_events_stats *out);

/* Limits of the per-key kernel's in-LDS paths: a key of more events has its
 * positions sorted in global memory; a key with more distinct processes keeps
 * the further ones in a global-memory table.  Both are exact.  Host-only. */
typedef struct lc_events_limit_info {
  int64_t max_lds_events;
  int64_t lds_process_capacity;
} lc_events_limit_info;

int lc_events_limits(lc_events_limit_info *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_EVENTS_H */
