/*
 * lincheck_counted.h — the counted-class search tier of lc_check
 * (LC_FLAG_COUNTED_CLASSES, include/lincheck.h): its layout rule as a
 * host-only planner, and its statistics.  Included by lincheck.h; additive
 * to ABI 5 (callers detect the feature by looking up lc_counted_plan).
 */
#ifndef LINCHECK_COUNTED_H
#define LINCHECK_COUNTED_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * LC_FLAG_COUNTED_CLASSES: the class table the counted tier uses for one key
 * (its n records).  Crashed writes/CAS (ret == LC_INF) with equal (f, value,
 * expected, version) are interchangeable, and deadline order linearizes them
 * in call order, so a configuration holds one count per class instead of one
 * window slot per crashed op.  The layout of a configuration's 64-bit mask:
 *
 *   classes     the distinct (f, value, expected, version) among the crashed
 *               writes/CAS, in order of first call (a version outside
 *               [-1, 2^31-2] reads as 2^31-2, as on the device)
 *   width[c]    floor(log2(members[c])) + 1 bits: the field holds the absolute
 *               number of the class's members linearized
 *   shift[c]    fields are packed from bit 63 downward in class order:
 *               shift[c] = 64 - (width[0] + ... + width[c])
 *   field_bits  the sum of the widths
 *   slots       min(64 - field_bits, 64 - n_classes): the low bits of the
 *               mask, one-bit window slots for every other open op (:ok ops,
 *               constraining reads); class c also owns wavefront lane 63 - c
 *   fits        n_classes <= LC_COUNTED_MAX_CLASSES && slots >= 1
 *
 * A key that does not fit, or that has more than `slots` other ops open at
 * once, stays :unknown with LC_REASON_WINDOW_OVERFLOW.  n_classes, field_bits
 * and slots count every class; the per-class arrays hold the first
 * LC_COUNTED_MAX_CLASSES.  Host-only; usable without a GPU.  Returns 0 or
 * -EINVAL (null buffers, n < 0).
 */
#define LC_COUNTED_MAX_CLASSES 16
typedef struct lc_counted_layout {
  int32_t n_classes;
  int32_t field_bits;
  int32_t slots;
  int32_t fits;
  int64_t f[LC_COUNTED_MAX_CLASSES];
  int64_t value[LC_COUNTED_MAX_CLASSES];
  int64_t expected[LC_COUNTED_MAX_CLASSES];
  int64_t version[LC_COUNTED_MAX_CLASSES];
  int64_t members[LC_COUNTED_MAX_CLASSES];
  int32_t shift[LC_COUNTED_MAX_CLASSES];
  int32_t width[LC_COUNTED_MAX_CLASSES];
} lc_counted_layout;

int lc_counted_plan(const lc_op *ops, int64_t n, lc_counted_layout *out);

/* The counted tier's share of the most recent call, summed over its devices. */
typedef struct lc_counted_stats {
  int64_t n_keys;     /* keys the tier took (left at LC_REASON_WINDOW_OVERFLOW by the tiers) */
  int64_t n_decided;  /* ... that it left with a verdict other than :unknown */
  int64_t n_unfit;    /* ... that it returned untouched as LC_REASON_WINDOW_OVERFLOW */
  double kernel_ms;   /* device time of the tier (HIP events) */
} lc_counted_stats;

int lc_last_counted_stats(lc_ctx *ctx, lc_counted_stats *out);

/*
 * knossos's :configs from the counted search, batched: lc_check_frontiers
 * (lincheck_fx.h) for keys with more ops open than its window holds, and with
 * pending lists of any length.  For every key, one wavefront runs the counted
 * tier's search up to the :ok return of record stop_op[k] (key-relative; an
 * invalid key's fail_op) and returns the frontier that return expands, over
 * the tier's ladder of set capacities.  Additive to ABI 5 (callers look the
 * symbol up); LC_FLAG_COUNTED_CLASSES is not needed, this call always counts.
 * Like lc_check_frontiers it runs on the context's first GPU over the
 * context's scratch buffers, and takes max_configs_per_key / time_budget_ms /
 * init_* from opts.
 *
 *   out[k * max_per_key + j]   configuration j of key k, j < n_out[k]
 *   pending[pending_at ...]    its n_pending pending ops: key-relative record
 *                              indices, sorted; pending_at = max_per_key *
 *                              (key_off[k] - key_off[0]) + j * n_k with n_k the
 *                              key's records (a pending set is never larger)
 *   n_out[k]                   configurations copied, at most max_per_key
 *   n_total[k]                 the frontier's size
 *
 * n_out[k] = n_total[k] = 0 when the stop op's return is a no-op (the op had
 * been linearized in every configuration), and -1 when the search could not
 * get there: the key does not fit lc_counted_plan's rule or has more than
 * `slots` other ops open at once, has a malformed record, the configuration
 * or time budget ran out, the key failed before that return, stop_op[k] is
 * not an :ok op of the key, or the frontier outgrew the top capacity.  Slots
 * of `out` and `pending` past a key's count are left as they were.
 *
 * A configuration's pending ops are the open ops not linearized in it; of a
 * class's crashed members, which the search linearizes in call order, the
 * ones from the first not linearized on.  Ops linearized in every
 * configuration are retired and pending in none.
 *
 * Returns 0, -EINVAL (null ctx or buffer, n_keys < 0, max_per_key < 1,
 * key_off not monotone, pending_cap < max_per_key * (key_off[n_keys] -
 * key_off[0]); message in lc_last_error), -ENOMEM or -EIO.
 */
typedef struct lc_counted_config {
  int64_t version, value; /* value: the caller's id; LC_NIL for nil */
  int64_t n_pending;      /* the whole pending set, no cap */
  int64_t pending_at;     /* index into `pending` of its sorted record indices */
} lc_counted_config;

int lc_check_frontiers_counted(lc_ctx *ctx, const lc_op *ops, const int64_t *key_off, int64_t n_keys,
                               const int64_t *stop_op, const lc_opts *opts,
                               lc_counted_config *out, int32_t max_per_key,
                               int32_t *n_out, int64_t *n_total,
                               int64_t *pending, int64_t pending_cap);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_COUNTED_H */
