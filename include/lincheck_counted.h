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

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_COUNTED_H */
