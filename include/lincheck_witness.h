/*
 * lincheck_witness.h — statistics of the witness search of lc_check
 * (LC_FLAG_SEARCH_WITNESS, LC_WITNESS_ORDER_FULL / LC_WITNESS_ORDER_PREFIX:
 * include/lincheck.h).  Included by lincheck.h; additive to ABI 5 (callers
 * detect the feature by looking up lc_last_witness_stats).
 */
#ifndef LINCHECK_WITNESS_H
#define LINCHECK_WITNESS_H

#include "lincheck.h"

#ifdef __cplusplus
extern "C" {
#endif

/* LC_FLAG_SEARCH_WITNESS: the witness search's share of the most recent call,
 * summed over its devices (all zero without the flag).  n_keys = n_found +
 * n_budget + n_window. */
typedef struct lc_witness_stats {
  int64_t n_keys;      /* decided keys without a witness that the search took */
  int64_t n_found;     /* ... that got an ORDER_FULL / ORDER_PREFIX witness */
  int64_t n_budget;    /* ... given up: search-step budget (max_configs_per_key, capped by the
                          library) or time_budget_ms spent */
  int64_t n_window;    /* ... given up: more than LC_MAX_WINDOW ops open at once */
  int64_t nodes;       /* search steps (ops linearized, retries included) */
  int64_t cache_hits;  /* configurations met again after they were found to be dead ends */
  double  kernel_ms;   /* device time of the stage (HIP events) */
} lc_witness_stats;

int lc_last_witness_stats(lc_ctx *ctx, lc_witness_stats *out);

/* LC_FLAG_COUNTED_WITNESS (with LC_FLAG_SEARCH_WITNESS): the share of the
 * second witness stage, which searches the keys counted in
 * lc_witness_stats.n_window with their crashed writes/CAS counted per class
 * (lc_counted_plan's layout); summed over the call's devices, all zero without
 * both flags.  n_keys = n_found + n_budget + n_unfit.  Additive to ABI 5:
 * callers detect the feature by looking up lc_last_counted_witness_stats. */
typedef struct lc_counted_witness_stats {
  int64_t n_keys;      /* keys the first stage left at n_window */
  int64_t n_found;     /* ... that got an ORDER_FULL / ORDER_PREFIX witness */
  int64_t n_budget;    /* ... given up: search-step budget or time_budget_ms spent */
  int64_t n_unfit;     /* ... given up: beyond lc_counted_plan's rule, or more than its
                          `slots` other ops open at once */
  int64_t nodes;       /* search steps (ops linearized, retries included) */
  int64_t cache_hits;  /* configurations met again after they were found to be dead ends */
  double  kernel_ms;   /* device time of the stage (HIP events) */
} lc_counted_witness_stats;

int lc_last_counted_witness_stats(lc_ctx *ctx, lc_counted_witness_stats *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_WITNESS_H */
