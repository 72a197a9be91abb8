/*
 * lincheck_wrlin.h — lc_wr_check_lin: lc_wr_check (lincheck_wr.h) with Elle's
 * :linearizable-keys? inference.  etcd claims strict serializability, so every
 * key is linearizable: real time orders each key's versions, and every
 * external read and write becomes checkable — a stale read between two blind
 * writes included, which the wfr edges alone never see.  The reference's :wr
 * workload comments the option out as expensive; here the inference runs on
 * the device.  Included by lincheck.h; additive to ABI 5 (callers detect the
 * feature by looking up lc_wr_check_lin).
 *
 * Rules 1-3, 5 and 8-10 of lincheck_wr.h hold word for word.  With
 * LC_WR_LINEARIZABLE_KEYS set, rules 4, 6 and 7 become:
 *
 *  4'. Lin edges.  Per key k, K(k) is the set of OK txns that touch k: a txn
 *      touches k if it has an external read of k or at least one write to it.
 *      INFO and FAIL txns are never in K(k).  For T in K(k), first(T, k) is
 *      its external read's value (nil included) if it has one, else its
 *      external write (its last write to k); last(T, k) is its external write
 *      if it writes k, else its external read's value.  T2 is a key-successor
 *      of T1 iff comp(T1) < inv(T2) and no T3 in K(k) has comp(T1) < inv(T3)
 *      and comp(T3) < inv(T2): rule 8's reduction, taken inside K(k).  Every
 *      such pair adds the version edge last(T1, k) -> first(T2, k) when the
 *      two differ; a lin edge never makes a self-loop.  The version graph is
 *      still a set: initial + wfr (if LC_WR_WFR_KEYS) + lin, each edge once
 *      however often it arises.
 *      Range form (the device and the host use it): with K(k) sorted by inv
 *      and m the least comp among the members with inv > comp(T1), T1's
 *      successors are the members with comp(T1) < inv < m, a contiguous run.
 *      This is ours by derivation, parity with Elle unpinned as for the rest:
 *      Elle walks the reduced whole-history graph through txns that do not
 *      touch k, which can add edges that the per-key reduction already implies
 *      transitively; reachability is the same either way.
 *  6'. Cyclic versions.  A key is LC_WR_K_CYCLIC iff its whole version graph
 *      has a cycle, wfr self-loops counting.  nil can now have incoming edges,
 *      so initial edges can close cycles.  cyc_value is the least non-nil
 *      value on a cycle — on one, not merely below or between cycles; every
 *      cycle holds a non-nil value.
 *  7'. Edges.  Rule 7 over the enlarged edge set.  A version edge whose head
 *      has no writer (nil, a phantom) gives no ww / rw edge; a tail without a
 *      writer gives rw edges only.  n_edges_raw keeps its definition, over
 *      the enlarged set.
 *
 * Elle's :sequential-keys? stays out of scope.
 */
#ifndef LINCHECK_WRLIN_H
#define LINCHECK_WRLIN_H

#include "lincheck_wr.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LC_WR_LINEARIZABLE_KEYS 2u  /* flags: infer the lin edges of rule 4' */

/* Parallel to out->keys (room for n_mops; sum->n_keys written). */
typedef struct lc_wr_lin_key {
  int64_t n_pairs;    /* key-successor pairs of the key */
  int32_t n_touches;  /* |K(k)| */
  int32_t n_vedges;   /* distinct version edges of the key, all three sources, self-loops included; the
                         initial edges count whether or not anybody read nil */
} lc_wr_lin_key;      /* 16 bytes */

typedef struct lc_wr_lin_summary {
  int64_t n_touches, n_pairs, n_vedges;  /* the records' fields summed */
  int64_t max_key_versions;  /* the most versions any key's graph holds (see lc_wr_lin_limits) */
  double lin_kernel_ms;      /* lc_wr_check_lin: the HIP-event interval from the touches to the closure; it
                                is part of sum->kernel_ms */
} lc_wr_lin_summary;

/*
 * Both calls: lc_wr_check's contract, but flags is any of LC_WR_WFR_KEYS |
 * LC_WR_LINEARIZABLE_KEYS (anything else: -EINVAL), and lin_keys may not be
 * NULL; lin_sum may.  Nothing is written on an error, to lin_keys and lin_sum
 * either (-ENOSPC writes sum as lc_wr_check does).  Without the lin bit every
 * output equals lc_wr_check(_host)'s and the lin records and summary hold
 * zeros.
 */
/* (struct tags, as in lincheck_screen.h: this header may be read, through lincheck.h, before lincheck_wr.h's body) */
int lc_wr_check_lin_host(const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_wr_mop *mops, int64_t n_mops,
                         uint32_t flags, const struct lc_wr_out *out, struct lc_wr_summary *sum,
                         lc_wr_lin_key *lin_keys, lc_wr_lin_summary *lin_sum);

/* Rules 1-8 on the context's first GPU, rule 9 by the host code.  Errors are
 * lc_wr_check's; -E2BIG also where a key's graph holds more than
 * lc_wr_lin_limits' max_key_versions versions.  After any error the context
 * stays usable.  A call without txns, or with txns that have no mop at all,
 * is answered by the host code: there is nothing for the device to do. */
int lc_wr_check_lin(lc_ctx *ctx, const struct lc_ap_txn *txns, int64_t n_txns, const struct lc_wr_mop *mops,
                    int64_t n_mops, uint32_t flags, const struct lc_wr_out *out, struct lc_wr_summary *sum,
                    lc_wr_lin_key *lin_keys, lc_wr_lin_summary *lin_sum);

/*
 * The device call keeps each key's version graph as a bit matrix: a key whose
 * graph holds V versions — the distinct values written to it or read from it
 * by a known read, nil among them only where a txn read it — owns V x
 * ceil(V / 64) 64-bit words.  Keys of at most wave_key_versions versions are
 * closed by one wavefront in registers, larger ones by one workgroup with the
 * rows in the LDS, which bounds V by max_key_versions; above it the call
 * returns -E2BIG.  As the versions number n_mops at most, the matrices take
 * at most max_key_versions x n_mops / 8 bytes (sum of V^2 / 8 rounded up to
 * whole words per row), which the call reserves and clears before it knows
 * the keys: 64 B per mop beside lc_wr_check's memory, whatever the keys'
 * sizes (160 MB at 2.5 x 10^6 mops, 34 GB at max_mops), so that a very large
 * call can return -ENOMEM where lc_wr_check succeeds.  (The host function
 * has no such bound.)  Host-only.
 */
typedef struct lc_wr_lin_limit_info {
  int64_t max_key_versions;   /* 512 */
  int64_t wave_key_versions;  /* 64 */
} lc_wr_lin_limit_info;

int lc_wr_lin_limits(lc_wr_lin_limit_info *out);

#ifdef __cplusplus
}
#endif

#endif /* LINCHECK_WRLIN_H */
