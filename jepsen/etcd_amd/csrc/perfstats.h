// perfstats.h — what lc_perf_stats' host code (perfstats_host.cpp, g++) and
// its kernels (perfstats.hip) share: rule 8's tests of include/lincheck_perf.h,
// rule 7's bucket arithmetic, rule 6's quantile index, and the launchers.
#pragma once
#include <errno.h>
#include <math.h>
#include <stdint.h>

#include "../../../include/lincheck_perf.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LCPS_HD __host__ __device__ __forceinline__
#else
#define LCPS_HD inline
#endif

namespace lcps {

constexpr int64_t kMaxF = 65536;                       // lc_ps_event.f is 16 bits
constexpr int64_t kMaxTableEntries = int64_t(1) << 24;
constexpr int64_t kDefaultLdsEntries = 8192;           // uint32 each: 32 KiB of a workgroup's LDS
constexpr int kWave = 64;
constexpr int kBlock = 256;
constexpr int kChunk = 2048;                           // slots a pair-pass workgroup takes at a time
constexpr int kMaxGrid = 1024;
static_assert(kChunk % kBlock == 0, "a chunk is whole rounds of the workgroup");

// what is wrong with one record (rule 8), as bits of the device's status word
constexpr int kBadTime = 1, kBadType = 2, kBadF = 4;

LCPS_HD int bad_event(const lc_ps_event &e, int32_t n_f) {
  int bad = 0;
  if (e.time < 0) bad |= kBadTime;
  if (e.type > LC_EV_INFO) bad |= kBadType;
  if (e.process >= 0 && (int32_t)e.f >= n_f) bad |= kBadF;
  return bad;
}

inline const char *bad_text(int bad) {
  return bad & kBadTime ? "a negative time" : bad & kBadType ? "a type above 3" : "a client event's f >= n_f";
}

// rule 6: one IEEE multiply (q and n are doubles before it: nothing to fuse)
LCPS_HD int64_t quantile_index(double q, int64_t n) {
  const double x = floor(q * (double)n);
  const int64_t i = (int64_t)x;
  return i < n - 1 ? i : n - 1;
}

// Rule 8's tests of the parameters and the arrays: 0 or -EINVAL / -E2BIG with
// the text in *why.
inline int check_params(const lc_ps_event *ev, int64_t n_events, const lc_ps_params *p, const lc_ps_out *out,
                        const char **why) {
  *why = nullptr;
  if (!p || !out)
    *why = "null params or out";
  else if (n_events < 0 || n_events >= (int64_t(1) << 31))
    *why = "n_events outside [0, 2^31)";
  else if (n_events > 0 && !ev)
    *why = "null events";
  else if (p->n_f < 1)
    *why = "n_f < 1";
  else if (p->n_q < 0 || p->n_q > LC_PS_MAX_Q)
    *why = "n_q outside [0, 8]";
  else if (p->rate_dt_ns <= 0 || p->quant_dt_ns <= 0)
    *why = "a dt of 0 or less";
  else if (!out->by_f || !out->rate || !out->quant_n || (p->n_q > 0 && !out->quant))
    *why = "a null table";
  else if (!out->comp_pos != !out->latency_ns)
    *why = "comp_pos and latency_ns are given together or not at all";
  else if (out->rate_cap < 0 || out->quant_cap < 0)
    *why = "a negative cap";
  if (*why) return -EINVAL;
  for (int i = 0; i < p->n_q; i++)
    if (!(p->q[i] >= 0.0 && p->q[i] <= 1.0)) {  // (a NaN fails both)
      *why = "a q outside [0, 1]";
      return -EINVAL;
    }
  if (p->n_f > kMaxF) {
    *why = "n_f above lc_perf_stats_limits' max_f";
    return -E2BIG;
  }
  return 0;
}

// Rule 7's counts from t_max, then rule 8's -E2BIG and -ENOSPC (the counts
// are written either way).
inline int check_tables(int64_t t_max, const lc_ps_params *p, const lc_ps_out *out, int64_t *n_rate, int64_t *n_quant,
                        const char **why) {
  *n_rate = t_max / p->rate_dt_ns + 1;
  *n_quant = t_max / p->quant_dt_ns + 1;
  const int64_t nq = p->n_q > 0 ? p->n_q : 1;
  if (*n_rate > kMaxTableEntries / (3 * (int64_t)p->n_f) || *n_quant > kMaxTableEntries / (nq * (int64_t)p->n_f)) {
    *why = "a table above lc_perf_stats_limits' max_table_entries";
    return -E2BIG;
  }
  if (out->rate_cap < *n_rate || out->quant_cap < *n_quant) {
    *why = "rate_cap or quant_cap below the buckets' count";
    return -ENOSPC;
  }
  return 0;
}

// -ENOSPC's summary: what the caller sizes its tables from
inline void summary_for_room(lc_ps_summary *sum, int64_t n_events, int64_t n_client, int64_t t_max, int64_t n_rate,
                             int64_t n_quant) {
  if (!sum) return;
  *sum = lc_ps_summary{};
  sum->n_events = n_events;
  sum->n_client = n_client;
  sum->t_max = t_max;
  sum->n_rate_buckets = n_rate;
  sum->n_quant_buckets = n_quant;
}

// The compact tables (rows of rule 7's counts) into the caller's (rows of its
// caps, the rest of a row 0 / LC_PS_NONE); by_f, the totals and the verdict
// from the rate table (rule 2 counts what rule 5 counts).
inline void place_tables(const lc_ps_params *p, const int64_t *rate, const int64_t *quant_n, const int64_t *quant,
                         int64_t n_rate, int64_t n_quant, const lc_ps_out *out, lc_ps_summary *sm) {
  const int64_t nf = p->n_f, nq = p->n_q;
  sm->valid = 1;
  for (int64_t f = 0; f < nf; f++) {
    int64_t by[3] = {0, 0, 0};
    for (int t = 0; t < 3; t++) {
      const int64_t *src = rate + (f * 3 + t) * n_rate;
      int64_t *dst = out->rate + (f * 3 + t) * out->rate_cap;
      for (int64_t b = 0; b < out->rate_cap; b++) dst[b] = b < n_rate ? src[b] : 0;
      for (int64_t b = 0; b < n_rate; b++) by[t] += src[b];
    }
    const int64_t count = by[0] + by[1] + by[2];
    int64_t *row = out->by_f + f * 4;
    row[0] = count, row[1] = by[0], row[2] = by[1], row[3] = by[2];
    sm->count += count, sm->ok += by[0], sm->fail += by[1], sm->info += by[2];
    if (count > 0 && by[0] == 0) sm->valid = 0;
    for (int64_t b = 0; b < out->quant_cap; b++) {
      out->quant_n[f * out->quant_cap + b] = b < n_quant ? quant_n[f * n_quant + b] : 0;
      for (int64_t k = 0; k < nq; k++)
        out->quant[(f * out->quant_cap + b) * nq + k] = b < n_quant ? quant[(f * n_quant + b) * nq + k] : LC_PS_NONE;
    }
  }
}

#if defined(__HIPCC__)
// what the scan and the pair pass tell the host
struct Status {
  int32_t bad;                 // kBad* bits of every record
  int32_t pad;
  unsigned long long t_max;    // over client events
  unsigned long long n_client;
  unsigned long long n_pairs, n_pending, n_ignored, n_mismatched;
};

// One call's device workspace.  A slot is a place in process-sorted order;
// the client events' slots come first (a record that is no client's sorts
// last).  hist: the rate table, then quant_n, both compact.
struct Ws {
  const lc_ps_event *ev;
  int64_t n_events;
  int32_t n_f, n_q;
  double q[LC_PS_MAX_Q];
  int64_t rate_dt, quant_dt;
  uint32_t *pkey_in, *pkey;    // n_events: the process (0xFFFFFFFF: no client's), before and after the sort
  int32_t *ppos_in, *ppos;     // n_events: the position
  int32_t *comp_pos;           // n_events, or null
  int64_t *latency;            // n_events, or null
  int64_t n_client;            // (after the scan)
  int64_t n_rate, n_quant;
  unsigned long long *hist;    // n_f * 3 * n_rate + n_f * n_quant, zeroed per call
  int64_t hist_entries, lds_entries;
  uint32_t *gkey, *gkey2;      // n_client: a pair's group f * n_quant + b, or n_f * n_quant
  int64_t *glat, *glat2;       // n_client: its latency
  int64_t *quant;              // n_f * n_quant * n_q
  Status *status;
  void *temp;                  // rocPRIM's
  size_t temp_bytes;
};

// the sorts' temporary storage for n slots (the largest of the three)
size_t sort_temp_bytes(int64_t n, int group_bits);
// Rule 8 on every record, t_max, n_client; the sort's keys and positions; the
// point arrays' "none".
hipError_t launch_scan(const Ws &w, hipStream_t st);
// the stable sort of positions by process
hipError_t launch_process_sort(const Ws &w, hipStream_t st);
// quant filled with LC_PS_NONE; pairs, counts and (group, latency) per slot
hipError_t launch_pairs(const Ws &w, hipStream_t st);
// by latency, then stable by group: sorted lands in gkey / glat again
hipError_t launch_group_sort(const Ws &w, int group_bits, hipStream_t st);
// each group's start picks its n_q entries
hipError_t launch_select(const Ws &w, hipStream_t st);
#endif

}  // namespace lcps
