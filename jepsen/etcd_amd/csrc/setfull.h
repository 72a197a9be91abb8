// setfull.h — what lc_set_full's host code (setfull_host.cpp, g++) and its
// kernels (setfull.hip) share: rules 4 to 6 of include/lincheck_setfull.h as
// one function, the element table's hash, and the kernels' launcher.
#pragma once
#include <stdint.h>

#include "../../../include/lincheck_setfull.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LCSF_HD __host__ __device__ __forceinline__
#else
#define LCSF_HD inline
#endif

namespace lcsf {

constexpr int64_t kEmpty = INT64_MIN;          // the table's empty key (lc_sf_add.value never is)
constexpr int64_t kDefaultTileBytes = int64_t(1) << 30;
constexpr int64_t kMaxPosition = 0x7FFFFFFF;   // positions are below 2^31 - 1
constexpr int kCounterStride = 16;             // in int64: the workgroups' counters lie 128 B apart
constexpr int kCounterShards = 32;

// The element table: open addressing, linear probing from this slot.  cap is
// a power of two of at least 2 E.  (murmur3's 64-bit finaliser: sequential
// ids and values that agree in their low bits both spread.)
LCSF_HD uint64_t slot_of(int64_t value, uint64_t cap) {
  uint64_t x = (uint64_t)value;
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x & (cap - 1);
}

inline uint64_t table_capacity(int64_t n_elements) {
  uint64_t cap = 64;
  while (cap < 2 * (uint64_t)n_elements) cap <<= 1;
  return cap;
}

// max(0, t - known) / 1,000,000 where t = time + 1 (rule 6), or t = 0 when
// `has` is false; in unsigned arithmetic, so that no input overflows.
LCSF_HD int64_t latency_ms(bool has, int64_t time, int64_t known) {
  if (!has) return known < 0 ? (int64_t)((0 - (uint64_t)known) / 1000000u) : 0;
  if (time < known) return 0;
  return (int64_t)(((uint64_t)time - (uint64_t)known + 1) / 1000000u);
}

// Rules 4 to 6 for one element, from what its concerning reads say: the
// first observing read's completion (fs_pos < 0: never observed), and the
// invokes last_present / last_absent (pos < 0: none) with their times.
// dup_max and LC_SF_DUPLICATED are the caller's (rule 7).
LCSF_HD lc_sf_element decide(const lc_sf_add &a, int32_t fs_pos, int64_t fs_time, int32_t lp_pos,
                             int64_t lp_time, int32_t la_pos, int64_t la_time) {
  lc_sf_element o;
  int32_t known_pos = -1;
  int64_t known_time = 0;
  if (a.ok_pos >= 0 && (fs_pos < 0 || a.ok_pos <= fs_pos)) {
    known_pos = a.ok_pos;
    known_time = a.ok_time;
  } else if (fs_pos >= 0) {
    known_pos = fs_pos;
    known_time = fs_time;
  }
  o.outcome = LC_SF_NEVER_READ;
  o.flags = 0;
  o.known_pos = known_pos;
  o.last_present = lp_pos;
  o.last_absent = la_pos;
  o.dup_max = 0;
  o.stable_latency_ms = -1;
  o.lost_latency_ms = -1;
  if (lp_pos >= 0 && la_pos < lp_pos) {
    o.outcome = LC_SF_STABLE;
    o.stable_latency_ms = latency_ms(la_pos >= 0, la_time, known_time);
    if (o.stable_latency_ms > 0) o.flags = LC_SF_STALE;
  } else if (known_pos >= 0 && la_pos >= 0 && lp_pos < la_pos && known_pos < la_pos) {
    o.outcome = LC_SF_LOST;
    o.lost_latency_ms = latency_ms(lp_pos >= 0, lp_time, known_time);
  }
  return o;
}

// setfull_host.cpp.  check_contract: 0 or -EINVAL with the text in err
// (everything but two adds of one value).  summarize: sum's counts and the
// verdict from the element array (rule 8); n_phantom, n_tiles and the times
// are the caller's.  count_duplicates: rule 7 for the elements with
// marked[e] != 0, into out[e].dup_max / LC_SF_DUPLICATED.
int check_contract(const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads, int64_t n_reads,
                   const int64_t *read_values, int64_t n_values, const char **err);
void summarize(const lc_sf_element *out, int64_t n_adds, int32_t linearizable, lc_sf_summary *sum);
int count_duplicates(const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads, int64_t n_reads,
                     const int64_t *read_values, const uint8_t *marked, lc_sf_element *out);

#if defined(__HIPCC__)
struct Ent {  // a table slot's payload: the element and its add's inv_pos
  int32_t id, inv_pos;
};

// One call's device workspace.  The bitmap holds the rows of elements
// [e0, e1) of one tile: row stride wpr = ceil(n_reads / 32) words, column c
// is reads[c] (ok_pos order).
struct Ws {
  const lc_sf_add *adds;
  const lc_sf_read *reads;
  const int64_t *values;   // the payload
  const int64_t *work_off; // n_reads + 1: prefix sums of the reads' len
  int64_t n_adds, n_reads, n_work;
  int64_t *tab_key;        // cap
  Ent *tab_ent;            // cap
  uint64_t cap;
  int32_t *r_inv, *r_ok;   // n_reads: the reads' positions, one array each
  uint32_t *bitmap;
  int64_t wpr;
  uint8_t *dup_seen;       // per element (zeroed per call)
  int64_t *counters;       // kCounterShards x kCounterStride (zeroed per call): phantoms
  int32_t *status;         // [0] two adds of one value, [1] one such element, [2] some dup_seen is set
  lc_sf_element *out;      // n_adds
};

// The table's fill and insertions, once per call.
hipError_t launch_table(const Ws &w, hipStream_t st);
// One tile: the bitmap zeroed, the mark pass restricted to elements
// [e0, e1), their records written.  Phantoms are counted when e0 == 0.
hipError_t launch_tile(const Ws &w, int64_t e0, int64_t e1, hipStream_t st);
#endif

}  // namespace lcsf
