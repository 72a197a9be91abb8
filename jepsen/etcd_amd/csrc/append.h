// append.h — what lc_append_check's host code (append_host.cpp, g++) and its
// kernels (append.hip) share: the (key, element) hash, the host's
// preparation pass, the host parts of the device call, and the kernels'
// workspace and launchers.  The rules are include/lincheck_append.h's.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../../include/lincheck_append.h"
#include "graph_host.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LCAP_HD __host__ __device__ __forceinline__
#else
#define LCAP_HD inline
#endif

namespace lcap {

constexpr int64_t kReserved = INT64_MIN;        // no key and no appended element
constexpr int64_t kMaxPosition = 0x7FFFFFFF;    // positions are below 2^31 - 1
constexpr int64_t kMaxMops = 0x7FFFFFFF;
// the device call's bound on n_mops: the key table (table_capacity) then has at most 2^30 slots, and a slot
// index is an int32 (mop_kslot, the slot list of the key records)
constexpr int64_t kMaxDeviceMops = int64_t(1) << 29;
constexpr int64_t kDefaultMaxPayload = int64_t(1) << 30;
constexpr int kCounterStride = 16;              // in int64: the waves' counters lie 128 B apart
constexpr int kCounterShards = 32;
constexpr int kCounters = 6;                    // duplicate, g1a, phantom, g1b, internal, slow reads
constexpr int kItemChunk = 4096;                // work items of one workgroup iteration of the item pass

LCAP_HD uint64_t mix64(uint64_t x) {  // murmur3's 64-bit finaliser
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}

// The writer table's hash of a (key, element) pair: the slot is its low bits,
// the slot's tag its high 32.
LCAP_HD uint64_t hash_pair(int64_t key, int64_t element) {
  return mix64(mix64((uint64_t)key) + 0x9E3779B97F4A7C15ull + (uint64_t)element);
}

// Both tables: a power of two of at least 2 n, at least 64.
inline uint64_t table_capacity(int64_t n) {
  uint64_t cap = 64;
  while (cap < 2 * (uint64_t)n) cap <<= 1;
  return cap;
}

// The longest-read word of a key: (len, ~read ordinal), larger is better;
// 0: never read.
LCAP_HD uint64_t pack_best(int32_t len, int32_t r) { return ((uint64_t)(uint32_t)len << 32) | (uint32_t)~r; }
LCAP_HD int32_t best_read(uint64_t b) { return (int32_t)~(uint32_t)b; }
LCAP_HD int32_t best_len(uint64_t b) { return (int32_t)(b >> 32); }

// What one pass over the input gives the host (append_host.cpp, prepare):
// the contract checked, and the arrays both paths index by.  The "real" reads
// are the READ mops with len >= 0, numbered r = 0.. in mop order; their
// payload entries are the work items, numbered through work_off.
struct Prep {
  std::vector<int32_t> mop_txn;   // n_mops
  std::vector<int32_t> rd_mop;    // per real read: its mop
  std::vector<int32_t> txn_r0;    // n_txns + 1: real reads before the txn's first mop
  std::vector<int64_t> work_off;  // real reads + 1: prefix sums of len
  int64_t n_ok = 0, n_nodes = 0, n_reads = 0, n_appends = 0;
};

// 0 or -EINVAL with the text in err (everything but two appends of one pair).
int prepare(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops, const int64_t *values,
            int64_t n_values, const lc_ap_out *out, Prep *p, const char **err);

// The writers of rule 1 as a host hash map (the host twin always, the device
// call only when it has slow reads).  build: 0, or -EINVAL at two appends of
// one pair.
struct Writers {
  struct Impl;
  Impl *impl = nullptr;
  std::vector<uint8_t> last;  // per mop: an append that is its txn's last to the key
  ~Writers();
  int build(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops);
  int32_t find(int64_t key, int64_t element) const;  // the mop, or -1
};

// Rules 3 and 4 for every read of txn t from their definitions (element
// look-ups and payload compares): mop_flags of its reads, LC_AP_R_NONPREFIX
// kept as found, and txn_flags[t].  Returns how many reads it did.
int64_t rules34_direct(const lc_ap_txn *txns, const lc_ap_mop *mops, const int64_t *values, const Prep &p,
                       const Writers &w, int64_t t, int32_t *mop_flags, int32_t *txn_flags);

// first_dup of one key's order from its definition (phantoms included).
int32_t first_dup_direct(const int64_t *order, int32_t len);

// Rule 6 on the host (graph_host.cpp).
using lcgraph::real_time_host;

// Rule 7 (graph_host.cpp's cycles_host) and rule 8 over finished flags, keys, edges and ranges: out->scc,
// scc_class, steps, cycle_off, cycle_scc, and every field of sum but the
// read counts (taken from counts[kCounters]), n_slow_reads and the device times.
void graph_and_summary(const lc_ap_txn *txns, int64_t n_txns, const Prep &p, const lc_ap_out *out, int64_t n_keys,
                       int64_t n_edges, int64_t n_nonprefix, const int64_t *counts, lc_ap_summary *sum);

#if defined(__HIPCC__)
// One call's device workspace.
struct Ws {
  const lc_ap_txn *txns;
  const lc_ap_mop *mops;
  const int64_t *values;
  const int32_t *mop_txn, *rd_mop, *txn_r0;
  const int64_t *work_off;
  int64_t n_txns, n_mops, n_real, n_work;
  // the writer table: a word is (tag << 32) | append mop, ~0 when empty;
  // stamp: the least order index that named the entry (-1: none; the
  // kernels' atomicMin reads it unsigned)
  unsigned long long *wtab;
  int32_t *stamp;
  uint64_t wcap;
  // the key table, slot by slot: the key (stored xor 2^63 - 1, so that the
  // reserved key is ~0: empty), the longest-read word, first_dup /
  // first_failed / first_phantom (-1: none, unsigned to atomicMin), flags
  // (LC_AP_K_INCOMPATIBLE; bit 30: two phantoms, first_dup is the host's)
  int64_t *ktab;
  unsigned long long *kbest;
  int32_t *kfirst;     // 3 per slot
  int32_t *kflags;
  uint64_t kcap;
  int32_t *mop_kslot;  // n_mops
  uint8_t *mop_last;   // n_mops: rule 1's "last append to the key"
  int32_t *ord_w;      // n_work: at the longest read's items, the entry's writer mop or -1
  uint8_t *nonprefix;  // per real read
  int32_t *mop_flags;  // n_mops
  int32_t *txn_flags;  // n_txns; bit 30: the host recomputes this txn's reads
  lc_ap_edge *slots;   // 2 n_real + n_work edge slots, from = -1 when empty
  lc_ap_key *keys;     // compacted key records (slot order; the host sorts them)
  int64_t *counters;   // kCounters x kCounterShards x kCounterStride (zeroed per call)
  int32_t *status;     // [0] two appends of one pair, [1] one such mop
};

constexpr int32_t kKeyTwoPhantoms = 1 << 30;
constexpr int32_t kTxnSlow = 1 << 30;

// Tables filled and built, longest reads taken, the item pass, the read/txn
// pass, the ww slots and the key records: everything before the edge sort.
// kslots has kcap entries; *d_n_keys receives the number of key records.
size_t key_temp_bytes(uint64_t kcap);
hipError_t launch_rules(const Ws &w, int32_t *kslots, int64_t *d_n_keys, void *temp, size_t temp_bytes,
                        hipStream_t st);

// Edge compaction, sort and unique; real time.  Temporary storage is the
// caller's: *_bytes(n) say how much a call over n records needs.
size_t edge_temp_bytes(int64_t n_slots);
hipError_t launch_edge_select(const Ws &w, lc_ap_edge *dst, int64_t *d_count, void *temp, size_t temp_bytes,
                              hipStream_t st);
hipError_t launch_edge_sort(lc_ap_edge *src, lc_ap_edge *dst, int64_t n, int64_t *d_count, void *temp,
                            size_t temp_bytes, hipStream_t st);
size_t rt_temp_bytes(int64_t n_txns);
// byc (n_ok of them), rt_lo, rt_hi on the device; the int32 arrays have
// n_txns entries each, d_count is one scratch word.
hipError_t launch_real_time(const Ws &w, int64_t n_ok, int32_t *ok_idx, int32_t *ok_comp, int32_t *byc,
                            int32_t *comp_sorted, int32_t *pm, int32_t *rt_lo, int32_t *rt_hi, int64_t *d_count,
                            void *temp, size_t temp_bytes, hipStream_t st);
#endif

}  // namespace lcap
