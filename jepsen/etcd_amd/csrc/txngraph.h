// txngraph.h — what the two Elle checkers (lc_append_check, lc_wr_check)
// share before a transaction graph's edges stand, on the host (g++) and on the
// device (hipcc): the (key, value) hash and the table sizing, the limits, the
// sharded counters' geometry, the item chunk, the edges' order, the contract
// of the txn records, and the launchers of txngraph.hip (the key table's
// occupied slots, the edges' select / sort / unique, real time).  The txn,
// edge and step records are list-append's (include/lincheck_wr.h names them
// anew).  What the checkers share once the edges stand is graph_host.h's.
// Header-only on the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <initializer_list>
#include <utility>

#include "../../../include/lincheck_append.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LCTG_HD __host__ __device__ __forceinline__
#else
#define LCTG_HD inline
#endif

namespace lctg {

constexpr int64_t kMaxPosition = 0x7FFFFFFF;    // positions are below 2^31 - 1
constexpr int64_t kMaxMops = 0x7FFFFFFF;
// the device calls' bound on n_mops: a table (table_capacity) then has at most 2^30 slots, and a slot
// index is an int32 (mop_kslot, the slot list of the key records)
constexpr int64_t kMaxDeviceMops = int64_t(1) << 29;
constexpr int kCounterStride = 16;              // in int64: the waves' counters lie 128 B apart
constexpr int kCounterShards = 32;
constexpr int kItemChunk = 4096;                // work items of one workgroup iteration of an item pass

LCTG_HD uint64_t mix64(uint64_t x) {  // murmur3's 64-bit finaliser
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}

// A pair table's hash of (key, element or value): the slot is its low bits,
// the slot's tag its high 32.
LCTG_HD uint64_t hash_pair(int64_t key, int64_t value) {
  return mix64(mix64((uint64_t)key) + 0x9E3779B97F4A7C15ull + (uint64_t)value);
}

struct PairHash {
  size_t operator()(const std::pair<int64_t, int64_t> &p) const { return (size_t)hash_pair(p.first, p.second); }
};

// Every table: a power of two of at least 2 n, at least 64.
inline uint64_t table_capacity(int64_t n) {
  uint64_t cap = 64;
  while (cap < 2 * (uint64_t)n) cap <<= 1;
  return cap;
}

// The edges' order, (from, to, type, key), and what makes two of them one:
// the host's sort and unique and the device's (txngraph.hip) give one list.
LCTG_HD bool edge_less(const lc_ap_edge &a, const lc_ap_edge &b) {
  if (a.from != b.from) return a.from < b.from;
  if (a.to != b.to) return a.to < b.to;
  if (a.type != b.type) return a.type < b.type;
  return a.key < b.key;
}

LCTG_HD bool edge_same(const lc_ap_edge &a, const lc_ap_edge &b) {
  return a.from == b.from && a.to == b.to && a.type == b.type && a.key == b.key;
}

// Counter b of kCounterShards x kCounterStride sharded ones (the host's copy).
inline int64_t sum_counters(const int64_t *h_counters, int b) {
  int64_t v = 0;
  for (int i = 0; i < kCounterShards; i++) v += h_counters[((size_t)b * kCounterShards + i) * kCounterStride];
  return v;
}

// The contract of txn x, the one after a txn invoked at prev_inv (-1: the
// first) whose mops end at `next`: null, or what is wrong with it.
inline const char *check_txn(const lc_ap_txn &x, int64_t prev_inv, int64_t next, int64_t n_mops) {
  if (x.inv_pos <= prev_inv || x.inv_pos >= kMaxPosition) return "txns not strictly ascending by inv_pos";
  if (x.type == LC_AP_INFO) {
    if (x.comp_pos != -1) return "an INFO txn with a comp_pos";
  } else if (x.type == LC_AP_OK || x.type == LC_AP_FAIL) {
    if (x.comp_pos <= x.inv_pos || x.comp_pos >= kMaxPosition) return "comp_pos not above inv_pos";
  } else {
    return "unknown txn type";
  }
  if (x.mop_off != next || x.mop_len < 0 || x.mop_len > n_mops - next)
    return "the txns' mop ranges do not tile the mops in order";
  return nullptr;
}

// No out, or one of its arrays missing (lc_ap_out and lc_wr_out name them alike).
template <class Out>
bool null_out(const Out *out) {
  return !out || !out->mop_flags || !out->txn_flags || !out->keys || !out->edges || !out->byc || !out->rt_lo ||
         !out->rt_hi || !out->scc || !out->scc_class || !out->steps || !out->cycle_off || !out->cycle_scc;
}

#if defined(__HIPCC__)
// The launchers of txngraph.hip.  Temporary storage is the caller's:
// *_temp_bytes say how much a call needs.

// The occupied slots of a key table of kcap slots (a stored key is
// key ^ kKeyXor, so an empty slot reads -1), in slot order, into kslots (kcap
// entries); *d_n_keys receives their number.
size_t key_temp_bytes(uint64_t kcap);
hipError_t launch_key_slots(const int64_t *ktab, uint64_t kcap, int32_t *kslots, int64_t *d_n_keys, void *temp,
                            size_t temp_bytes, hipStream_t st);

// Edge compaction (the slots with from >= 0 into dst, their number into
// *d_count), then sort into dst and unique back into src.
size_t edge_temp_bytes(int64_t n_slots);
hipError_t launch_edge_select(const lc_ap_edge *slots, int64_t n_slots, lc_ap_edge *dst, int64_t *d_count, void *temp,
                              size_t temp_bytes, hipStream_t st);
hipError_t launch_edge_sort(lc_ap_edge *src, lc_ap_edge *dst, int64_t n, int64_t *d_count, void *temp,
                            size_t temp_bytes, hipStream_t st);

// Real time's arrays on the device, n_txns entries each: the results byc
// (n_ok of them), rt_lo and rt_hi, and four the passes hand one another.
struct RtArrays {
  int32_t *ok_idx, *ok_comp, *byc, *comp_sorted, *pm, *rt_lo, *rt_hi;
  template <class Carver>
  void carve(Carver &ws, size_t nt) {
    int32_t *p = ws.template take<int32_t>(7 * nt);  // one array of the arena
    for (int32_t **a : {&ok_idx, &ok_comp, &byc, &comp_sorted, &pm, &rt_lo, &rt_hi}) {
      *a = p;
      if (p) p += nt;
    }
  }
};
size_t rt_temp_bytes(int64_t n_txns);
// d_count is one scratch word.
hipError_t launch_real_time(const lc_ap_txn *txns, int64_t n_txns, int64_t n_ok, const RtArrays &rt, int64_t *d_count,
                            void *temp, size_t temp_bytes, hipStream_t st);
#endif

}  // namespace lctg
