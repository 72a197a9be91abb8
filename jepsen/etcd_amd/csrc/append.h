// append.h — what lc_append_check's host code (append_host.cpp, g++) and its
// kernels (append.hip) share: the host's preparation pass, the host parts of
// the device call, and the kernels' workspace and launcher.  The rules are
// include/lincheck_append.h's; what lc_wr_check shares with them is
// txngraph.h's.
#pragma once
#include <stdint.h>

#include <vector>

#include "graph_host.h"
#include "txngraph.h"

namespace lcap {

using namespace lctg;  // the hash, the limits and the launchers both Elle checkers share

constexpr int64_t kReserved = INT64_MIN;        // no key and no appended element
constexpr int64_t kDefaultMaxPayload = int64_t(1) << 30;
constexpr int kCounters = 6;                    // duplicate, g1a, phantom, g1b, internal, slow reads

// The longest-read word of a key: (len, ~read ordinal), larger is better;
// 0: never read.
LCTG_HD uint64_t pack_best(int32_t len, int32_t r) { return ((uint64_t)(uint32_t)len << 32) | (uint32_t)~r; }
LCTG_HD int32_t best_read(uint64_t b) { return (int32_t)~(uint32_t)b; }
LCTG_HD int32_t best_len(uint64_t b) { return (int32_t)(b >> 32); }

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
// no_scc: the caller knows of no nontrivial SCC, and rule 7 only fills.  mp: rule 7 runs over the marked txns
// (cycles_host_marked); its error, the hook's, is returned and *sum is then not written.  0 otherwise.
int graph_and_summary(const lc_ap_txn *txns, int64_t n_txns, const Prep &p, const lc_ap_out *out, int64_t n_keys,
                      int64_t n_edges, int64_t n_nonprefix, const int64_t *counts, lc_ap_summary *sum,
                      bool no_scc = false, lcgraph::MarkedPass *mp = nullptr);

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
// pass, the ww slots and the key records: everything before the edge select.
// kslots has kcap entries; *d_n_keys receives the number of key records; temp
// has key_temp_bytes(kcap).
hipError_t launch_rules(const Ws &w, int32_t *kslots, int64_t *d_n_keys, void *temp, size_t temp_bytes,
                        hipStream_t st);
#endif

}  // namespace lcap
