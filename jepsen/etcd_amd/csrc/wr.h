// wr.h — what lc_wr_check's host code (wr_host.cpp, g++), its driver
// (wr_dev.cpp) and its kernels (wr.hip) share.  The rules are
// include/lincheck_wr.h's.  The (key, value) hash, the table sizing, the
// sharded counters' geometry, the item chunk, and the key-slot, edge select /
// sort / unique and real-time launchers are txngraph.h's, which
// lc_append_check shares.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../../include/lincheck_wr.h"
#include "graph_host.h"
#include "txngraph.h"

namespace lcwr {

using namespace lctg;  // the hash, the limits and the launchers both Elle checkers share

constexpr int64_t kReserved = INT64_MIN;  // no key; as a value, nil
constexpr int64_t kDefaultMaxEdges = int64_t(1) << 27;
constexpr int kCounters = 5;  // internal, phantom, g1a, g1b, lost-update versions

// What one pass over the input gives the host (wr_host.cpp, prepare): the
// contract checked, and each mop's txn.
struct Prep {
  std::vector<int32_t> mop_txn;  // n_mops
  int64_t n_ok = 0, n_nodes = 0;
};

// 0 or -EINVAL with the text in err (everything but two writes of one pair).
int prepare(const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops, uint32_t flags,
            const lc_wr_out *out, Prep *p, const char **err);

// Rules 9 and 10 over finished flags, keys, edges and ranges: out->scc,
// scc_class, steps, cycle_off, cycle_scc, and every field of sum but
// n_edges_raw and the device times.  counts[kCounters] are the read counts
// and the lost-update versions.
// no_scc: the caller knows of no nontrivial SCC, and rule 9 only fills.  mp: rule 9 runs over the marked txns
// (cycles_host_marked); its error, the hook's, is returned and *sum is then not written.  0 otherwise.
int graph_and_summary(const lc_wr_txn *txns, int64_t n_txns, const Prep &p, const lc_wr_out *out, int64_t n_keys,
                      int64_t n_edges, const int64_t *counts, lc_wr_summary *sum,
                      bool no_scc = false, lcgraph::MarkedPass *mp = nullptr);

#if defined(__HIPCC__)
// One call's device workspace.
struct Ws {
  const lc_wr_txn *txns;
  const lc_wr_mop *mops;
  const int32_t *mop_txn;
  int64_t n_txns, n_mops;
  uint32_t flags;
  // the version table over (key, value), nil included once it is read: a
  // word is (tag << 32) | a mop that names the pair, ~0 when empty
  unsigned long long *vtab;
  uint64_t vcap;
  int32_t *vwriter;   // the pair's write mop, -1: none
  int32_t *vnread;    // external readers (rule 2)
  int32_t *vnrw;      // of them, those whose txn writes the key (rule 5)
  int32_t *vnchild;   // children: version edges out of the entry
  int32_t *ptr_a, *ptr_b;  // rule 6's pointers (the wfr parent's slot, -1: a root), doubled from one to the other
  int32_t *rd_off, *ch_off;  // vcap + 1: the groups' offsets into readers / children
  int32_t *rd_cur, *ch_cur;  // the fill's cursors
  int64_t *rc;               // vcap + 1: readers x children per slot (0 under a cyclic key); rc[vcap] stays 0
  int64_t *item_off;         // vcap + 1: rc's prefix sums; item_off[vcap] is the number of rw items
  int32_t *readers;   // grouped by version: the reading txns (n_mops at most)
  int32_t *children;  // grouped by version: the child versions' write mops (2 n_mops at most)
  // the key table, as lc_append_check's: the key stored xor 2^63 - 1
  int64_t *ktab;
  uint64_t kcap;
  int32_t *kflags;    // LC_WR_K_*
  int32_t *kcount;    // 3 per slot: write mops, distinct non-nil values, external reads
  unsigned long long *kcyc;  // the least value on a cycle, xor 2^63 (unsigned order is int64's), ~0: none yet
  int32_t *mop_kslot, *mop_vslot;  // n_mops (vslot -1: an ignored read)
  uint8_t *mop_last;  // n_mops: rule 1's "last write to the key"
  int32_t *mop_par;   // n_mops: on a txn's external write, the slot of the wfr edge's tail (-1: no such edge)
  int32_t *mop_nil;   // n_mops: on a node txn's write, the slot of (key, nil) (-1: nobody read nil)
  int32_t *mop_flags, *txn_flags;
  lc_wr_edge *slots;  // n_mops wr / ww slots (by mop), then the rw items'; from = -1 when empty
  lc_wr_key *keys;    // compacted key records (slot order; the host sorts them)
  int64_t *counters;  // kCounters x kCounterShards x kCounterStride
  int32_t *status;    // [0] two writes of one pair, [1] one such mop
};

size_t scan_temp_bytes(uint64_t vcap, uint64_t kcap);
// Tables, the txn pass, rule 6 in `rounds` doublings, the groups and their
// prefix sums (item_off[vcap] is the number of rw items), the ww slots and the
// key records.  kslots has kcap entries; *d_n_keys receives the key count;
// temp has scan_temp_bytes(vcap, kcap).
hipError_t launch_rules(const Ws &w, int rounds, int32_t *kslots, int64_t *d_n_keys, void *temp, size_t temp_bytes,
                        hipStream_t st);
// The rw slots: n_items work items into slots[n_mops ..].
hipError_t launch_items(const Ws &w, int64_t n_items, hipStream_t st);
#endif

}  // namespace lcwr
