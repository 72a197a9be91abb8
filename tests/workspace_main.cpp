// workspace_main.cpp — csrc/workspace.h on its own (tests/test_workspace.py
// builds this with g++ and the address and undefined-behaviour sanitizers).
// A layout of the append driver's shape is run as the drivers run theirs:
// once over a null base for the size, once over an allocation of that size.
// Every array is then filled with a byte of its own and read back, and one
// line per array goes to stdout for the test to judge:
//   <name> <count> <element bytes> <offset, sizing pass> <offset, binding pass> <null in the sizing pass>
// and at the end "total <sizing pass> <binding pass>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../jepsen/etcd_amd/csrc/workspace.h"

namespace {

struct Edge {
  int32_t from, to, type, pad;
  int64_t key;
};
struct Txn {
  int64_t mop_off;
  int32_t inv_pos, comp_pos, type, mop_len;
};

// The kernels' view: typed pointers, the inputs const.
struct Ws {
  const Txn *txns;
  const Edge *mops;
  const int64_t *values;
  const int32_t *mop_txn, *rd_mop, *txn_r0;
  const int64_t *work_off;
  unsigned long long *wtab;
  int32_t *stamp;
  int64_t *ktab;
  unsigned long long *kbest;
  int32_t *kfirst, *kflags, *mop_kslot;
  uint8_t *mop_last;
  int32_t *ord_w;
  uint8_t *nonprefix;
  int32_t *mop_flags, *txn_flags;
  Edge *slots, *keys;
  int64_t *counters;
  int32_t *status;
};
struct Beside {  // the pointers a driver passes beside its Ws
  int32_t *kslots, *rt;
  int64_t *count;
  void *temp;
  Edge *edges_a, *edges_b;
};

struct Row {
  std::string name;
  size_t count, elem, off;
  const void *p;
};

struct Sizes {
  size_t nt, nm, nr, n_work, n_values, wcap, kcap, n_slots, n_room, temp;
};

// The layout, written once.  `rows` notes what each take() was asked and gave.
size_t layout(lcrt::Carver ws, const Sizes &z, Ws &w, Beside &b, std::vector<Row> &rows) {
#define TAKE(dst, T, n)                                         \
  do {                                                          \
    const size_t at_ = ws.size;                                 \
    dst = ws.take<T>(n);                                        \
    rows.push_back(Row{#dst, (size_t)(n), sizeof(T), at_, dst}); \
  } while (0)
  TAKE(w.txns, Txn, z.nt);
  TAKE(w.mops, Edge, z.nm);
  TAKE(w.values, int64_t, z.n_values);
  TAKE(w.work_off, int64_t, z.nr + 1);
  TAKE(w.mop_txn, int32_t, z.nm);
  TAKE(w.rd_mop, int32_t, z.nr);
  TAKE(w.txn_r0, int32_t, z.nt + 1);
  TAKE(w.wtab, unsigned long long, z.wcap);
  TAKE(w.stamp, int32_t, z.wcap);
  TAKE(w.ktab, int64_t, z.kcap);
  TAKE(w.kbest, unsigned long long, z.kcap);
  TAKE(w.kfirst, int32_t, 3 * z.kcap);
  TAKE(w.kflags, int32_t, z.kcap);
  TAKE(w.mop_kslot, int32_t, z.nm);
  TAKE(w.mop_last, uint8_t, z.nm);
  TAKE(w.ord_w, int32_t, z.n_work);
  TAKE(w.nonprefix, uint8_t, z.nr);
  TAKE(w.mop_flags, int32_t, z.nm);
  TAKE(w.txn_flags, int32_t, z.nt);
  TAKE(w.slots, Edge, z.n_slots);
  TAKE(b.edges_a, Edge, z.n_room);
  TAKE(b.edges_b, Edge, z.n_room);
  TAKE(b.kslots, int32_t, z.kcap);
  TAKE(w.keys, Edge, z.nm);
  TAKE(w.counters, int64_t, 6 * 32 * 16);
  TAKE(b.count, int64_t, 4);
  TAKE(w.status, int32_t, 4);
  TAKE(b.rt, int32_t, 7 * z.nt);
  TAKE(b.temp, uint8_t, z.temp);
#undef TAKE
  return ws.size;
}

int run(const Sizes &z) {
  Ws w{}, w0{};
  Beside b{}, b0{};
  std::vector<Row> sizing, binding;
  const size_t total = layout(lcrt::Carver{}, z, w0, b0, sizing);
  char *base = static_cast<char *>(aligned_alloc(256, total));  // (total is a multiple of 256)
  if (!base) return 2;
  const size_t total2 = layout(lcrt::Carver{base}, z, w, b, binding);
  if (sizing.size() != binding.size()) return 3;
  // every array filled to the extent it was promised: max(count * element, 256) bytes ...
  for (size_t i = 0; i < binding.size(); i++) {
    const Row &r = binding[i];
    memset(const_cast<void *>(r.p), (int)(i + 1), std::max<size_t>(r.count * r.elem, 256));
  }
  // ... and none of them reached into another
  for (size_t i = 0; i < binding.size(); i++) {
    const Row &r = binding[i];
    const unsigned char *q = static_cast<const unsigned char *>(r.p);
    const size_t n = std::max<size_t>(r.count * r.elem, 256);
    for (size_t j = 0; j < n; j++)
      if (q[j] != (unsigned char)(i + 1)) {
        fprintf(stderr, "%s: byte %zu overwritten\n", r.name.c_str(), j);
        return 4;
      }
  }
  for (size_t i = 0; i < binding.size(); i++)
    printf("%s %zu %zu %zu %zu %d\n", binding[i].name.c_str(), binding[i].count, binding[i].elem, sizing[i].off,
           (size_t)(static_cast<const char *>(binding[i].p) - base), sizing[i].p == nullptr);
  printf("total %zu %zu\n", total, total2);
  free(base);
  return 0;
}

}  // namespace

int main() {
  // a call with txns, mops, reads and a payload (odd counts), then one without
  // mops: nm, nr, n_work, n_values, n_slots all 0
  const Sizes full{301, 1237, 77, 5003, 5003, 2048, 4096, 2 * 77 + 5003, 2 * 77 + 611, 70001};
  const Sizes bare{3, 0, 0, 0, 0, 64, 64, 0, 0, 1};
  if (int rc = run(full)) return rc;
  printf("next\n");
  return run(bare);
}
