// plan_main.cpp — csrc/plan_host.h and plan_host.cpp on their own
// (tests/test_plan_host.py builds this with g++ and the address and
// undefined-behaviour sanitizers): lc_check's chunk plan and device split,
// the 24- and 16-byte packers, and the counted classes.  One line per case
// goes to stdout for the test to judge:
//   const kChunkBytes kChunkTail kMaxChunks kKeyStride kSampleStride
//   chunks <case> <record bytes> <nk> <n> k <k[0..n]> r <r[0..n]> want <off[k[i]] - off[0]>
//   devices <case> <record bytes> <nd> <n_keys> bounds <bounds[0..nd]> len <key lengths>
//   pack <case> <width> <rc> <records> <records that widen back to themselves>
//   counted <case> rc <rc> n_classes <n> fits <plan.fits> take <take> plan <value:members ...> host <value:members ...>
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../jepsen/etcd_amd/csrc/plan_host.cpp"

namespace {

void chunks_case(const char *name, size_t rec, const std::vector<int64_t> &off) {
  const int64_t nk = (int64_t)off.size() - 1;
  ChunkPlan ch;
  plan_chunks(off.data(), nk, rec, ch);
  printf("chunks %s %zu %lld %d k", name, rec, (long long)nk, ch.n);
  for (int64_t k : ch.k) printf(" %lld", (long long)k);
  printf(" r");
  for (int64_t r : ch.r) printf(" %lld", (long long)r);
  printf(" want");
  for (int64_t k : ch.k) printf(" %lld", (long long)(k >= 0 && k <= nk ? off[(size_t)k] - off[0] : -1));
  printf("\n");
}

// Offsets of keys of `len` records each over `records` records (the last key
// takes the remainder), from first record `r0`, with `lead` and `trail`
// empty keys around them.
std::vector<int64_t> uniform(int64_t records, int64_t len, int64_t r0 = 0, int lead = 0, int trail = 0) {
  std::vector<int64_t> off(1 + (size_t)lead, r0);
  for (int64_t r = 0; r < records;) {
    r = std::min(records, r + len);
    off.push_back(r0 + r);
  }
  for (int i = 0; i < trail; i++) off.push_back(off.back());
  return off;
}

void all_chunks(size_t rec) {
  chunks_case("one_key", rec, {7, 107});
  chunks_case("all_empty", rec, {5, 5, 5, 5, 5, 5});
  const int64_t tail = (int64_t)(kChunkTail / rec);  // (whole records: 2 MiB is no multiple of 24 or 48)
  chunks_case("tail_minus", rec, uniform(tail - 1, 100));
  chunks_case("tail", rec, uniform(tail, 100, 1000));
  chunks_case("tail_plus", rec, uniform(tail + 1, 100));
  chunks_case("max_chunks", rec, uniform((int64_t)((size_t(1200) << 20) / rec), 1 << 12, 3));
  chunks_case("empty_ends", rec, uniform((int64_t)((size_t(60) << 20) / rec), 5000, 11, 3, 4));
}

lc_op op(int64_t f, int64_t value, int64_t expected, int64_t version, int64_t call, int64_t ret) {
  return lc_op{f, value, expected, version, call, ret};
}

// n_keys clean version-pinned keys of lengths 10 + (7 k) % 23, except key
// `odd` (if >= 0), whose first record is a crashed write.
template <class Op>
void devices_case(const char *name, int nd, int64_t n_keys, int64_t odd) {
  std::vector<int64_t> off(1, 0);
  std::vector<lc_op> wide;
  for (int64_t k = 0; k < n_keys; k++) {
    const int64_t n = 10 + (7 * k) % 23;
    for (int64_t i = 0; i < n; i++) {
      const int64_t t = 10 * (int64_t)wide.size();
      wide.push_back(k == odd && i == 0 ? op(LC_F_WRITE, 3, LC_NIL, LC_NIL, t, LC_INF)
                                        : op(LC_F_WRITE, i % 5, LC_NIL, i + 1, t, t + 5));
    }
    off.push_back((int64_t)wide.size());
  }
  std::vector<Op> ops(wide.size());
  std::vector<int64_t> base((size_t)n_keys);
  if (sizeof(Op) == sizeof(lc_op)) {
    memcpy(static_cast<void *>(ops.data()), wide.data(), wide.size() * sizeof(lc_op));
  } else if (lc_pack32(wide.data(), off.data(), n_keys, reinterpret_cast<lc_op32 *>(ops.data()), base.data())) {
    printf("devices %s pack failed\n", name);
    return;
  }
  std::vector<int64_t> bounds((size_t)nd + 1, -7);
  plan_devices(ops.data(), off.data(), n_keys, nd, bounds.data());
  printf("devices %s %zu %d %lld bounds", name, sizeof(Op), nd, (long long)n_keys);
  for (int64_t b : bounds) printf(" %lld", (long long)b);
  printf(" len");
  for (int64_t k = 0; k < n_keys; k++) printf(" %lld", (long long)(off[(size_t)k + 1] - off[(size_t)k]));
  printf("\n");
}

template <class Op>
void all_devices() {
  devices_case<Op>("nd1", 1, 100, -1);
  devices_case<Op>("nd2", 2, 100, -1);
  devices_case<Op>("nd8", 8, 100, -1);
  devices_case<Op>("more_devices_than_keys", 8, 3, -1);
  devices_case<Op>("irregular_at_0", 4, 100, 0);
  devices_case<Op>("irregular_unprobed", 4, 100, kKeyStride + 5);
}

bool same(const lc_op &a, const lc_op &b) {
  return a.f == b.f && a.value == b.value && a.expected == b.expected && a.version == b.version &&
         a.call == b.call && a.ret == b.ret;
}

// Three keys, the middle one empty; the last holds a crashed op and ids at
// `top`.  Both packers, and every record widened back.
void pack_case(const char *name, int64_t top) {
  std::vector<lc_op> ops = {
      op(LC_F_WRITE, 1, LC_NIL, 1, 1000, 1004),  op(LC_F_READ, 1, LC_NIL, 1, 1002, 1010),
      op(LC_F_CAS, 2, 1, 2, 1011, 1020),         op(LC_F_WRITE, top, LC_NIL, 1, 5000, 5003),
      op(LC_F_CAS, 4, top, LC_NIL, 5001, LC_INF), op(LC_F_READ, LC_NIL, LC_NIL, LC_NIL, 5002, LC_INF),
      op(LC_F_READ, top, LC_NIL, 1, 5004, 5009)};
  const std::vector<int64_t> off = {0, 3, 3, 7};
  const int64_t n_keys = 3;
  std::vector<int64_t> base((size_t)n_keys, -1);
  std::vector<lc_op32> q32(ops.size());
  int rc = lc_pack32(ops.data(), off.data(), n_keys, q32.data(), base.data());
  int back = 0;
  for (int64_t k = 0; k < n_keys && !rc; k++)
    for (int64_t i = off[(size_t)k]; i < off[(size_t)k + 1]; i++)
      back += same(widen_op(q32[(size_t)i], base[(size_t)k]), ops[(size_t)i]);
  printf("pack %s 32 %d %zu %d\n", name, rc, ops.size(), back);
  std::vector<lc_op16> q16(ops.size());
  rc = lc_pack16(ops.data(), off.data(), n_keys, q16.data(), base.data());
  back = 0;
  for (int64_t k = 0; k < n_keys && !rc; k++)
    for (int64_t i = off[(size_t)k]; i < off[(size_t)k + 1]; i++)
      back += same(widen_op(q16[(size_t)i], base[(size_t)k]), ops[(size_t)i]);
  printf("pack %s 16 %d %zu %d\n", name, rc, ops.size(), back);
  bool inf = q32[4].ret == LC_INF32 && q32[5].ret == LC_INF32 && q32[3].ret != LC_INF32;
  printf("pack %s inf32 %d 1 %d\n", name, 0, (int)inf);
}

// A key of n_classes classes of crashed writes (class i: value i + 1, 1 +
// i % 3 members, interleaved) and an :ok read to stop at.
void counted_case(const char *name, int n_classes) {
  std::vector<lc_op> ops;
  for (int round = 0; round < 3; round++)
    for (int i = 0; i < n_classes; i++)
      if (round <= i % 3) ops.push_back(op(LC_F_WRITE, i + 1, LC_NIL, LC_NIL, 10 * (int64_t)ops.size(), LC_INF));
  ops.push_back(op(LC_F_READ, 1, LC_NIL, LC_NIL, 10 * (int64_t)ops.size(), 10 * (int64_t)ops.size() + 5));
  const int64_t n = (int64_t)ops.size();
  lc_counted_layout lay;
  const int rc = lc_counted_plan(ops.data(), n, &lay);
  const CountedKey ck = counted_classes_of(ops.data(), n, n - 1);
  printf("counted %s rc %d n_classes %d fits %d take %d plan", name, rc, lay.n_classes, lay.fits, (int)ck.take);
  for (int k = 0; k < std::min<int>(lay.n_classes, LC_COUNTED_MAX_CLASSES); k++)
    printf(" %lld:%lld", (long long)lay.value[k], (long long)lay.members[k]);
  printf(" host");
  for (const auto &m : ck.members) printf(" %lld:%zu", (long long)ops[(size_t)m[0]].value, m.size());
  printf("\n");
}

}  // namespace

int main() {
  printf("const %zu %zu %d %lld %lld\n", kChunkBytes, kChunkTail, kMaxChunks, (long long)kKeyStride,
         (long long)kSampleStride);
  for (size_t rec : {sizeof(lc_op16), sizeof(lc_op32), sizeof(lc_op)}) all_chunks(rec);
  all_devices<lc_op>();
  all_devices<lc_op32>();
  pack_case("ids_at_max", LC_ID15_MAX);
  pack_case("ids_past_max", LC_ID15_MAX + 1);
  printf("pack no_keys 32 %d 0 0\n", lc_pack32(nullptr, nullptr, 0, nullptr, nullptr));
  printf("pack no_keys 16 %d 0 0\n", lc_pack16(nullptr, nullptr, 0, nullptr, nullptr));
  counted_case("classes16", 16);
  counted_case("classes17", 17);
  return 0;
}
