// plan_host.h — the register path's host arithmetic: what a record of any
// width says (rec_kind), what a key costs, lc_check's split over its devices
// and its chunk plan, and the counted classes of a key's crashed writes/CAS.
// Host-only, nothing of HIP: plan_host.cpp (the exported planners and
// packers) reads it as plain C++, and tests/plan_main.cpp compiles both
// with g++.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <thread>
#include <vector>

#include "../../../include/lincheck.h"
#include "counted.h"

namespace lcrt __attribute__((visibility("hidden"))) {

// Per-key device cost in record-scan units.  The tier a key
// lands in follows from its records alone (check_kernel.hip, fast_key):
//   * version-order tier (every :ok mutation versioned, nothing crashed):
//     one pass over the records, cost n;
//   * gap tier (crashed writes/CAS, versions pinned): two skeleton passes,
//     the matching and, for an invalid key, the bisection; measured ~6x the
//     fast tier per record on C2 with 5 % crashed ops (crash_leg), plus the
//     matching's share, which grows with the crashed ops;
//   * frontier search (an :ok mutation or a read [nil x] without a version):
//     the frontier grows with the open window w; measured (model_leg,
//     tools/frontier_dist.py) ~1,600x the fast tier per record at
//     concurrency 10 and ~4,700x at 20, i.e. ~12 w^2, and crashed ops
//     multiply the configurations (capped: the search's budget bounds it).
// Plus a fixed 64 per key (launch share, result write).
// (Records of either width: lc_op, or lc_op32 with LC_INF32 for LC_INF.)
inline bool rec_crashed(const lc_op32 &o) { return o.ret == LC_INF32; }
inline int64_t rec_call(const lc_op &o) { return o.call; }
inline int64_t rec_call(const lc_op32 &o) { return (int64_t)o.call; }
inline int64_t rec_ret(const lc_op &o) { return o.ret; }
inline int64_t rec_ret(const lc_op32 &o) { return o.ret == LC_INF32 ? LC_INF : (int64_t)o.ret; }
// a crashed write/CAS, or an :ok op without a version that the version order
// cannot pin (a mutation, or a read of a value)
template <class Op>
inline void rec_kind(const Op &o, bool *crashed_mut, bool *unpinned) {
  const bool mut = o.f == LC_F_WRITE || o.f == LC_F_CAS;
  *crashed_mut = mut && rec_crashed(o);
  *unpinned = !rec_crashed(o) && o.version == (int32_t)LC_NIL &&
              (mut || (o.f == LC_F_READ && o.value != (int32_t)LC_NIL));
}
inline void rec_kind(const lc_op &o, bool *crashed_mut, bool *unpinned) {
  const bool mut = o.f == LC_F_WRITE || o.f == LC_F_CAS;
  *crashed_mut = mut && o.ret == LC_INF;
  *unpinned = o.ret != LC_INF && o.version == LC_NIL &&
              (mut || (o.f == LC_F_READ && o.value != LC_NIL));
}

// An lc_op16 record as the lc_op32 it stands for (include/lincheck.h)
inline lc_op32 as32(const lc_op16 &q) {
  const uint32_t v = q.fve >> 15 & 0x7FFFu, x = q.fve & 0x7FFFu;
  return lc_op32{(int32_t)(q.fve >> 30), v == 0x7FFFu ? -2 : (int32_t)v - 1,
                 x == 0x7FFFu ? -2 : (int32_t)x - 1, q.version, q.call, q.ret};
}
inline int64_t rec_call(const lc_op16 &o) { return (int64_t)o.call; }
inline int64_t rec_ret(const lc_op16 &o) { return o.ret == LC_INF32 ? LC_INF : (int64_t)o.ret; }
inline void rec_kind(const lc_op16 &o, bool *crashed_mut, bool *unpinned) {
  rec_kind(as32(o), crashed_mut, unpinned);
}

// An lc_op32 record as the lc_op it stands for (include/lincheck.h, ABI 4).
inline lc_op widen_op(const lc_op &o, int64_t) { return o; }
inline lc_op widen_op(const lc_op32 &o, int64_t base) {
  return lc_op{o.f, o.value, o.expected, o.version, base + (int64_t)o.call,
               o.ret == LC_INF32 ? LC_INF : base + (int64_t)o.ret};
}
inline lc_op widen_op(const lc_op16 &o, int64_t base) { return widen_op(as32(o), base); }

template <class Op>
double key_cost(const Op *o, int64_t n) {
  int64_t crashed = 0, unpinned = 0;
  for (int64_t i = 0; i < n; i++) {
    bool cm, un;
    rec_kind(o[i], &cm, &un);
    crashed += cm;
    unpinned += un;
  }
  const double kOverhead = 64;
  if (!unpinned && !crashed) return (double)n + kOverhead;
  if (!unpinned) return (6.0 + 0.01 * (double)crashed) * (double)n + kOverhead;
  // open window: the most ops called and not yet returned at once
  std::vector<int64_t> rets;
  rets.reserve((size_t)n);
  for (int64_t i = 0; i < n; i++) rets.push_back(rec_ret(o[i]));
  std::sort(rets.begin(), rets.end());
  int64_t w = 0;
  size_t j = 0;
  for (int64_t i = 0; i < n; i++) {  // records are sorted by call
    while (j < rets.size() && rets[j] < rec_call(o[i])) j++;
    w = std::max<int64_t>(w, i + 1 - (int64_t)j);
  }
  const double blow = std::pow(2.0, (double)std::min<int64_t>(crashed, 12));
  return (double)n * (1.0 + 12.0 * (double)w * (double)w) * blow + kOverhead;
}

// lc_check's own split over its devices: the same contiguous equal-cost cut
// as lc_plan_partition, but a key is priced by all its records only when a
// sample of them (every kSampleStride-th) shows it is not a clean
// version-pinned key (a crashed write/CAS, an :ok op without a version);
// otherwise it costs its record count, which is what lc_key_cost gives a
// clean key.  And the sample itself is taken only when a first probe — the
// same sample of every kKeyStride-th key — finds an irregular key: a batch
// whose probe is clean is split by record count.  Pricing every record read
// the whole batch on the host (480 MB for C2: several ms even on 16 threads)
// before any copy could start; sampling every key still touched every page
// (0.6-0.9 ms of a 5-ms call on the GPU box, tools/plan_probe.cpp); the
// probe reads ~1/16 of them.  Only the split's balance, never a verdict,
// depends on these estimates.
constexpr int64_t kSampleStride = 64;
constexpr int64_t kKeyStride = 16;
template <class Op>
bool irregular_sample(const Op *o, int64_t n) {
  for (int64_t i = 0; i < n; i += kSampleStride) {
    bool cm, un;
    rec_kind(o[i], &cm, &un);
    if (cm || un) return true;
  }
  return false;
}

// fn(k0, k1) over the keys [0, n_keys), cut into nth contiguous ranges with
// a thread each (nth <= 1: on this thread).
template <class F>
void for_key_ranges(int64_t n_keys, int nth, F fn) {
  if (nth <= 1) return fn(0, n_keys);
  std::vector<std::thread> th;
  for (int t = 0; t < nth; t++) th.emplace_back(fn, n_keys * t / nth, n_keys * (t + 1) / nth);
  for (auto &x : th) x.join();
}

// The contiguous split at equal cost over a prefix-summed cost array (pre[0]
// = 0, pre[k + 1] = the cost of keys [0, k]): boundary p is the first key
// whose prefix reaches p/n_parts of the total.
inline void cut_at_equal_cost(const std::vector<double> &pre, int64_t n_keys, int n_parts, int64_t *bounds) {
  const double total = pre[(size_t)n_keys];
  bounds[0] = 0;
  int64_t k = 0;
  for (int p = 1; p < n_parts; p++) {
    const double goal = total * p / n_parts;
    while (k < n_keys && pre[(size_t)k] < goal) k++;
    bounds[p] = k;
  }
  bounds[n_parts] = n_keys;
}

template <class Op>
void plan_devices(const Op *ops, const int64_t *key_off, int64_t n_keys, int nd,
                  int64_t *bounds) {
  std::vector<double> pre((size_t)n_keys + 1, 0.0);
  bool any = false;
  for (int64_t k = 0; k < n_keys && !any; k += kKeyStride)
    any = irregular_sample(ops + key_off[k], key_off[k + 1] - key_off[k]);
  auto price = [&](int64_t k0, int64_t k1) {
    for (int64_t k = k0; k < k1; k++) {
      const Op *o = ops + key_off[k];
      const int64_t n = key_off[k + 1] - key_off[k];
      pre[(size_t)k + 1] = any && irregular_sample(o, n) ? key_cost(o, n) : (double)n + 64.0;
    }
  };
  const int nth = any ? (int)std::min<int64_t>(16, std::max<int64_t>(1, n_keys >> 10)) : 1;
  for_key_ranges(n_keys, nth, price);
  for (int64_t k = 0; k < n_keys; k++) pre[(size_t)k + 1] += pre[(size_t)k];
  cut_at_equal_cost(pre, n_keys, nd, bounds);
}

// lc_check's host-to-device pipeline cuts a device's key range into chunks
// of kChunkBytes, the last ones halving down to kChunkTail: the compute
// stream's tail after the last copy is one small chunk's widening and
// version-order pass.  (Measured on C2's 240 MB of 24-byte records: 10
// chunks of 24 MB 4.66 ms per call, 0.12 ms of it after the last copy; 29
// chunks of 8 MB 5.2 ms — each pageable copy has a fixed cost.)
constexpr size_t kChunkBytes = size_t(24) << 20;
constexpr size_t kChunkTail = size_t(2) << 20;
constexpr int kMaxChunks = 48;
struct ChunkPlan {
  int n = 0;
  std::vector<int64_t> k;  // key boundaries, n + 1, local to the device's range
  std::vector<int64_t> r;  // record offsets of those keys from the range's first record
};

// The chunks of nk keys with offsets off[0..nk], records of rec_bytes:
// contiguous key ranges of about kChunkBytes of input records, the last ones
// halving down to kChunkTail (cut at key boundaries).  Fills ch.n, ch.k, ch.r.
inline void plan_chunks(const int64_t *off, int64_t nk, size_t rec_bytes, ChunkPlan &ch) {
  const int64_t r0 = off[0];
  const size_t in_bytes = rec_bytes * (size_t)(off[nk] - r0);
  std::vector<size_t> sizes;  // from the end of the range
  size_t sum = 0;
  for (size_t left = in_bytes, want = kChunkTail; left > 0 && (int)sizes.size() < kMaxChunks - 1;) {
    const size_t take = std::min(left, want);
    sizes.push_back(take);
    sum += take;
    left -= take;
    want = std::min(kChunkBytes, 2 * want);
  }
  ch.k.assign(1, 0);
  int64_t rec_goal = (int64_t)((in_bytes - sum) / rec_bytes);  // records before the next cut
  for (size_t i = sizes.size(); i-- > 1;) {
    rec_goal += (int64_t)(sizes[i] / rec_bytes);
    const int64_t k = std::lower_bound(off, off + nk, r0 + rec_goal) - off;
    if (k > ch.k.back() && k < nk) ch.k.push_back(k);
  }
  ch.k.push_back(nk);
  ch.n = (int)ch.k.size() - 1;
  ch.r.clear();
  for (int64_t k : ch.k) ch.r.push_back(off[k] - r0);
}

// The device's decoding (records.h, decode) of a 48-byte record of a key
// whose first call is `base` reads it as malformed: a field outside what 32
// bits hold.  (lc_pack32 / lc_pack16 mark such a record; the counted
// frontiers leave its key out.)
inline bool rec_malformed(const lc_op &o, int64_t base) {
  constexpr int64_t kFieldMax = 0x7FFFFFFE, kNever = 0xFFFFFFFFll;
  const int64_t rc = o.call - base, rr = o.ret - base;
  return o.value < -1 || o.value > kFieldMax || o.expected < -1 || o.expected > kFieldMax ||
         o.call < 0 || o.ret <= o.call || rc < 0 || rc >= kNever || (o.ret != LC_INF && rr >= kNever);
}

// The counted classes (counted.h): a crashed write/CAS record's class is its
// (f, value, expected, version as the device reads it).  class_of returns the
// index of o's class in cls, in order of first call, adding it when new:
// lc_counted_plan and counted_classes_of cut a key's classes through it, so
// identically.
struct CrashClass {
  int64_t f, value, expected, version;
};
inline bool crashed_mutation(const lc_op &o) {
  return (o.f == LC_F_WRITE || o.f == LC_F_CAS) && o.ret == LC_INF;
}
inline size_t class_of(std::vector<CrashClass> &cls, const lc_op &o) {
  const int64_t ver = lccount::counted_version(o.version);
  size_t ci = 0;
  while (ci < cls.size() && !(cls[ci].f == o.f && cls[ci].value == o.value &&
                              cls[ci].expected == o.expected && cls[ci].version == ver))
    ci++;
  if (ci == cls.size()) cls.push_back(CrashClass{o.f, o.value, o.expected, ver});
  return ci;
}

// One key of lc_check_frontiers_counted on the host: whether the device may
// search it, and each class's members (record indices, in record order).
// The classes are lc_counted_plan's, cut as the device cuts them: a key with
// a record the device reads as malformed (records.h decode) is left out, so
// every field the classes compare is the same number on both sides.
struct CountedKey {
  bool take = false;
  std::vector<std::vector<int32_t>> members;
};
inline CountedKey counted_classes_of(const lc_op *k, int64_t n, int64_t stop) {
  CountedKey ck;
  if (n <= 0 || n > INT32_MAX || stop < 0 || stop >= n || k[stop].ret == LC_INF) return ck;
  std::vector<CrashClass> cls;
  for (int64_t i = 0; i < n; i++) {
    if (rec_malformed(k[i], k[0].call)) return ck;
    if (!crashed_mutation(k[i])) continue;
    const size_t ci = class_of(cls, k[i]);
    if (ci == (size_t)LC_COUNTED_MAX_CLASSES) return ck;
    if (ci == ck.members.size()) ck.members.emplace_back();
    ck.members[ci].push_back((int32_t)i);
  }
  int bits = 0;
  for (const auto &m : ck.members) bits += lccount::counted_width((int64_t)m.size());
  const int ncls = (int)ck.members.size();
  ck.take = lccount::counted_fits(ncls, lccount::counted_slots(bits, ncls));
  return ck;
}

}  // namespace lcrt
