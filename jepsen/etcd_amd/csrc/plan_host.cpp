// plan_host.cpp — the planners and packers of include/lincheck.h that need
// no GPU: lc_key_cost, lc_plan_partition, lc_pack32, lc_pack16 and
// lc_counted_plan, over plan_host.h.  Nothing of HIP; compiled by hipcc's clang
// as plain C++ (Makefile, HOST_CLANG), and by g++ under tests/plan_main.cpp.
#include <errno.h>

#include <atomic>

#include "plan_host.h"

using namespace lcrt;

namespace {

// How many threads price or pack a batch: each key reads its records once;
// 10M records (480 MB) is tens of ms on one thread, so large batches go over
// up to 16 threads.
int batch_threads(const int64_t *key_off, int64_t n_keys) {
  const int64_t n_rec = n_keys ? key_off[n_keys] - key_off[0] : 0;
  return (int)std::min<int64_t>(16, std::max<int64_t>(1, std::min<int64_t>(n_keys, n_rec >> 18)));
}

// lc_pack32 / lc_pack16's argument check.
int pack_args(const void *ops, const int64_t *key_off, int64_t n_keys, const void *out,
              const int64_t *key_base) {
  if (n_keys < 0 || (n_keys > 0 && (!ops || !key_off || !out || !key_base))) return -EINVAL;
  if (n_keys == 0) return 0;
  if (key_off[0] < 0) return -EINVAL;
  for (int64_t k = 0; k < n_keys; k++)
    if (key_off[k + 1] < key_off[k]) return -EINVAL;
  return 0;
}

// What both narrow widths keep of a record's version and times.
constexpr int64_t kFieldMax = 0x7FFFFFFE;
inline int32_t pack_version(const lc_op &o) {
  return o.version < -1 || o.version > kFieldMax ? (int32_t)kFieldMax : (int32_t)o.version;
}
// (a malformed record's return may land on LC_INF32 modulo 2^32: it stays a
// return, which is what the witness initialisation reads)
inline uint32_t pack_ret(const lc_op &o, int64_t base) {
  const int64_t rr = o.ret - base;
  return o.ret == LC_INF ? LC_INF32 : (uint32_t)rr == LC_INF32 ? LC_INF32 - 1 : (uint32_t)rr;
}

}  // namespace

extern "C" {

int lc_key_cost(const lc_op *ops, const int64_t *key_off, int64_t n_keys, double *costs) {
  if (!ops || !key_off || !costs || n_keys < 0) return -EINVAL;
  for (int64_t k = 0; k < n_keys; k++) {
    const int64_t n = key_off[k + 1] - key_off[k];
    if (n < 0) return -EINVAL;
    costs[k] = key_cost(ops + key_off[k], n);
  }
  return 0;
}

// Contiguous split at equal cost: boundary p is the first key whose cost
// prefix reaches p/n_parts of the total (keys stay in order, so each device
// gets one contiguous slice of the caller's arrays).
int lc_plan_partition(const lc_op *ops, const int64_t *key_off, int64_t n_keys,
                      int32_t n_parts, int64_t *bounds) {
  if (!key_off || !bounds || n_parts < 1 || n_keys < 0) return -EINVAL;
  for (int64_t k = 0; k < n_keys; k++)
    if (key_off[k + 1] < key_off[k]) return -EINVAL;
  std::vector<double> pre((size_t)n_keys + 1, 0.0);
  auto price = [&](int64_t k0, int64_t k1) {
    for (int64_t k = k0; k < k1; k++) {
      const int64_t n = key_off[k + 1] - key_off[k];
      pre[(size_t)k + 1] = ops ? key_cost(ops + key_off[k], n) : (double)n + 64.0;
    }
  };
  for_key_ranges(n_keys, ops ? batch_threads(key_off, n_keys) : 1, price);
  for (int64_t k = 0; k < n_keys; k++) pre[(size_t)k + 1] += pre[(size_t)k];
  cut_at_equal_cost(pre, n_keys, n_parts, bounds);
  return 0;
}

int lc_pack32(const lc_op *ops, const int64_t *key_off, int64_t n_keys, lc_op32 *out,
              int64_t *key_base) {
  if (int e = pack_args(ops, key_off, n_keys, out, key_base)) return e;
  if (n_keys == 0) return 0;
  // the device's decoding (records.h, decode) of a 48-byte record, applied
  // here: what it reads of each field fits 32 bits
  auto pack = [&](int64_t k0, int64_t k1) {
    for (int64_t k = k0; k < k1; k++) {
      const int64_t b = key_off[k], e = key_off[k + 1];
      const int64_t base = e > b ? ops[b].call : 0;
      key_base[k] = base;
      for (int64_t i = b; i < e; i++) {
        const lc_op &o = ops[i];
        lc_op32 &q = out[i];
        q.f = o.f >= 0 && o.f <= LC_F_CAS ? (int32_t)o.f : 3;
        q.value = rec_malformed(o, base) ? -2 : (int32_t)o.value;  // -2: malformed, in either width
        q.expected = (int32_t)o.expected;
        q.version = pack_version(o);
        q.call = (uint32_t)(o.call - base);
        q.ret = pack_ret(o, base);
      }
    }
  };
  for_key_ranges(n_keys, batch_threads(key_off, n_keys), pack);
  return 0;
}

int lc_pack16(const lc_op *ops, const int64_t *key_off, int64_t n_keys, lc_op16 *out,
              int64_t *key_base) {
  if (int e = pack_args(ops, key_off, n_keys, out, key_base)) return e;
  if (n_keys == 0) return 0;
  // lc_pack32's narrowing, then the ids into 15 bits (a record it marks
  // malformed: value field 0x7FFF, its expected field clamped — the device
  // reads nothing else of a malformed key's records)
  std::atomic<bool> range{true};
  auto pack = [&](int64_t k0, int64_t k1) {
    for (int64_t k = k0; k < k1; k++) {
      const int64_t b = key_off[k], e = key_off[k + 1];
      const int64_t base = e > b ? ops[b].call : 0;
      key_base[k] = base;
      for (int64_t i = b; i < e; i++) {
        const lc_op &o = ops[i];
        const bool bad = rec_malformed(o, base);
        if (!bad && (o.value > LC_ID15_MAX || o.expected > LC_ID15_MAX)) {
          range.store(false, std::memory_order_relaxed);
          return;
        }
        const uint32_t f = o.f >= 0 && o.f <= LC_F_CAS ? (uint32_t)o.f : 3u;
        const uint32_t v = bad ? 0x7FFFu : (uint32_t)(o.value + 1);
        const uint32_t x = (uint32_t)std::min<int64_t>(0x7FFF, std::max<int64_t>(0, o.expected + 1));
        lc_op16 &q = out[i];
        q.fve = f << 30 | v << 15 | x;
        q.version = pack_version(o);
        q.call = (uint32_t)(o.call - base);
        q.ret = pack_ret(o, base);
      }
    }
  };
  for_key_ranges(n_keys, batch_threads(key_off, n_keys), pack);
  return range.load() ? 0 : -ERANGE;
}

int lc_counted_plan(const lc_op *ops, int64_t n, lc_counted_layout *out) {
  if (!out || n < 0 || (n > 0 && !ops)) return -EINVAL;
  *out = lc_counted_layout{};
  std::vector<CrashClass> cls;  // in order of first call (records are sorted by call)
  std::vector<int64_t> members;
  for (int64_t i = 0; i < n; i++) {
    if (!crashed_mutation(ops[i])) continue;
    const size_t ci = class_of(cls, ops[i]);
    if (ci == members.size()) members.push_back(0);
    members[ci]++;
  }
  int64_t bits = 0;
  for (size_t k = 0; k < cls.size(); k++) {
    const int w = lccount::counted_width(members[k]);
    bits += w;
    if (k < (size_t)LC_COUNTED_MAX_CLASSES) {
      out->f[k] = cls[k].f;
      out->value[k] = cls[k].value;
      out->expected[k] = cls[k].expected;
      out->version[k] = cls[k].version;
      out->members[k] = members[k];
      out->width[k] = w;
      out->shift[k] = (int32_t)(64 - bits);
    }
  }
  const int64_t ncls = (int64_t)cls.size();
  out->n_classes = (int32_t)std::min<int64_t>(ncls, INT32_MAX);
  out->field_bits = (int32_t)std::min<int64_t>(bits, INT32_MAX);
  // (beyond int: far from fitting either way)
  out->slots = (int32_t)std::max<int64_t>(std::min(64 - bits, 64 - ncls), INT32_MIN);
  out->fits = lccount::counted_fits(out->n_classes, out->slots);
  return 0;
}

}  // extern "C"
