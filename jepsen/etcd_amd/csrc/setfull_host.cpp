// setfull_host.cpp — lc_set_full_host: set-full's rules (include/
// lincheck_setfull.h) on the host, single-threaded; and the host parts of
// lc_set_full: the contract's check, the duplicates' exact count and the
// summary.  Compiled with g++: nothing here needs a GPU.
//
// The host function is jepsen's reduce over flat arrays: at every read it
// stamps the elements of the payload, then updates every element the read
// concerns as present or absent.  Its work is reads x elements plus the
// payload.
#include <errno.h>
#include <stdlib.h>

#include <chrono>
#include <new>
#include <vector>

#include "setfull.h"

namespace lcsf {

int check_contract(const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads, int64_t n_reads,
                   const int64_t *read_values, int64_t n_values, const char **err) {
  const char *dummy;
  if (!err) err = &dummy;
  if (n_adds < 0 || n_reads < 0 || n_values < 0 || (n_adds > 0 && !adds) || (n_reads > 0 && !reads) ||
      (n_values > 0 && !read_values)) {
    *err = "a null array or a negative count";
    return -EINVAL;
  }
  int64_t prev = -1;
  for (int64_t e = 0; e < n_adds; e++) {
    const lc_sf_add &a = adds[e];
    if (a.inv_pos < 0 || a.inv_pos >= kMaxPosition || a.ok_pos < -1 || a.ok_pos >= kMaxPosition) {
      *err = "an add's position outside [0, 2^31 - 1)";
      return -EINVAL;
    }
    if (a.inv_pos <= prev) {
      *err = "adds not strictly ascending by inv_pos";
      return -EINVAL;
    }
    if (a.ok_pos >= 0 && a.ok_pos <= a.inv_pos) {
      *err = "an add's ok_pos at or below its inv_pos";
      return -EINVAL;
    }
    if (a.value == kEmpty) {
      *err = "an add of the reserved value INT64_MIN";
      return -EINVAL;
    }
    prev = a.inv_pos;
  }
  prev = -1;
  for (int64_t r = 0; r < n_reads; r++) {
    const lc_sf_read &q = reads[r];
    if (q.inv_pos < 0 || q.ok_pos < 0 || q.ok_pos >= kMaxPosition) {
      *err = "a read's position outside [0, 2^31 - 1)";
      return -EINVAL;
    }
    if (q.inv_pos >= q.ok_pos) {
      *err = "a read's inv_pos at or above its ok_pos";
      return -EINVAL;
    }
    if (q.ok_pos <= prev) {
      *err = "reads not strictly ascending by ok_pos";
      return -EINVAL;
    }
    if (q.off < 0 || q.len < 0 || q.off > n_values || q.len > n_values - q.off) {
      *err = "a read's payload range outside read_values";
      return -EINVAL;
    }
    prev = q.ok_pos;
  }
  return 0;
}

void summarize(const lc_sf_element *out, int64_t n_adds, int32_t linearizable, lc_sf_summary *sum) {
  sum->linearizable = linearizable;
  sum->n_elements = n_adds;
  sum->n_stable = sum->n_lost = sum->n_never_read = sum->n_stale = sum->n_duplicated = 0;
  for (int64_t e = 0; e < n_adds; e++) {
    const lc_sf_element &o = out[e];
    if (o.outcome == LC_SF_STABLE) sum->n_stable++;
    else if (o.outcome == LC_SF_LOST) sum->n_lost++;
    else sum->n_never_read++;
    if (o.flags & LC_SF_STALE) sum->n_stale++;
    if (o.flags & LC_SF_DUPLICATED) sum->n_duplicated++;
  }
  if (sum->n_duplicated || sum->n_lost) sum->valid = 0;
  else if (!sum->n_stable) sum->valid = -1;
  else if (linearizable && sum->n_stale) sum->valid = 0;
  else sum->valid = 1;
}

namespace {

// value -> element, open addressing (the layout the device's table has).
struct Table {
  std::vector<int64_t> key;
  std::vector<int32_t> id;
  uint64_t cap = 0;

  explicit Table(int64_t n) : cap(table_capacity(n)) {
    key.assign(cap, kEmpty);
    id.assign(cap, -1);
  }
  // false: the value is there already
  bool insert(int64_t v, int32_t e) {
    uint64_t s = slot_of(v, cap);
    while (key[s] != kEmpty) {
      if (key[s] == v) return false;
      s = (s + 1) & (cap - 1);
    }
    key[s] = v;
    id[s] = e;
    return true;
  }
  int32_t find(int64_t v) const {
    if (v == kEmpty) return -1;
    uint64_t s = slot_of(v, cap);
    while (key[s] != kEmpty) {
      if (key[s] == v) return id[s];
      s = (s + 1) & (cap - 1);
    }
    return -1;
  }
};

}  // namespace

int count_duplicates(const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads, int64_t n_reads,
                     const int64_t *read_values, const uint8_t *marked, lc_sf_element *out) {
  try {
    int64_t n_marked = 0;
    for (int64_t e = 0; e < n_adds; e++) n_marked += marked[e] != 0;
    if (!n_marked) return 0;
    Table tab(n_marked);
    for (int64_t e = 0; e < n_adds; e++)
      if (marked[e]) tab.insert(adds[e].value, (int32_t)e);
    std::vector<int64_t> stamp((size_t)n_adds, -1);
    std::vector<int32_t> cnt((size_t)n_adds, 0);
    for (int64_t r = 0; r < n_reads; r++) {
      const lc_sf_read &q = reads[r];
      for (int64_t i = q.off; i < q.off + q.len; i++) {
        const int32_t e = tab.find(read_values[i]);
        if (e < 0 || q.ok_pos <= adds[e].inv_pos) continue;
        if (stamp[e] != r) {
          stamp[e] = r;
          cnt[e] = 1;
        } else if (++cnt[e] > out[e].dup_max) {
          out[e].dup_max = cnt[e];
          out[e].flags |= LC_SF_DUPLICATED;
        }
      }
    }
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  return 0;
}

}  // namespace lcsf

extern "C" int lc_set_full_host(const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads,
                                int64_t n_reads, const int64_t *read_values, int64_t n_values,
                                int32_t linearizable, lc_sf_element *out, lc_sf_summary *sum) {
  using namespace lcsf;
  const auto t0 = std::chrono::steady_clock::now();
  if (int rc = check_contract(adds, n_adds, reads, n_reads, read_values, n_values, nullptr)) return rc;
  if (n_adds > 0 && !out) return -EINVAL;
  try {
    const size_t n = (size_t)n_adds;
    Table tab(n_adds);
    for (int64_t e = 0; e < n_adds; e++)
      if (!tab.insert(adds[e].value, (int32_t)e)) return -EINVAL;  // two adds of one value
    // per element: the first observing read, and the reads whose invokes are
    // last_present / last_absent (-1: none)
    std::vector<int64_t> first(n, -1), present(n, -1), absent(n, -1), stamp(n, -1);
    std::vector<int32_t> cnt(n, 0), dup(n, 0);
    int64_t n_phantom = 0, nc = 0;  // nc: the elements the current read concerns (a prefix)
    for (int64_t r = 0; r < n_reads; r++) {
      const lc_sf_read &q = reads[r];
      while (nc < n_adds && adds[nc].inv_pos < q.ok_pos) nc++;
      for (int64_t i = q.off; i < q.off + q.len; i++) {
        const int32_t e = tab.find(read_values[i]);
        if (e < 0 || e >= nc) {
          n_phantom++;
        } else if (stamp[e] != r) {
          stamp[e] = r;
          cnt[e] = 1;
        } else if (++cnt[e] > dup[e]) {
          dup[e] = cnt[e];
        }
      }
      for (int64_t e = 0; e < nc; e++) {
        if (stamp[e] == r) {
          if (first[e] < 0) first[e] = r;
          if (present[e] < 0 || q.inv_pos >= reads[present[e]].inv_pos) present[e] = r;
        } else if (absent[e] < 0 || q.inv_pos >= reads[absent[e]].inv_pos) {
          absent[e] = r;
        }
      }
    }
    for (int64_t e = 0; e < n_adds; e++) {
      const lc_sf_read *f = first[e] < 0 ? nullptr : &reads[first[e]];
      const lc_sf_read *p = present[e] < 0 ? nullptr : &reads[present[e]];
      const lc_sf_read *a = absent[e] < 0 ? nullptr : &reads[absent[e]];
      lc_sf_element o = decide(adds[e], f ? f->ok_pos : -1, f ? f->ok_time : 0, p ? p->inv_pos : -1,
                               p ? p->inv_time : 0, a ? a->inv_pos : -1, a ? a->inv_time : 0);
      if (dup[e]) {
        o.dup_max = dup[e];
        o.flags |= LC_SF_DUPLICATED;
      }
      out[e] = o;
    }
    if (sum) {
      summarize(out, n_adds, linearizable, sum);
      sum->n_phantom = n_phantom;
      sum->n_tiles = 0;
      sum->h2d_ms = sum->kernel_ms = 0;
      sum->total_ms =
          std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  return 0;
}

extern "C" int lc_set_full_limits(lc_sf_limit_info *out) {
  if (!out) return -EINVAL;
  out->default_tile_bytes = lcsf::kDefaultTileBytes;
  out->tile_bytes = lcsf::kDefaultTileBytes;
  if (const char *e = getenv("LC_SF_TILE_BYTES")) {
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end != e && v > 0) out->tile_bytes = v;
  }
  out->max_position = lcsf::kMaxPosition;
  out->value_bytes = sizeof(int64_t);
  return 0;
}
