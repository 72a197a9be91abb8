// watch_host.cpp — lc_watch_check_host: the rules of include/lincheck_watch.h
// on the host, single-threaded; and the host steps of lc_watch_check (the
// contract, the class rounds, the canonical log, the deltas' order and the
// summary), which watch_dev.cpp runs between its kernels.  g++, no GPU.
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <unordered_set>

#include "watch.h"

namespace lcwt {

Limits limits() {
  Limits l{kDefaultMaxD, kDefaultTraceBytes, ~uint64_t(0), ~uint64_t(0)};
  if (const char *e = getenv("LC_WT_MAX_D")) {
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end != e && v >= 0) l.max_d = std::min<long long>(v, LC_WT_MAX_D_LIMIT);
  }
  if (const char *e = getenv("LC_WT_TRACE_BYTES")) {
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end != e && v > 0) l.trace_bytes = v;
  }
  if (const char *e = getenv("LC_WT_HASH_MASK")) {
    char *end = nullptr;
    const unsigned long long v = strtoull(e, &end, 0);
    if (end != e) l.mask = v, l.mask_hi = 0;  // (a 64-bit number onto a 128-bit hash)
  }
  return l;
}

int validate(const lc_wt_thread *threads, int64_t n_threads, const int64_t *values, int64_t n_values,
             int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out, const char **err) {
#define LCWT_BAD(text) \
  do {                 \
    *err = text;       \
    return -EINVAL;    \
  } while (0)
  if (n_threads < 0 || n_values < 0 || (n_threads > 0 && !threads) || (n_values > 0 && !values))
    LCWT_BAD("null array or negative count");
  if (n_threads >= kMaxLen) LCWT_BAD("2^31 - 1 or more threads");
  if (n_nonmonotonic < 0) LCWT_BAD("negative n_nonmonotonic");
  if (flags) LCWT_BAD("unknown flag");
  if (!out || !out->cls || !out->distance || !out->deltas || !out->edits) LCWT_BAD("null out");
  if (out->edit_cap < 0) LCWT_BAD("negative edit_cap");
  std::unordered_set<int64_t> ids;
  ids.reserve((size_t)n_threads * 2);
  for (int64_t t = 0; t < n_threads; t++) {
    const lc_wt_thread &x = threads[t];
    if (x.off < 0 || x.len < 0) LCWT_BAD("a negative off or len");
    if (x.len >= kMaxLen) LCWT_BAD("a log of 2^31 - 1 entries or more");
    if (x.off > n_values || x.len > n_values - x.off) LCWT_BAD("a log runs past n_values");
    if (!ids.insert(x.thread).second) LCWT_BAD("a thread id repeated");
  }
  return 0;
#undef LCWT_BAD
}

// The log hash of watch.h by Horner's rule.
static Hash hash_log(const int64_t *v, int64_t n) {
  uint64_t h1 = 0, h2 = 0;
  for (int64_t i = 0; i < n; i++) {
    h1 = h1 * kBase1 + mix1(v[i]);
    h2 = h2 * kBase2 + mix2(v[i]);
  }
  return Hash{h1, h2};
}

void ClassRounds::init(const lc_wt_thread *threads, int64_t n_threads, const Hash *hashes, uint64_t mask,
                       uint64_t mask_hi) {
  cls.assign((size_t)n_threads, -1);
  n_collisions = 0;
  pending_.clear();
  rep_.clear();
  std::vector<int32_t> idx((size_t)n_threads);
  for (int64_t t = 0; t < n_threads; t++) idx[(size_t)t] = (int32_t)t;
  auto key_less = [&](int32_t a, int32_t b) {
    if (threads[a].len != threads[b].len) return threads[a].len < threads[b].len;
    const uint64_t a1 = hashes[a].h1 & mask, b1 = hashes[b].h1 & mask;
    if (a1 != b1) return a1 < b1;
    const uint64_t a2 = hashes[a].h2 & mask_hi, b2 = hashes[b].h2 & mask_hi;
    if (a2 != b2) return a2 < b2;
    return a < b;
  };
  auto same_key = [&](int32_t a, int32_t b) {
    return threads[a].len == threads[b].len && (hashes[a].h1 & mask) == (hashes[b].h1 & mask) &&
           (hashes[a].h2 & mask_hi) == (hashes[b].h2 & mask_hi);
  };
  std::sort(idx.begin(), idx.end(), key_less);
  for (size_t i = 0; i < idx.size();) {
    size_t j = i + 1;  // (within a group the order is by position: the first is its representative)
    while (j < idx.size() && same_key(idx[i], idx[j])) j++;
    cls[(size_t)idx[i]] = idx[i];
    rep_.push_back(idx[i]);
    pending_.emplace_back(idx.begin() + (long)i + 1, idx.begin() + (long)j);
    i = j;
  }
  make_pairs();
}

void ClassRounds::make_pairs() {
  pairs_.clear();
  for (size_t g = 0; g < pending_.size(); g++)
    for (int32_t t : pending_[g]) pairs_.emplace_back(t, rep_[g]);
}

void ClassRounds::feed(const std::vector<uint8_t> &equal) {
  size_t i = 0;
  for (size_t g = 0; g < pending_.size(); g++) {
    std::vector<int32_t> left;
    for (int32_t t : pending_[g]) {
      if (equal[i++]) {
        cls[(size_t)t] = rep_[g];
      } else {
        n_collisions++;
        left.push_back(t);
      }
    }
    if (!left.empty()) {  // the lowest of them stands for a class of its own
      rep_[g] = left.front();
      cls[(size_t)left.front()] = left.front();
      left.erase(left.begin());
    }
    pending_[g].swap(left);
  }
  make_pairs();
}

int32_t pick_canonical(const lc_wt_thread *threads, int64_t n_threads, const std::vector<int32_t> &cls,
                       int64_t *size, int64_t *n_classes) {
  std::vector<int64_t> count((size_t)n_threads, 0);
  for (int64_t t = 0; t < n_threads; t++) count[(size_t)cls[(size_t)t]]++;
  int32_t best = -1;
  int64_t classes = 0, largest = 0;
  for (int64_t t = 0; t < n_threads; t++)
    if (count[(size_t)t]) {
      classes++;
      largest = std::max(largest, count[(size_t)t]);
    }
  for (int64_t t = 0; t < n_threads; t++) {
    if (!count[(size_t)t]) continue;
    // a mode exists: the largest class; otherwise the longest log; the first of equals
    const bool better = best < 0 || (largest > 1 ? count[(size_t)t] > count[(size_t)best]
                                                 : threads[t].len > threads[best].len);
    if (better) best = (int32_t)t;
  }
  *size = best < 0 ? 0 : count[(size_t)best];
  *n_classes = classes;
  return best;
}

// Rule 4's p and s.
static void trim_host(const int64_t *A, int64_t la, const int64_t *B, int64_t lb, int64_t *p, int64_t *s) {
  const int64_t lim = std::min(la, lb);
  int64_t i = 0;
  while (i < lim && A[i] == B[i]) i++;
  int64_t j = 0;
  while (j < lim - i && A[la - 1 - j] == B[lb - 1 - j]) j++;
  *p = i;
  *s = j;
}

namespace {

// V over the diagonals -d .. d in O(d) memory: the non-negative ones and the negative ones.
struct Diagonals {
  std::vector<int64_t> pos, neg;
  int64_t &at(int64_t k) {
    std::vector<int64_t> &v = k >= 0 ? pos : neg;
    const size_t i = (size_t)(k >= 0 ? k : -k);
    if (v.size() <= i) v.resize(i + 1, 0);
    return v[i];
  }
};

}  // namespace

int64_t myers_host(const int64_t *a, int64_t n, const int64_t *b, int64_t m, int64_t max_d, int64_t base,
                   std::vector<lc_wt_edit> *script, bool *scripted) {
  Diagonals V;
  V.at(1) = 0;
  // x <= n + d < 2^32: a trace entry is a uint32.  Kept only while d <= max_d.
  std::vector<uint32_t> trace;
  bool tracing = max_d >= 0;
  int64_t D = -1;
  for (int64_t d = 0; d <= n + m; d++) {
    if (tracing && d > max_d) {
      tracing = false;
      std::vector<uint32_t>().swap(trace);
    }
    V.at(d + 1);  // (both neighbours of every diagonal of this round exist)
    V.at(-d - 1);
    for (int64_t k = -d; k <= d; k += 2) {
      int64_t x = comes_down(k, d, V.at(k - 1), V.at(k + 1)) ? V.at(k + 1) : V.at(k - 1) + 1;
      int64_t y = x - k;
      while (x < n && y < m && a[x] == b[y]) x++, y++;
      V.at(k) = x;
      if (tracing) trace.push_back((uint32_t)x);
    }
    if (d >= std::abs(n - m) && ((d ^ (n - m)) & 1) == 0 && V.at(n - m) >= n) {
      D = d;
      break;
    }
  }
  if (scripted) *scripted = false;
  if (!tracing || !script) return D;
  script->assign((size_t)D, lc_wt_edit{});
  int64_t k = n - m;
  for (int64_t d = D; d >= 1; d--) {
    const uint32_t *row = trace.data() + trace_row(d - 1);
    // row d - 1 holds k' = -(d-1) + 2 i; the neighbour the rule does not read may lie outside it
    auto get = [&](int64_t kk) -> int64_t {
      const int64_t i = kk + (d - 1);
      return (i < 0 || i > 2 * (d - 1)) ? 0 : (int64_t)row[i / 2];
    };
    lc_wt_edit &e = (*script)[(size_t)(d - 1)];
    if (comes_down(k, d, get(k - 1), get(k + 1))) {
      const int64_t x = get(k + 1), y = x - (k + 1);
      e = lc_wt_edit{base + x, b[y], LC_WT_INSERT, 0};
      k = k + 1;
    } else {
      const int64_t x = get(k - 1);
      e = lc_wt_edit{base + x, a[x], LC_WT_DELETE, 0};
      k = k - 1;
    }
  }
  *scripted = true;
  return D;
}

int place_and_summarize(const lc_wt_thread *threads, int64_t n_threads, int64_t n_nonmonotonic,
                        const std::vector<int32_t> &cls, int32_t canonical, int64_t canonical_size, int64_t n_classes,
                        int64_t n_collisions, std::vector<Diff> *diffs, const lc_wt_out *out, lc_wt_summary *sum) {
  std::sort(diffs->begin(), diffs->end(), [](const Diff &a, const Diff &b) {
    return a.dist != b.dist ? a.dist > b.dist : a.thread < b.thread;
  });
  int64_t n_edits = 0, n_no_script = 0;
  for (const Diff &d : *diffs) {
    if (d.no_script) n_no_script++;
    else n_edits += d.dist;
  }
  if (n_edits > out->edit_cap) {
    if (sum) {
      *sum = lc_wt_summary{};
      sum->n_edits = n_edits;
    }
    return -ENOSPC;
  }
  for (int64_t t = 0; t < n_threads; t++) {
    out->cls[t] = cls[(size_t)t];
    out->distance[t] = 0;
  }
  int64_t off = 0;
  for (size_t i = 0; i < diffs->size(); i++) {
    const Diff &d = (*diffs)[i];
    out->distance[d.thread] = d.dist;
    const int64_t len = d.no_script ? 0 : d.dist;
    out->deltas[i] = lc_wt_delta{d.thread, d.no_script ? LC_WT_NO_SCRIPT : 0u, d.dist, d.p, d.s, off, len};
    off += len;
  }
  if (!sum) return 0;
  lc_wt_summary sm{};
  sm.canonical = canonical;
  sm.canonical_size = canonical_size;
  sm.n_threads = n_threads;
  sm.n_classes = n_classes;
  sm.n_deltas = (int64_t)diffs->size();
  sm.n_edits = n_edits;
  sm.n_no_script = n_no_script;
  sm.n_collisions = n_collisions;
  sm.revisions_equal = 1;
  for (int64_t t = 1; t < n_threads; t++)
    if (threads[t].revision != threads[0].revision) sm.revisions_equal = 0;
  // rule 9
  if (n_nonmonotonic > 0) sm.valid = 0;
  else if (n_threads == 0 || !sm.revisions_equal) sm.valid = -1;
  else sm.valid = diffs->empty() ? 1 : 0;
  *sum = sm;
  return 0;
}

namespace {

int check_host(const lc_wt_thread *threads, int64_t n_threads, const int64_t *values, int64_t n_values,
               int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out, lc_wt_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  const char *why = nullptr;
  if (int e = validate(threads, n_threads, values, n_values, n_nonmonotonic, flags, out, &why)) return e;
  const Limits lim = limits();
  std::vector<Hash> hashes((size_t)n_threads);
  for (int64_t t = 0; t < n_threads; t++) hashes[(size_t)t] = hash_log(values + threads[t].off, threads[t].len);
  ClassRounds cr;
  cr.init(threads, n_threads, hashes.data(), lim.mask, lim.mask_hi);
  while (!cr.pairs().empty()) {
    std::vector<uint8_t> equal;
    for (const auto &pr : cr.pairs())  // (one length: the hash's group)
      equal.push_back(threads[pr.first].len == 0 ||
                      memcmp(values + threads[pr.first].off, values + threads[pr.second].off,
                             sizeof(int64_t) * (size_t)threads[pr.first].len) == 0);
    cr.feed(equal);
  }
  int64_t size = 0, n_classes = 0;
  const int32_t canon = pick_canonical(threads, n_threads, cr.cls, &size, &n_classes);
  std::vector<Diff> diffs;
  std::vector<std::vector<lc_wt_edit>> scripts((size_t)n_threads);
  for (int64_t t = 0; t < n_threads; t++) {
    if (cr.cls[(size_t)t] == canon) continue;
    const int64_t *A = values + threads[canon].off, *B = values + threads[t].off;
    const int64_t la = threads[canon].len, lb = threads[t].len;
    Diff d{(int32_t)t, false, 0, 0, 0};
    trim_host(A, la, B, lb, &d.p, &d.s);
    bool scripted = false;
    d.dist = myers_host(A + d.p, la - d.p - d.s, B + d.p, lb - d.p - d.s, lim.max_d, d.p, &scripts[(size_t)t],
                        &scripted);
    d.no_script = !scripted;
    diffs.push_back(d);
  }
  lc_wt_summary sm;
  if (int e = place_and_summarize(threads, n_threads, n_nonmonotonic, cr.cls, canon, size, n_classes,
                                  cr.n_collisions, &diffs, out, sum ? &sm : nullptr)) {
    if (sum) *sum = sm;
    return e;
  }
  for (size_t i = 0; i < diffs.size(); i++) {
    const std::vector<lc_wt_edit> &s = scripts[(size_t)diffs[i].thread];
    if (!diffs[i].no_script && !s.empty())
      memcpy(out->edits + out->deltas[i].script_off, s.data(), sizeof(lc_wt_edit) * s.size());
  }
  if (sum) {
    sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    *sum = sm;
  }
  return 0;
}

}  // namespace

}  // namespace lcwt

extern "C" int lc_watch_check_host(const lc_wt_thread *threads, int64_t n_threads, const int64_t *values,
                                   int64_t n_values, int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out,
                                   lc_wt_summary *sum) {
  try {
    return lcwt::check_host(threads, n_threads, values, n_values, n_nonmonotonic, flags, out, sum);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int lc_watch_limits(lc_wt_limit_info *out) {
  if (!out) return -EINVAL;
  const lcwt::Limits l = lcwt::limits();
  out->max_d = l.max_d;
  out->default_max_d = lcwt::kDefaultMaxD;
  out->trace_bytes = l.trace_bytes;
  out->default_trace_bytes = lcwt::kDefaultTraceBytes;
  out->max_len = lcwt::kMaxLen;
  out->max_device_len = lcwt::kMaxDeviceLen;
  out->hash_mask = l.mask;
  return 0;
}
