// screen_host.cpp — lc_cycle_screen_host (include/lincheck_screen.h): the
// definition on one thread, the Jacobi iteration written plainly; and what
// the device call shares with it (the contract, the limits).  g++, no GPU.
#include <errno.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <utility>
#include <vector>

#include "screen.h"

namespace lcscreen {

int validate(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
             const lc_screen_out *out, int64_t *n_ok, const char **err) {
  *n_ok = 0;
  if (n_txns < 0 || n_edges < 0 || n_txns > INT32_MAX || (n_txns && !txns) || (n_edges && !edges)) {
    *err = "bad counts or null inputs";
    return -EINVAL;
  }
  if (!out || !out->reach_lo || !out->reach_hi || !out->mark) {
    *err = "out or one of its arrays is null";
    return -EINVAL;
  }
  int64_t prev = -1;
  for (int64_t t = 0; t < n_txns; t++) {
    const lc_ap_txn &x = txns[t];
    if (x.inv_pos <= prev || x.inv_pos >= kMaxPosition) {
      *err = "txns not strictly ascending by inv_pos";
      return -EINVAL;
    }
    prev = x.inv_pos;
    if (x.type == LC_AP_INFO) {
      if (x.comp_pos != -1) {
        *err = "an INFO txn with a comp_pos";
        return -EINVAL;
      }
    } else if (x.type == LC_AP_OK || x.type == LC_AP_FAIL) {
      if (x.comp_pos <= x.inv_pos || x.comp_pos >= kMaxPosition) {
        *err = "comp_pos not above inv_pos";
        return -EINVAL;
      }
    } else {
      *err = "unknown txn type";
      return -EINVAL;
    }
    *n_ok += x.type == LC_AP_OK;
  }
  for (int64_t e = 0; e < n_edges; e++) {
    const lc_ap_edge &x = edges[e];
    if (x.from < 0 || x.from >= n_txns || x.to < 0 || x.to >= n_txns) {
      *err = "an edge end out of range";
      return -EINVAL;
    }
    if (txns[x.from].type == LC_AP_FAIL || txns[x.to].type == LC_AP_FAIL) {
      *err = "an edge end that is a FAIL txn";
      return -EINVAL;
    }
    if (x.from == x.to) {
      *err = "an edge from a txn to itself";
      return -EINVAL;
    }
    if (e && !edge_less(edges[e - 1], x)) {
      *err = "edges not strictly ascending by (from, to, type, key)";
      return -EINVAL;
    }
  }
  return 0;
}

int32_t max_rounds() {
  if (const char *e = getenv("LC_SCREEN_MAX_ROUNDS")) {
    const long long v = atoll(e);
    if (v > 0) return (int32_t)std::min<long long>(v, INT32_MAX);
  }
  return kDefaultMaxRounds;
}

namespace {

int screen_host(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
                const lc_screen_out *out, lc_screen_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  int64_t n_ok = 0;
  const char *why = nullptr;
  if (int e = validate(txns, n_txns, edges, n_edges, out, &n_ok, &why)) return e;
  lc_screen_summary sm{};
  sm.max_rounds = max_rounds();
  sm.clean = 1;
  const size_t n = (size_t)n_txns;
  if (n) {
    // byc, rt_hi(v) and first(u)
    std::vector<std::pair<int32_t, int32_t>> done;  // (comp_pos, txn) of the OK txns
    for (size_t t = 0; t < n; t++)
      if (txns[t].type == LC_AP_OK) done.push_back({txns[t].comp_pos, (int32_t)t});
    std::sort(done.begin(), done.end());
    std::vector<int32_t> rt_hi(n, 0), first(n, (int32_t)n);
    for (size_t t = 0; t < n; t++) {
      if (txns[t].type != LC_AP_FAIL)
        rt_hi[t] = (int32_t)(std::lower_bound(done.begin(), done.end(), std::make_pair(txns[t].inv_pos, (int32_t)-1)) -
                             done.begin());
      if (txns[t].type == LC_AP_OK) {
        size_t lo = 0, hi = n;
        while (lo < hi) {
          const size_t mid = (lo + hi) / 2;
          if (txns[mid].inv_pos > txns[t].comp_pos) hi = mid;
          else lo = mid + 1;
        }
        first[t] = (int32_t)lo;
      }
    }
    std::vector<int32_t> h(n), k(n), hn(n), kn(n), s(n + 1), p(done.size() + 1);
    for (size_t t = 0; t < n; t++) {
      h[t] = txns[t].type == LC_AP_OK ? txns[t].comp_pos : kNoComp;
      k[t] = txns[t].type == LC_AP_FAIL ? kNoInv : txns[t].inv_pos;
    }
    bool converged = false;
    for (int32_t r = 1; r <= sm.max_rounds && !converged; r++) {
      s[n] = kNoComp;
      for (size_t t = n; t-- > 0;) s[t] = std::min(s[t + 1], h[t]);
      p[0] = kNoInv;
      for (size_t i = 0; i < done.size(); i++) p[i + 1] = std::max(p[i], k[done[i].second]);
      for (size_t t = 0; t < n; t++) {
        hn[t] = txns[t].type == LC_AP_OK ? std::min(h[t], s[first[t]]) : h[t];
        kn[t] = std::max(k[t], p[rt_hi[t]]);
      }
      for (int64_t e = 0; e < n_edges; e++) {
        const int32_t u = edges[e].from, v = edges[e].to;
        hn[u] = std::min(hn[u], h[v]);
        kn[v] = std::max(kn[v], k[u]);
      }
      converged = hn == h && kn == k;
      h.swap(hn);
      k.swap(kn);
      sm.label_rounds = r;
    }
    std::vector<uint8_t> alive(n, 0), an(n), has_in(n), has_out(n);
    for (size_t t = 0; t < n; t++) {
      const bool node = txns[t].type != LC_AP_FAIL, rt = node && h[t] < k[t];
      out->reach_lo[t] = h[t];
      out->reach_hi[t] = k[t];
      out->mark[t] = rt ? LC_SCREEN_RT : 0;
      sm.n_rt_members += rt;
      alive[t] = node && !rt;
    }
    if (!converged) {
      sm.clean = -1;
    } else {
      bool quiet = false;
      for (int32_t r = 1; r <= sm.max_rounds && !quiet; r++) {
        std::fill(has_in.begin(), has_in.end(), 0);
        std::fill(has_out.begin(), has_out.end(), 0);
        for (int64_t e = 0; e < n_edges; e++) {
          const int32_t u = edges[e].from, v = edges[e].to;
          if (alive[u] && alive[v] && h[u] == h[v] && k[u] == k[v]) has_out[u] = has_in[v] = 1;
        }
        for (size_t t = 0; t < n; t++) an[t] = alive[t] & has_in[t] & has_out[t];
        quiet = an == alive;
        alive.swap(an);
        sm.trim_rounds = r;
      }
      for (size_t t = 0; t < n; t++)
        if (alive[t]) {
          out->mark[t] |= LC_SCREEN_TRIM;
          sm.n_trim_survivors++;
        }
      sm.clean = !quiet ? -1 : (sm.n_rt_members == 0 && sm.n_trim_survivors == 0);
    }
  }
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  return 0;
}

}  // namespace

}  // namespace lcscreen

extern "C" int lc_screen_limits(lc_screen_limit_info *out) {
  if (!out) return -EINVAL;
  out->default_max_rounds = lcscreen::kDefaultMaxRounds;
  out->max_rounds = lcscreen::max_rounds();
  return 0;
}

extern "C" int lc_cycle_screen_host(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
                                    const lc_screen_out *out, lc_screen_summary *sum) {
  try {
    return lcscreen::screen_host(txns, n_txns, edges, n_edges, out, sum);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}
