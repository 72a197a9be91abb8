// perfstats_host.cpp — lc_perf_stats_host: the rules of
// include/lincheck_perf.h on the host, single-threaded: the fallback for calls
// the device has nothing to do for, the device path's oracle and the probe's
// baseline.  lc_perf_stats_limits.  Nothing of HIP: tests/perfstats_main.cpp
// compiles this file with g++ and the sanitizers.
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <unordered_map>
#include <utility>
#include <vector>

#include "perfstats.h"

namespace {

int perf_stats_host(const lc_ps_event *ev, int64_t n, const lc_ps_params *p, const lc_ps_out *out,
                    lc_ps_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  const char *why = nullptr;
  if (int rc = lcps::check_params(ev, n, p, out, &why)) return rc;
  int64_t t_max = 0, n_client = 0;
  for (int64_t i = 0; i < n; i++) {
    if (lcps::bad_event(ev[i], p->n_f)) return -EINVAL;
    if (ev[i].process < 0) continue;
    n_client++;
    t_max = std::max(t_max, ev[i].time);
  }
  int64_t n_rate = 0, n_quant = 0;
  if (int rc = lcps::check_tables(t_max, p, out, &n_rate, &n_quant, &why)) {
    if (rc == -ENOSPC) lcps::summary_for_room(sum, n, n_client, t_max, n_rate, n_quant);
    return rc;
  }
  const int64_t nf = p->n_f, nq = p->n_q;
  std::vector<int64_t> rate((size_t)(nf * 3 * n_rate), 0), quant_n((size_t)(nf * n_quant), 0),
      quant((size_t)(nf * n_quant * nq), LC_PS_NONE);
  lc_ps_summary sm{};
  sm.n_events = n;
  sm.n_client = n_client;
  sm.t_max = t_max;
  sm.n_rate_buckets = n_rate;
  sm.n_quant_buckets = n_quant;
  if (out->comp_pos)
    for (int64_t i = 0; i < n; i++) {
      out->comp_pos[i] = -1;
      out->latency_ns[i] = LC_PS_NONE;
    }
  // rule 3: the process's last event, where it is an invoke that nothing followed yet
  std::unordered_map<int32_t, int32_t> open;
  std::vector<std::pair<int64_t, int64_t>> lat;  // (group, latency)
  for (int64_t i = 0; i < n; i++) {
    const lc_ps_event &e = ev[i];
    if (e.process < 0) continue;
    auto it = open.find(e.process);
    if (e.type == LC_EV_INVOKE) {
      if (it == open.end())
        open.emplace(e.process, (int32_t)i);
      else {
        if (it->second >= 0) sm.n_pending++;
        it->second = (int32_t)i;
      }
      continue;
    }
    rate[(size_t)((e.f * 3 + (e.type - 1)) * n_rate + e.time / p->rate_dt_ns)]++;
    if (it == open.end() || it->second < 0) {
      sm.n_ignored_completions++;
      continue;
    }
    const lc_ps_event &inv = ev[it->second];
    const int64_t l = e.time - inv.time;
    if (out->comp_pos) {
      out->comp_pos[it->second] = (int32_t)i;
      out->latency_ns[it->second] = l;
    }
    sm.n_pairs++;
    if (e.f != inv.f) sm.n_mismatched_f++;
    lat.emplace_back(inv.f * n_quant + inv.time / p->quant_dt_ns, l);
    it->second = -1;
  }
  for (const auto &kv : open)
    if (kv.second >= 0) sm.n_pending++;
  // rule 6
  std::sort(lat.begin(), lat.end());
  for (size_t a = 0; a < lat.size();) {
    size_t b = a;
    while (b < lat.size() && lat[b].first == lat[a].first) b++;
    const int64_t g = lat[a].first, cnt = (int64_t)(b - a);
    quant_n[(size_t)g] = cnt;
    for (int64_t k = 0; k < nq; k++)
      quant[(size_t)(g * nq + k)] = lat[a + (size_t)lcps::quantile_index(p->q[k], cnt)].second;
    a = b;
  }
  lcps::place_tables(p, rate.data(), quant_n.data(), quant.data(), n_rate, n_quant, out, &sm);
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  return 0;
}

}  // namespace

extern "C" int lc_perf_stats_host(const lc_ps_event *ev, int64_t n_events, const lc_ps_params *params,
                                  const lc_ps_out *out, lc_ps_summary *sum) {
  try {
    return perf_stats_host(ev, n_events, params, out, sum);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int lc_perf_stats_limits(lc_ps_limit_info *out) {
  if (!out) return -EINVAL;
  lc_ps_limit_info l{};
  l.max_f = lcps::kMaxF;
  l.max_table_entries = lcps::kMaxTableEntries;
  l.lds_entries = l.default_lds_entries = lcps::kDefaultLdsEntries;
  if (const char *s = getenv("LC_PS_LDS_ENTRIES")) {
    char *end = nullptr;
    const long long v = strtoll(s, &end, 10);
    if (end != s && *end == 0 && v >= 0 && v <= lcps::kDefaultLdsEntries) l.lds_entries = v;
  }
  l.wave = lcps::kWave;
  l.block = lcps::kBlock;
  l.chunk = lcps::kChunk;
  l.max_grid = lcps::kMaxGrid;
  *out = l;
  return 0;
}
