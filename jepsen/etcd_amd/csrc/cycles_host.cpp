// cycles_host.cpp — lc_cycle_reach_host (include/lincheck_cycles.h): the
// definition on one thread; what the device call shares with it (the
// contract, the limits); and lc_cycles_host, rule 7 alone for tests and
// tools.  g++, no GPU.
#include <errno.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <vector>

#include "cycles.h"

namespace lccyc {

namespace {

int check_offsets(const int64_t *off, int64_t n, int64_t total) {
  if (off[0] != 0 || off[n] != total) return -EINVAL;
  for (int64_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return -EINVAL;
  return 0;
}

}  // namespace

int validate(int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred, int64_t n_queries,
             const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads, int64_t n_heads, uint32_t flags,
             const int32_t *hit, const char **err) {
#define LCCYC_BAD(text) \
  do {                  \
    *err = text;        \
    return -EINVAL;     \
  } while (0)
  if (n_nodes < 0 || n_nodes >= INT32_MAX || n_queries < 0 || n_queries >= INT32_MAX || n_pred < 0 || n_heads < 0)
    LCCYC_BAD("a count out of range");
  if (!pred_off || !q_head_off || (n_pred && !pred) || (n_queries && !q_node) || (n_heads && !q_heads))
    LCCYC_BAD("a null input");
  if (flags & ~LC_REACH_ALL) LCCYC_BAD("unknown flags");
  if ((flags & LC_REACH_ALL) && n_queries && !hit) LCCYC_BAD("LC_REACH_ALL without hit");
  if (check_offsets(pred_off, n_nodes, n_pred)) LCCYC_BAD("pred_off does not start at 0, ascend and end at n_pred");
  if (check_offsets(q_head_off, n_queries, n_heads))
    LCCYC_BAD("q_head_off does not start at 0, ascend and end at n_heads");
  for (int64_t i = 0; i < n_pred; i++)
    if (pred[i] < 0 || pred[i] >= n_nodes) LCCYC_BAD("a predecessor that is no node");
  for (int64_t q = 0; q < n_queries; q++) {
    if (q_node[q] < 0 || q_node[q] >= n_nodes) LCCYC_BAD("a source that is no node");
    if (q && q_node[q] <= q_node[q - 1]) LCCYC_BAD("q_node not strictly ascending");
    for (int64_t i = q_head_off[q]; i < q_head_off[q + 1]; i++) {
      if (q_heads[i] < 0 || q_heads[i] >= n_nodes) LCCYC_BAD("a head that is no node");
      if (q_heads[i] == q_node[q]) LCCYC_BAD("a head that is its query's source");
    }
  }
  return 0;
#undef LCCYC_BAD
}

int64_t min_work() {
  if (const char *e = getenv("LC_CYCLE_MIN_WORK")) {
    char *end = nullptr;
    const long long v = strtoll(e, &end, 10);
    if (end != e && v >= 0) return v;
  }
  return kDefaultMinWork;
}

int workgroups(int64_t n_nodes, int64_t n_queries) {
  const int64_t room = kQueueBytes / (int64_t)sizeof(int32_t) / std::max<int64_t>(n_nodes, 1);
  return (int)std::max<int64_t>(1, std::min<int64_t>({n_queries, kMaxWorkgroups, room}));
}

namespace {

int reach_host(int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred, int64_t n_queries,
               const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads, int64_t n_heads,
               uint32_t flags, int32_t *hit, lc_reach_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  const char *why = nullptr;
  if (int e = validate(n_nodes, pred_off, pred, n_pred, n_queries, q_node, q_head_off, q_heads, n_heads, flags, hit,
                       &why))
    return e;
  const bool all = flags & LC_REACH_ALL;
  lc_reach_summary sm{};
  sm.first_hit = -1;
  // stamps instead of bitmaps: seen[x] == q + 1 once query q has marked x, is_head[x] == q + 1 for its heads
  std::vector<int32_t> seen((size_t)n_nodes, 0), is_head((size_t)n_nodes, 0), queue;
  queue.reserve((size_t)n_nodes);
  for (int64_t q = 0; q < n_queries; q++) {
    const int32_t stamp = (int32_t)q + 1;
    for (int64_t i = q_head_off[q]; i < q_head_off[q + 1]; i++) is_head[(size_t)q_heads[i]] = stamp;
    bool found = false;
    queue.assign(1, q_node[q]);
    seen[(size_t)q_node[q]] = stamp;
    for (size_t at = 0; at < queue.size() && (all || !found); at++) {
      const int32_t b = queue[at];
      for (int64_t i = pred_off[b]; i < pred_off[b + 1] && (all || !found); i++) {
        const int32_t a = pred[i];
        if (seen[(size_t)a] == stamp) continue;
        seen[(size_t)a] = stamp;
        if (is_head[(size_t)a] == stamp) found = true;
        queue.push_back(a);
      }
    }
    sm.n_queries_run++;
    sm.nodes_visited += (int64_t)queue.size();
    if (all) hit[q] = found;
    if (found && sm.first_hit < 0) sm.first_hit = q;
    if (found && !all) break;
  }
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  return 0;
}

}  // namespace

}  // namespace lccyc

extern "C" int lc_cycle_reach_host(int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred,
                                   int64_t n_queries, const int32_t *q_node, const int64_t *q_head_off,
                                   const int32_t *q_heads, int64_t n_heads, uint32_t flags, int32_t *hit,
                                   lc_reach_summary *sum) {
  try {
    return lccyc::reach_host(n_nodes, pred_off, pred, n_pred, n_queries, q_node, q_head_off, q_heads, n_heads, flags,
                             hit, sum);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}

extern "C" int lc_cycle_reach_limits(lc_reach_limit_info *out) {
  if (!out) return -EINVAL;
  out->max_nodes = lccyc::kMaxNodes;
  out->min_work = lccyc::min_work();
  out->default_min_work = lccyc::kDefaultMinWork;
  out->max_workgroups = lccyc::kMaxWorkgroups;
  out->pad = 0;
  return 0;
}

extern "C" int lc_cycles_host(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
                              const int32_t *mark, lc_reach_fn reach, void *user, int64_t min_work, int64_t max_nodes,
                              int32_t *scc, int32_t *scc_class, lc_ap_step *steps, int64_t *cycle_off,
                              int32_t *cycle_scc, int64_t *n_class, int64_t *n_scc, lc_cycle_search_summary *srch) {
  try {
    std::vector<int32_t> byc((size_t)n_txns), lo((size_t)n_txns), hi((size_t)n_txns);
    lcgraph::real_time_host(txns, n_txns, byc.data(), lo.data(), hi.data());
    int64_t n_ok = 0, n_nodes = 0;
    for (int64_t t = 0; t < n_txns; t++) {
      n_ok += txns[t].type == LC_AP_OK;
      n_nodes += txns[t].type != LC_AP_FAIL;
    }
    lcgraph::CycleCounts cc{};
    lc_cycle_search_summary sr{};
    if (!mark) {
      lcgraph::cycles_host(txns, n_txns, n_nodes, edges, n_edges, byc.data(), lo.data(), hi.data(), scc, scc_class,
                           steps, cycle_off, cycle_scc, &cc);
    } else {
      lcgraph::MarkedPass mp;
      mp.mark = mark;
      mp.min_work = min_work;
      if (max_nodes > 0) mp.max_nodes = max_nodes;
      if (reach)
        mp.hook = [&](const lcgraph::ReachProblem &p, int64_t *first_hit) {
          return reach(user, p.n_nodes, p.pred_off, p.pred, p.n_queries, p.q_node, p.q_head_off, p.q_heads,
                       first_hit)
                     ? -E2BIG  // (the host loop)
                     : 0;
        };
      if (int e = lcgraph::cycles_host_marked(txns, n_txns, edges, n_edges, byc.data(), n_ok, lo.data(), hi.data(),
                                              &mp, scc, scc_class, steps, cycle_off, cycle_scc, &cc))
        return e;
      sr.restricted = 1;
      sr.n_marked = mp.n_marked;
      sr.n_device_searches = mp.n_device_searches;
      sr.n_device_queries = mp.n_device_queries;
      sr.n_host_fallbacks = mp.n_host_fallbacks;
      sr.search_ms = mp.search_ms;
    }
    std::copy(cc.n_class, cc.n_class + 8, n_class);
    *n_scc = cc.n_scc;
    if (srch) *srch = sr;
    return 0;
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}
