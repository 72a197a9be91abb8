// cycles_dev.cpp — lc_cycle_reach's driver (include/lincheck_cycles.h): the
// graph and the queries copied to the context's first device, one launch
// (cycles.hip), the result word, the counts and, with LC_REACH_ALL, the hits
// copied back.  reach_problem is the same for the checkers' drivers
// (lc_append_check_restricted, lc_wr_check_restricted), whose class loop asks
// it from the host.
#include <algorithm>
#include <chrono>
#include <string>

#include "runtime.h"
// (after runtime.h: the launcher names HIP types)
#include "cycles.h"

using namespace lcrt;

namespace {

struct Pinned {
  int32_t words[2];
  unsigned long long counts[2 * lccyc::kMaxWorkgroups];
};

// The inputs are valid and n_nodes, n_queries > 0.
int reach_run(lc_ctx *c, int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_queries,
              const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads, uint32_t flags, int32_t *hit,
              lc_reach_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  if (n_nodes > lccyc::kMaxNodes) {
    set_err(c, "lc_cycle_reach: more nodes than lc_cycle_reach_limits' max_nodes");
    return -E2BIG;
  }
  const size_t nn = (size_t)n_nodes, nq = (size_t)n_queries, np = (size_t)pred_off[n_nodes],
               nh = (size_t)q_head_off[n_queries];
  const int n_wg = lccyc::workgroups(n_nodes, n_queries);
  SideState &s = c->cys;
  hipStream_t st;
  if (int e = side_begin(c, s, 4, sizeof(Pinned), &st)) return e;
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], k0 = s.ev[2], k1 = s.ev[3];
  Pinned &h = *s.words<Pinned>();
  lccyc::Ws w{};
  w.n_nodes = n_nodes;
  w.n_queries = n_queries;
  auto layout = [&](Carver ws) {
    w.pred_off = ws.take<int64_t>(nn + 1);
    w.pred = ws.take<int32_t>(np);
    w.q_node = ws.take<int32_t>(nq);
    w.q_head_off = ws.take<int64_t>(nq + 1);
    w.q_heads = ws.take<int32_t>(nh);
    w.queue = ws.take<int32_t>((size_t)n_wg * nn);
    w.hit = ws.take<int32_t>(nq);
    w.words = ws.take<int32_t>(2);
    w.counts = ws.take<unsigned long long>(2 * (size_t)n_wg);
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}))) return e;
  layout(Carver{s.arena.p});
  h.words[0] = INT32_MAX;  // no hit
  h.words[1] = 0;          // the first ticket
  HIP_TRY(c, hipEventRecord(e0, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.pred_off), pred_off, sizeof(int64_t) * (nn + 1), hipMemcpyHostToDevice, st));
  if (np) HIP_TRY(c, hipMemcpyAsync(writable(w.pred), pred, sizeof(int32_t) * np, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.q_node), q_node, sizeof(int32_t) * nq, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.q_head_off), q_head_off, sizeof(int64_t) * (nq + 1), hipMemcpyHostToDevice,
                            st));
  if (nh) HIP_TRY(c, hipMemcpyAsync(writable(w.q_heads), q_heads, sizeof(int32_t) * nh, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(w.words, h.words, sizeof(h.words), hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipEventRecord(e1, st));
  HIP_TRY(c, hipEventRecord(k0, st));
  HIP_TRY(c, lccyc::launch_reach(w, n_wg, flags, st));
  HIP_TRY(c, hipEventRecord(k1, st));
  HIP_TRY(c, hipMemcpyAsync(h.words, w.words, sizeof(h.words), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h.counts, w.counts, sizeof(unsigned long long) * 2 * (size_t)n_wg, hipMemcpyDeviceToHost,
                            st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int64_t first = h.words[0] == INT32_MAX ? -1 : h.words[0];
  if (first < -1 || first >= n_queries) {
    set_err(c, "lc_cycle_reach: the device named a query that does not exist");
    return -EIO;
  }
  // (the hits last: an error above has written nothing)
  if (flags & LC_REACH_ALL) {
    HIP_TRY(c, hipMemcpyAsync(hit, w.hit, sizeof(int32_t) * nq, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  lc_reach_summary sm{};
  sm.first_hit = first;
  for (int b = 0; b < n_wg; b++) {
    sm.n_queries_run += (int64_t)h.counts[2 * b];
    sm.nodes_visited += (int64_t)h.counts[2 * b + 1];
  }
  sm.h2d_ms = elapsed_ms(e0, e1);
  sm.kernel_ms = elapsed_ms(k0, k1);
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  return 0;
}

int reach_device(lc_ctx *c, int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred,
                 int64_t n_queries, const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads,
                 int64_t n_heads, uint32_t flags, int32_t *hit, lc_reach_summary *sum) {
  const char *why = nullptr;
  if (lccyc::validate(n_nodes, pred_off, pred, n_pred, n_queries, q_node, q_head_off, q_heads, n_heads, flags, hit,
                      &why)) {
    set_err(c, std::string("lc_cycle_reach: ") + why);
    return -EINVAL;
  }
  if (n_nodes == 0 || n_queries == 0)
    return lc_cycle_reach_host(n_nodes, pred_off, pred, n_pred, n_queries, q_node, q_head_off, q_heads, n_heads, flags,
                               hit, sum);
  return reach_run(c, n_nodes, pred_off, pred, n_queries, q_node, q_head_off, q_heads, flags, hit, sum);
}

}  // namespace

// The class loop's own arrays obey the contract by construction (graph_host.cpp).
int lccyc::reach_problem(lc_ctx *c, const lcgraph::ReachProblem &p, int64_t *first_hit) {
  lc_reach_summary sm;
  if (int e = reach_run(c, p.n_nodes, p.pred_off, p.pred, p.n_queries, p.q_node, p.q_head_off, p.q_heads, 0, nullptr,
                        &sm))
    return e;
  *first_hit = sm.first_hit;
  return 0;
}

void lccyc::device_pass(lc_ctx *c, const int32_t *mark, lcgraph::MarkedPass *mp) {
  mp->mark = mark;
  mp->min_work = lccyc::min_work();
  mp->max_nodes = lccyc::kMaxNodes;
  mp->hook = [c](const lcgraph::ReachProblem &p, int64_t *first_hit) { return reach_problem(c, p, first_hit); };
}

lc_cycle_search_summary lccyc::search_summary(const lcgraph::MarkedPass *mp) {
  lc_cycle_search_summary s{};
  if (!mp) return s;
  s.restricted = 1;
  s.n_marked = mp->n_marked;
  s.n_device_searches = mp->n_device_searches;
  s.n_device_queries = mp->n_device_queries;
  s.n_host_fallbacks = mp->n_host_fallbacks;
  s.search_ms = mp->search_ms;
  return s;
}

extern "C" int lc_cycle_reach(lc_ctx *c, int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred,
                              int64_t n_queries, const int32_t *q_node, const int64_t *q_head_off,
                              const int32_t *q_heads, int64_t n_heads, uint32_t flags, int32_t *hit,
                              lc_reach_summary *sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_cycle_reach", [&] {
    return reach_device(c, n_nodes, pred_off, pred, n_pred, n_queries, q_node, q_head_off, q_heads, n_heads, flags, hit,
                        sum);
  });
}
