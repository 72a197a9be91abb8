// cycles_main.cpp — lc_cycle_reach_host and lc_cycles_host (csrc/cycles_host.cpp,
// csrc/graph_host.cpp) as a stand-alone program for
// tests/test_cycles_host_sanitize.py, which builds it with the address and
// undefined-behaviour sanitizers.  It reads the cases the test wrote (argv[1]:
// n_reach, then per case n_nodes, n_pred, n_queries, n_heads, pred_off, pred,
// q_node, q_head_off, q_heads; then n_graphs, and per graph n_txns, n_edges,
// the txns, the edges) and generates graphs of its own.  Every output array
// is sized exactly.  One line per call: the code and the counts, judged by the
// test.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../include/lincheck_cycles.h"

namespace {

// An array of exactly n entries on the heap, n == 0 included: a write past
// it is the sanitizer's to find.
template <class T>
struct Exact {
  T *p;
  explicit Exact(size_t n) : p(new T[n]()) {}
  ~Exact() { delete[] p; }
  Exact(const Exact &) = delete;
  T &operator[](size_t i) { return p[i]; }
};

struct Reach {
  int64_t n_nodes = 0;
  std::vector<int64_t> pred_off{0}, q_head_off{0};
  std::vector<int32_t> pred, q_node, q_heads;
};

int run_reach(const char *name, int idx, const Reach &r) {
  const size_t nq = r.q_node.size();
  int rc[2];
  long long first[2] = {-9, -9}, visited[2] = {0, 0}, hits = 0;
  for (int all = 1; all >= 0; all--) {
    Exact<int32_t> hit(all ? nq : 0);
    lc_reach_summary s{};
    rc[all] = lc_cycle_reach_host(r.n_nodes, r.pred_off.data(), r.pred.data(), (int64_t)r.pred.size(), (int64_t)nq,
                                  r.q_node.data(), r.q_head_off.data(), r.q_heads.data(), (int64_t)r.q_heads.size(),
                                  all ? LC_REACH_ALL : 0u, all ? hit.p : nullptr, &s);
    if (rc[all]) continue;
    first[all] = s.first_hit;
    visited[all] = s.nodes_visited;
    for (size_t q = 0; all && q < nq; q++) hits += hit[q];
  }
  printf("%s %d rc %d rc_first %d first_hit %lld first_hit_early %lld hits %lld visited %lld visited_early %lld\n", name,
         idx, rc[1], rc[0], first[1], first[0], hits, visited[1], visited[0]);
  return rc[1];
}

// The host loop as a hook, through lc_cycle_reach_host itself.
int host_hook(void *user, int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_queries,
              const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads, int64_t *first_hit) {
  lc_reach_summary s{};
  const int rc = lc_cycle_reach_host(n_nodes, pred_off, pred, pred_off[n_nodes], n_queries, q_node, q_head_off, q_heads,
                                     q_head_off[n_queries], 0, nullptr, &s);
  *first_hit = s.first_hit;
  ++*static_cast<long long *>(user);
  return rc;
}

// Rule 7 three times: over the whole graph, over every txn as marked with the
// host loop, and with the hook.  The three must agree; the line carries the
// first one's counts.
int run_cycles(const char *name, int idx, const std::vector<lc_ap_txn> &txns, const std::vector<lc_ap_edge> &edges) {
  const size_t nt = txns.size();
  long long sums[3][4] = {}, asked = 0;
  int64_t n_scc[3] = {};
  int rc = 0;
  for (int pass = 0; pass < 3; pass++) {
    Exact<int32_t> scc(nt), cls(nt), cycle_scc(LC_AP_MAX_CYCLES), mark(nt);
    Exact<lc_ap_step> steps(nt);
    Exact<int64_t> cycle_off(LC_AP_MAX_CYCLES + 1), n_class(8);
    for (size_t t = 0; t < nt; t++) mark[t] = 1;
    lc_cycle_search_summary srch{};
    rc = lc_cycles_host(txns.data(), (int64_t)nt, edges.data(), (int64_t)edges.size(), pass ? mark.p : nullptr,
                        pass == 2 ? host_hook : nullptr, &asked, 0, 0, scc.p, cls.p, steps.p, cycle_off.p, cycle_scc.p,
                        n_class.p, &n_scc[pass], &srch);
    if (rc) break;
    for (size_t t = 0; t < nt; t++) {
      sums[pass][0] += scc[t];
      sums[pass][1] += cls[t];
    }
    for (int64_t i = 0; i < cycle_off[LC_AP_MAX_CYCLES]; i++) sums[pass][2] += steps[(size_t)i].txn * 3 + steps[(size_t)i].type;
    for (int k = 0; k < 8; k++) sums[pass][3] += (k + 1) * n_class[(size_t)k];
  }
  bool same = true;
  for (int pass = 1; pass < 3; pass++)
    for (int f = 0; f < 4; f++) same = same && sums[pass][f] == sums[0][f] && n_scc[pass] == n_scc[0];
  printf("%s %d rc %d same %d n_scc %lld scc %lld cls %lld steps %lld classes %lld asked %lld\n", name, idx, rc,
         (int)same, (long long)n_scc[0], sums[0][0], sums[0][1], sums[0][2], sums[0][3], asked);
  return rc;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % n;
}

Reach gen_reach(int n, int n_edges, int every) {
  Reach r;
  r.n_nodes = n;
  std::vector<std::vector<int32_t>> lists((size_t)n);
  for (int e = 0; e < n_edges && n; e++) lists[rnd((uint32_t)n)].push_back((int32_t)rnd((uint32_t)n));
  for (int b = 0; b < n; b++) {
    r.pred.insert(r.pred.end(), lists[(size_t)b].begin(), lists[(size_t)b].end());
    r.pred_off.push_back((int64_t)r.pred.size());
  }
  for (int s = 0; s < n; s += every) {
    r.q_node.push_back(s);
    for (uint32_t h = rnd(4); h > 0; h--) {
      const int32_t x = (int32_t)rnd((uint32_t)n);
      if (x != s) r.q_heads.push_back(x);
    }
    r.q_head_off.push_back((int64_t)r.q_heads.size());
  }
  return r;
}

// As tests/screen_main.cpp's: n_txns txns invoked at even positions and
// completed at odd ones up to 2 * width later; n_edges edges between nodes at
// most 2 * width apart, one in `back` against txn order.
void gen_graph(int n_txns, int n_edges, int width, int back, std::vector<lc_ap_txn> *txns,
               std::vector<lc_ap_edge> *edges) {
  txns->clear();
  edges->clear();
  std::vector<uint8_t> used(2 * (size_t)(n_txns + width) + 4, 0);
  std::vector<int32_t> nodes;
  for (int t = 0; t < n_txns; t++) {
    const uint32_t r = rnd(100);
    const int32_t type = r < 8 ? LC_AP_INFO : r < 16 ? LC_AP_FAIL : LC_AP_OK;
    int32_t comp = -1;
    if (type != LC_AP_INFO) {
      comp = 2 * (t + (int32_t)rnd((uint32_t)width + 1)) + 1;
      while (used[(size_t)comp]) comp += 2;
      used[(size_t)comp] = 1;
    }
    txns->push_back(lc_ap_txn{0, 2 * t, comp, type, 0});
    if (type != LC_AP_FAIL) nodes.push_back(t);
  }
  if (nodes.size() < 2) return;
  for (int e = 0; e < n_edges; e++) {
    size_t i = rnd((uint32_t)nodes.size()), j = i + 1 + rnd(2 * (uint32_t)width);
    if (j >= nodes.size()) i = nodes.size() - 2, j = nodes.size() - 1;
    if (back && rnd((uint32_t)back) == 0) std::swap(i, j);
    edges->push_back(lc_ap_edge{nodes[i], nodes[j], (int32_t)rnd(3), 0, (int64_t)rnd(5)});
  }
  const auto less = [](const lc_ap_edge &a, const lc_ap_edge &b) {
    if (a.from != b.from) return a.from < b.from;
    if (a.to != b.to) return a.to < b.to;
    if (a.type != b.type) return a.type < b.type;
    return a.key < b.key;
  };
  std::sort(edges->begin(), edges->end(), less);
  edges->erase(std::unique(edges->begin(), edges->end(),
                           [&](const lc_ap_edge &a, const lc_ap_edge &b) { return !less(a, b) && !less(b, a); }),
               edges->end());
}

template <class T>
bool read_vec(FILE *f, std::vector<T> *v, int64_t n) {
  v->resize((size_t)n);
  return n == 0 || fread(v->data(), sizeof(T), (size_t)n, f) == (size_t)n;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, f) != 1) return 2;
  for (int64_t c = 0; c < n_cases; c++) {
    int64_t n[4];
    Reach r;
    if (fread(n, 8, 4, f) != 4) return 2;
    r.n_nodes = n[0];
    if (!read_vec(f, &r.pred_off, n[0] + 1) || !read_vec(f, &r.pred, n[1]) || !read_vec(f, &r.q_node, n[2]) ||
        !read_vec(f, &r.q_head_off, n[2] + 1) || !read_vec(f, &r.q_heads, n[3]))
      return 2;
    run_reach("reach", (int)c, r);
  }
  if (fread(&n_cases, 8, 1, f) != 1) return 2;
  std::vector<lc_ap_txn> txns;
  std::vector<lc_ap_edge> edges;
  for (int64_t c = 0; c < n_cases; c++) {
    int64_t n[2];
    if (fread(n, 8, 2, f) != 2 || !read_vec(f, &txns, n[0]) || !read_vec(f, &edges, n[1])) return 2;
    run_cycles("graph", (int)c, txns, edges);
  }
  fclose(f);
  // (n_nodes, n_edges, a query every so many nodes)
  const int reach_shapes[][3] = {{0, 0, 1}, {1, 0, 1}, {2, 2, 1}, {64, 100, 1}, {65, 300, 2}, {300, 400, 1}, {1000, 1500, 7}};
  int i = 0;
  for (const auto &sh : reach_shapes) run_reach("gen-reach", i++, gen_reach(sh[0], sh[1], sh[2]));
  // (n_txns, n_edges, width, back)
  const int shapes[][4] = {{0, 0, 1, 0},    {1, 0, 1, 0},       {2, 3, 1, 2},        {64, 100, 4, 0},   {65, 200, 4, 3},
                           {300, 900, 8, 10}, {300, 900, 30, 2}, {1000, 3000, 6, 50}, {1500, 6000, 10, 40}};
  i = 0;
  for (const auto &sh : shapes) {
    gen_graph(sh[0], sh[1], sh[2], sh[3], &txns, &edges);
    run_cycles("gen-graph", i++, txns, edges);
  }
  // refusals: nothing may be written, whatever the arrays' size
  Reach bad = gen_reach(40, 80, 1);
  std::swap(bad.q_node[3], bad.q_node[4]);
  run_reach("unsorted-queries", 0, bad);
  bad = gen_reach(40, 80, 1);
  bad.pred[0] = 40;
  run_reach("pred-out-of-range", 0, bad);
  bad = gen_reach(40, 80, 1);
  bad.q_heads[0] = bad.q_node[0];
  bad.q_head_off[1] = std::max<int64_t>(bad.q_head_off[1], 1);
  run_reach("head-is-source", 0, bad);
  return 0;
}
