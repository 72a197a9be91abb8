// graph_host.cpp — the host code both Elle checkers run over a finished
// transaction graph (graph_host.h): real time's ranges, and the cycles by an
// iterative Tarjan, the class tests and a breadth-first witness search.
// g++, no GPU.
#include "graph_host.h"

#include <algorithm>
#include <utility>
#include <vector>

namespace lcgraph {

void real_time_host(const lc_ap_txn *txns, int64_t n_txns, int32_t *byc, int32_t *rt_lo, int32_t *rt_hi) {
  int64_t n_ok = 0;
  for (int64_t t = 0; t < n_txns; t++)
    if (txns[t].type == LC_AP_OK) byc[n_ok++] = (int32_t)t;
  std::stable_sort(byc, byc + n_ok, [&](int32_t a, int32_t b) { return txns[a].comp_pos < txns[b].comp_pos; });
  std::vector<int32_t> comp((size_t)n_ok), pm((size_t)n_ok);
  for (int64_t i = 0; i < n_ok; i++) {
    comp[(size_t)i] = txns[byc[i]].comp_pos;
    pm[(size_t)i] = std::max(i ? pm[(size_t)i - 1] : -1, txns[byc[i]].inv_pos);
  }
  for (int64_t t = 0; t < n_txns; t++) {
    rt_lo[t] = rt_hi[t] = 0;
    if (txns[t].type == LC_AP_FAIL) continue;
    const int64_t hi = std::lower_bound(comp.begin(), comp.end(), txns[t].inv_pos) - comp.begin();
    if (hi == 0) continue;
    const int32_t m = pm[(size_t)hi - 1];
    rt_lo[t] = (int32_t)(std::upper_bound(comp.begin(), comp.end(), m) - comp.begin());
    rt_hi[t] = (int32_t)hi;
  }
}

namespace {

// The graph, walked against its edges: SCCs, cycles and "v reaches u" are the
// same in the transposed graph, and a txn's real-time predecessors are a
// range where its successors are not.
struct Graph {
  int64_t n;
  const lc_ap_edge *edges;
  int64_t n_edges;
  const int32_t *byc, *lo, *hi;
  std::vector<int64_t> in_off, out_off;  // edges by to (through in_idx) and by from (they are sorted so)
  std::vector<int32_t> in_idx;
  // scratch of scc(): index 0 means unvisited
  std::vector<int32_t> index, low, comp, stack;
  std::vector<uint8_t> on_stack;
  std::vector<std::pair<int32_t, int64_t>> frames;
  // scratch of the searches
  std::vector<int32_t> mark, par, par_type, queue;
  std::vector<int64_t> par_key;
  int32_t mark_now = 0;

  int64_t n_pred(int32_t b, int mask) const {
    return in_off[(size_t)b + 1] - in_off[(size_t)b] + ((mask & 8) ? hi[b] - lo[b] : 0);
  }
  // the i-th predecessor of b under mask, or -1 where its edge is not in mask
  int32_t pred(int32_t b, int mask, int64_t i, int32_t *type, int64_t *key) const {
    const int64_t n_in = in_off[(size_t)b + 1] - in_off[(size_t)b];
    if (i < n_in) {
      const lc_ap_edge &e = edges[in_idx[(size_t)(in_off[(size_t)b] + i)]];
      *type = e.type;
      *key = e.key;
      return ((mask >> e.type) & 1) ? e.from : -1;
    }
    *type = LC_AP_RT;
    *key = 0;
    return byc[lo[b] + (i - n_in)];
  }

  void init() {
    in_off.assign((size_t)n + 1, 0);
    out_off.assign((size_t)n + 1, 0);
    for (int64_t i = 0; i < n_edges; i++) {
      in_off[(size_t)edges[i].to + 1]++;
      out_off[(size_t)edges[i].from + 1]++;
    }
    for (int64_t t = 0; t < n; t++) {
      in_off[(size_t)t + 1] += in_off[(size_t)t];
      out_off[(size_t)t + 1] += out_off[(size_t)t];
    }
    in_idx.resize((size_t)n_edges);
    std::vector<int64_t> at(in_off.begin(), in_off.end() - 1);
    for (int64_t i = 0; i < n_edges; i++) in_idx[(size_t)at[(size_t)edges[i].to]++] = (int32_t)i;
    index.assign((size_t)n, 0);
    low.assign((size_t)n, 0);
    comp.assign((size_t)n, -1);
    on_stack.assign((size_t)n, 0);
    mark.assign((size_t)n, 0);
    par.assign((size_t)n, -1);
    par_type.assign((size_t)n, 0);
    par_key.assign((size_t)n, 0);
  }

  // Tarjan, iterative, over `nodes` under mask, staying where region[x] ==
  // tag (region null: everywhere).  comp[x] of every node is set to its
  // component's number (0 .. return value - 1); index / low are left clean.
  int32_t scc(const std::vector<int32_t> &nodes, int mask, const int32_t *region, int32_t tag) {
    int32_t n_comp = 0, counter = 0;
    for (int32_t root : nodes) {
      if (index[(size_t)root]) continue;
      frames.assign(1, {root, 0});
      index[(size_t)root] = low[(size_t)root] = ++counter;
      stack.push_back(root);
      on_stack[(size_t)root] = 1;
      while (!frames.empty()) {
        const int32_t v = frames.back().first;
        int64_t &i = frames.back().second;
        if (i < n_pred(v, mask)) {
          int32_t type;
          int64_t key;
          const int32_t u = pred(v, mask, i++, &type, &key);
          if (u < 0 || (region && region[u] != tag)) continue;
          if (!index[(size_t)u]) {
            index[(size_t)u] = low[(size_t)u] = ++counter;
            stack.push_back(u);
            on_stack[(size_t)u] = 1;
            frames.push_back({u, 0});
          } else if (on_stack[(size_t)u]) {
            low[(size_t)v] = std::min(low[(size_t)v], index[(size_t)u]);
          }
          continue;
        }
        if (low[(size_t)v] == index[(size_t)v]) {
          int32_t x;
          do {
            x = stack.back();
            stack.pop_back();
            on_stack[(size_t)x] = 0;
            comp[(size_t)x] = n_comp;
          } while (x != v);
          n_comp++;
        }
        frames.pop_back();
        if (!frames.empty()) {
          const int32_t up = frames.back().first;
          low[(size_t)up] = std::min(low[(size_t)up], low[(size_t)v]);
        }
      }
    }
    for (int32_t x : nodes) index[(size_t)x] = low[(size_t)x] = 0;
    return n_comp;
  }

  // Breadth first from u against the edges of mask, inside region[] == tag and
  // comp[] == comp[u]:
  // the first out-edge of u of type ct whose head v is met gives the cycle
  // u -ct-> v -> ... -> u.  Its steps go to `steps`; false if there is none.
  bool cycle_from(int32_t u, int ct, int mask, const int32_t *region, int32_t tag, std::vector<lc_ap_step> *steps) {
    const int32_t cu = comp[(size_t)u];
    int32_t now = ++mark_now;
    // the candidates: heads of u's ct edges inside the component
    bool any = false;
    for (int64_t i = out_off[(size_t)u]; i < out_off[(size_t)u + 1]; i++)
      if (edges[i].type == ct && region[edges[i].to] == tag && comp[(size_t)edges[i].to] == cu) any = true;
    if (!any) return false;
    queue.assign(1, u);
    mark[(size_t)u] = now;
    auto is_head = [&](int32_t x, int64_t *key) {
      for (int64_t i = out_off[(size_t)u]; i < out_off[(size_t)u + 1]; i++)
        if (edges[i].type == ct && edges[i].to == x) {
          *key = edges[i].key;
          return true;
        }
      return false;
    };
    for (size_t q = 0; q < queue.size(); q++) {
      const int32_t b = queue[q];
      const int64_t np = n_pred(b, mask);
      for (int64_t i = 0; i < np; i++) {
        int32_t type;
        int64_t key;
        const int32_t a = pred(b, mask, i, &type, &key);
        if (a < 0 || region[a] != tag || comp[(size_t)a] != cu || mark[(size_t)a] == now) continue;
        mark[(size_t)a] = now;
        par[(size_t)a] = b;  // a -type/key-> b lies on a's way to u
        par_type[(size_t)a] = type;
        par_key[(size_t)a] = key;
        int64_t ck;
        if (is_head(a, &ck)) {
          steps->push_back({u, ct, ck});
          for (int32_t x = a; x != u; x = par[(size_t)x])
            steps->push_back({x, par_type[(size_t)x], par_key[(size_t)x]});
          return true;
        }
        queue.push_back(a);
      }
    }
    return false;
  }
};

}  // namespace

void cycles_host(const lc_ap_txn *txns, int64_t n_txns, int64_t n_nodes, const lc_ap_edge *edges, int64_t n_edges,
                 const int32_t *byc, const int32_t *rt_lo, const int32_t *rt_hi, int32_t *scc, int32_t *scc_class,
                 lc_ap_step *out_steps, int64_t *cycle_off, int32_t *cycle_scc, CycleCounts *counts) {
  CycleCounts s{};
  Graph g;
  g.n = n_txns;
  g.edges = edges;
  g.n_edges = n_edges;
  g.byc = byc;
  g.lo = rt_lo;
  g.hi = rt_hi;
  g.init();
  std::vector<int32_t> nodes;
  nodes.reserve((size_t)n_nodes);
  for (int64_t t = 0; t < n_txns; t++) {
    scc[t] = scc_class[t] = -1;
    if (txns[t].type != LC_AP_FAIL) nodes.push_back((int32_t)t);
  }
  const int32_t n_comp = g.scc(nodes, 15, nullptr, 0);
  // the nontrivial components, numbered by their least txn
  std::vector<int32_t> size((size_t)n_comp, 0), id((size_t)n_comp, -1);
  for (int32_t x : nodes) size[(size_t)g.comp[(size_t)x]]++;
  std::vector<std::vector<int32_t>> members;
  for (int32_t x : nodes) {
    const int32_t c = g.comp[(size_t)x];
    if (size[(size_t)c] < 2) continue;
    if (id[(size_t)c] < 0) {
      id[(size_t)c] = (int32_t)members.size();
      members.emplace_back();
    }
    scc[x] = id[(size_t)c];
    members[(size_t)id[(size_t)c]].push_back(x);
  }
  static const int kCt[4] = {LC_AP_WW, LC_AP_WR, LC_AP_RW, LC_AP_RW};
  static const int kMask[4] = {1, 3, 3, 7};
  int64_t n_steps = 0, n_cycles = 0;
  cycle_off[0] = 0;
  std::vector<lc_ap_step> steps;
  for (size_t c = 0; c < members.size(); c++) {
    const std::vector<int32_t> &mem = members[c];
    int32_t cls = -1;
    steps.clear();
    for (int k = 0; k < 8 && cls < 0; k++) {
      const int ct = kCt[k & 3], mask = kMask[k & 3] | (k >= 4 ? 8 : 0);
      // a cycle closed by a ct edge lies inside one component of mask + ct
      g.scc(mem, mask | (1 << ct), scc, (int32_t)c);
      for (int32_t u : mem)
        if (g.cycle_from(u, ct, mask, scc, (int32_t)c, &steps)) {
          cls = k;
          break;
        }
    }
    if (cls < 0) cls = LC_AP_G2_ITEM + LC_AP_REALTIME;  // (a nontrivial SCC is cyclic under every edge type)
    for (int32_t x : mem) scc_class[x] = cls;
    s.n_class[cls]++;
    if (n_cycles < LC_AP_MAX_CYCLES) {
      for (const lc_ap_step &st : steps) out_steps[n_steps++] = st;
      cycle_scc[n_cycles] = (int32_t)c;
      cycle_off[++n_cycles] = n_steps;
    }
  }
  for (int64_t i = n_cycles; i < LC_AP_MAX_CYCLES; i++) {
    cycle_off[i + 1] = n_steps;
    cycle_scc[i] = -1;
  }
  s.n_scc = (int64_t)members.size();
  s.n_cycles_returned = n_cycles;
  *counts = s;
}

void no_cycles(int64_t n_txns, int32_t *scc, int32_t *scc_class, int64_t *cycle_off, int32_t *cycle_scc,
               CycleCounts *counts) {
  for (int64_t t = 0; t < n_txns; t++) scc[t] = scc_class[t] = -1;
  for (int i = 0; i <= LC_AP_MAX_CYCLES; i++) cycle_off[i] = 0;
  for (int i = 0; i < LC_AP_MAX_CYCLES; i++) cycle_scc[i] = -1;
  *counts = CycleCounts{};
}

}  // namespace lcgraph
