// graph_host.cpp — the host code both Elle checkers run over a finished
// transaction graph (graph_host.h): real time's ranges, and the cycles by an
// iterative Tarjan, the class tests and a breadth-first witness search.
// g++, no GPU.
#include "graph_host.h"

#include <errno.h>

#include <algorithm>
#include <chrono>
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

namespace {

// The marked txns as a graph of their own: local ids in txn order, the edges
// with both ends marked under those ids (still sorted: the renaming is
// monotone), and real time's ranges over the marked OK txns by comp_pos.
// byc is the stable sort of the OK txns by comp_pos, so its marked entries
// are the stable sort of the marked OK txns, and the entries before index i
// of it are the txns below (comp_pos, txn) of byc[i].
struct MarkedGraph {
  std::vector<int32_t> ids;  // local -> txn
  std::vector<lc_ap_edge> edges;
  std::vector<int32_t> byc, lo, hi;

  int32_t local(int32_t t) const {  // -1: not marked
    const auto it = std::lower_bound(ids.begin(), ids.end(), t);
    return it != ids.end() && *it == t ? (int32_t)(it - ids.begin()) : -1;
  }

  void build(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *all, int64_t n_edges, const int32_t *full_byc,
             int64_t n_ok, const int32_t *rt_lo, const int32_t *rt_hi, const int32_t *mark) {
    for (int64_t t = 0; t < n_txns; t++)
      if (mark[t] && txns[t].type != LC_AP_FAIL) ids.push_back((int32_t)t);
    const size_t m = ids.size();
    // the edges are sorted by from: a marked txn's out-edges by two binary searches
    for (size_t u = 0; u < m; u++) {
      const int32_t t = ids[u];
      const lc_ap_edge *e = std::lower_bound(all, all + n_edges, t, [](const lc_ap_edge &x, int32_t f) { return x.from < f; });
      for (; e < all + n_edges && e->from == t; e++) {
        const int32_t v = local(e->to);
        if (v >= 0) edges.push_back(lc_ap_edge{(int32_t)u, v, e->type, 0, e->key});
      }
    }
    std::vector<int32_t> ok;  // marked OK txns (local), by (comp_pos, txn)
    for (size_t u = 0; u < m; u++)
      if (txns[ids[u]].type == LC_AP_OK) ok.push_back((int32_t)u);
    std::stable_sort(ok.begin(), ok.end(),
                     [&](int32_t a, int32_t b) { return txns[ids[(size_t)a]].comp_pos < txns[ids[(size_t)b]].comp_pos; });
    byc = ok;
    // the marked entries of full_byc before its index i
    auto before = [&](int64_t i) -> int32_t {
      if (i >= n_ok) return (int32_t)ok.size();
      const int32_t bt = full_byc[i];
      const int32_t bc = txns[bt].comp_pos;
      return (int32_t)(std::lower_bound(ok.begin(), ok.end(), 0,
                                        [&](int32_t a, int) {
                                          const int32_t at = ids[(size_t)a];
                                          return txns[at].comp_pos < bc || (txns[at].comp_pos == bc && at < bt);
                                        }) -
                       ok.begin());
    };
    lo.resize(m);
    hi.resize(m);
    for (size_t u = 0; u < m; u++) {
      const int32_t t = ids[u];
      lo[u] = hi[u] = 0;
      if (rt_hi[t] <= rt_lo[t]) continue;
      lo[u] = before(rt_lo[t]);
      hi[u] = before(rt_hi[t]);
    }
  }
};

}  // namespace

int cycles_host_marked(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
                       const int32_t *byc, int64_t n_ok, const int32_t *rt_lo, const int32_t *rt_hi, MarkedPass *mp,
                       int32_t *scc, int32_t *scc_class, lc_ap_step *out_steps, int64_t *cycle_off,
                       int32_t *cycle_scc, CycleCounts *counts) {
  CycleCounts s{};
  for (int64_t t = 0; t < n_txns; t++) scc[t] = scc_class[t] = -1;
  MarkedGraph mg;
  mg.build(txns, n_txns, edges, n_edges, byc, n_ok, rt_lo, rt_hi, mp->mark);
  const std::vector<int32_t> &ids = mg.ids;
  const size_t m = ids.size();
  mp->n_marked = (int64_t)m;
  Graph g;
  g.n = (int64_t)m;
  g.edges = mg.edges.data();
  g.n_edges = (int64_t)mg.edges.size();
  g.byc = mg.byc.data();
  g.lo = mg.lo.data();
  g.hi = mg.hi.data();
  g.init();
  std::vector<int32_t> nodes(m), lscc(m, -1);  // lscc: scc[] under the local ids
  for (size_t u = 0; u < m; u++) nodes[u] = (int32_t)u;
  const int32_t n_comp = g.scc(nodes, 15, nullptr, 0);
  // the nontrivial components, numbered by their least txn (the local ids ascend with the txns)
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
    lscc[(size_t)x] = id[(size_t)c];
    scc[ids[(size_t)x]] = id[(size_t)c];
    members[(size_t)id[(size_t)c]].push_back(x);
  }
  static const int kCt[4] = {LC_AP_WW, LC_AP_WR, LC_AP_RW, LC_AP_RW};
  static const int kMask[4] = {1, 3, 3, 7};
  int64_t n_steps = 0, n_cycles = 0;
  cycle_off[0] = 0;
  std::vector<lc_ap_step> steps;
  // scratch of the G-single searches: a member's index in its SCC, the
  // candidates with their heads, the SCC's predecessor lists
  std::vector<int32_t> midx(m, -1), q_node, q_heads, pred;
  std::vector<int64_t> q_head_off, pred_off;
  for (size_t c = 0; c < members.size(); c++) {
    const std::vector<int32_t> &mem = members[c];
    const int32_t tag = (int32_t)c;
    int32_t cls = -1;
    steps.clear();
    for (size_t i = 0; i < mem.size(); i++) midx[(size_t)mem[i]] = (int32_t)i;
    for (int k = 0; k < 8 && cls < 0; k++) {
      const int ct = kCt[k & 3], mask = kMask[k & 3] | (k >= 4 ? 8 : 0);
      g.scc(mem, mask | (1 << ct), lscc.data(), tag);
      // u's ct out-edges into its own component of mask + ct: cycle_from's opening test
      auto closes = [&](int32_t u, int32_t to) {
        return lscc[(size_t)to] == tag && g.comp[(size_t)to] == g.comp[(size_t)u];
      };
      if ((k & 3) != 2) {
        // ct belongs to mask, so the component is one of mask alone: the head
        // of a closing edge of u reaches u inside it, and the search from u
        // succeeds as soon as the opening test passes.  cycles_host's loop
        // stops at the first member whose search succeeds, which is the first
        // that passes the test; the members before it leave no trace.
        for (int32_t u : mem) {
          bool any = false;
          for (int64_t i = g.out_off[(size_t)u]; i < g.out_off[(size_t)u + 1] && !any; i++)
            any = g.edges[i].type == ct && closes(u, g.edges[i].to);
          if (!any) continue;
          if (g.cycle_from(u, ct, mask, lscc.data(), tag, &steps)) {
            cls = k;
            break;
          }
        }
        continue;
      }
      // G-single (k 2) and G-single-realtime (k 6): the component is one of
      // mask + rw, the search walks mask alone, so a candidate may search the
      // whole component and fail.  Which candidate is the first to succeed is
      // a ReachProblem over the SCC's members.
      q_node.clear();
      q_heads.clear();
      q_head_off.assign(1, 0);
      for (int32_t u : mem) {
        const size_t h0 = q_heads.size();
        for (int64_t i = g.out_off[(size_t)u]; i < g.out_off[(size_t)u + 1]; i++) {
          const lc_ap_edge &e = g.edges[i];
          if (e.type != ct || !closes(u, e.to)) continue;
          if (q_heads.size() > h0 && q_heads.back() == midx[(size_t)e.to]) continue;  // (one head, two keys)
          q_heads.push_back(midx[(size_t)e.to]);
        }
        if (q_heads.size() == h0) continue;
        q_node.push_back(midx[(size_t)u]);
        q_head_off.push_back((int64_t)q_heads.size());
      }
      if (q_node.empty()) continue;
      int64_t first = -2;  // -2: not asked
      if (mp->hook) {
        // the predecessors under mask, inside the components of mask + rw (a
        // path from a head to its source closes a cycle, so it stays in one)
        pred.clear();
        pred_off.assign(1, 0);
        for (int32_t b : mem) {
          const int64_t np = g.n_pred(b, mask);
          for (int64_t i = 0; i < np; i++) {
            int32_t type;
            int64_t key;
            const int32_t a = g.pred(b, mask, i, &type, &key);
            if (a < 0 || lscc[(size_t)a] != tag || g.comp[(size_t)a] != g.comp[(size_t)b]) continue;
            pred.push_back(midx[(size_t)a]);
          }
          pred_off.push_back((int64_t)pred.size());
        }
        const double work = (double)q_node.size() * (double)(mem.size() + pred.size());
        if (work >= (double)mp->min_work) {
          if ((int64_t)mem.size() > mp->max_nodes) {
            mp->n_host_fallbacks++;
          } else {
            const auto t0 = std::chrono::steady_clock::now();
            const ReachProblem rp{(int64_t)mem.size(), pred_off.data(), pred.data(),  (int64_t)q_node.size(),
                                  q_node.data(),       q_head_off.data(), q_heads.data()};
            int64_t fh = -1;
            const int rc = mp->hook(rp, &fh);
            mp->search_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc == -E2BIG) {
              mp->n_host_fallbacks++;
            } else if (rc) {
              return rc;
            } else if (fh < -1 || fh >= (int64_t)q_node.size()) {
              return -EIO;
            } else {
              mp->n_device_searches++;
              mp->n_device_queries += (int64_t)q_node.size();
              first = fh;
            }
          }
        }
      }
      if (first == -2) {  // the host loop, over the members that pass the opening test
        for (int32_t qn : q_node)
          if (g.cycle_from(mem[(size_t)qn], ct, mask, lscc.data(), tag, &steps)) {
            cls = k;
            break;
          }
      } else if (first >= 0) {
        if (!g.cycle_from(mem[(size_t)q_node[(size_t)first]], ct, mask, lscc.data(), tag, &steps)) return -EIO;
        cls = k;
      }
    }
    if (cls < 0) cls = LC_AP_G2_ITEM + LC_AP_REALTIME;  // (a nontrivial SCC is cyclic under every edge type)
    for (int32_t x : mem) {
      scc_class[ids[(size_t)x]] = cls;
      midx[(size_t)x] = -1;
    }
    s.n_class[cls]++;
    if (n_cycles < LC_AP_MAX_CYCLES) {
      for (const lc_ap_step &st : steps) out_steps[n_steps++] = lc_ap_step{ids[(size_t)st.txn], st.type, st.key};
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
  return 0;
}

void no_cycles(int64_t n_txns, int32_t *scc, int32_t *scc_class, int64_t *cycle_off, int32_t *cycle_scc,
               CycleCounts *counts) {
  for (int64_t t = 0; t < n_txns; t++) scc[t] = scc_class[t] = -1;
  for (int i = 0; i <= LC_AP_MAX_CYCLES; i++) cycle_off[i] = 0;
  for (int i = 0; i < LC_AP_MAX_CYCLES; i++) cycle_scc[i] = -1;
  *counts = CycleCounts{};
}

}  // namespace lcgraph
