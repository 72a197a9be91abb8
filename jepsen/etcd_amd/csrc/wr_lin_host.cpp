// wr_lin_host.cpp — lc_wr_check_lin_host: the rules of include/lincheck_wrlin.h
// on the host, single-threaded, with hash maps and per-key sorted vectors.
// Rules 1-3 and 5 as wr_host.cpp has them; rule 4' by the range form over each
// key's touches; rule 6' is Tarjan's SCCs per key over an explicit edge list
// (nothing here mirrors the device's bit matrices); rule 9 and the summary are
// wr_host.cpp's graph_and_summary.  g++, no GPU.
#include <errno.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <unordered_map>

#include "wr_lin.h"

namespace lcwr {

bool lin_flags_ok(uint32_t flags) { return !(flags & ~(LC_WR_WFR_KEYS | LC_WR_LINEARIZABLE_KEYS)); }

void lin_zero(lc_wr_lin_key *lin_keys, int64_t n_keys, lc_wr_lin_summary *lin_sum) {
  std::fill(lin_keys, lin_keys + n_keys, lc_wr_lin_key{});
  if (lin_sum) *lin_sum = lc_wr_lin_summary{};
}

}  // namespace lcwr

extern "C" int lc_wr_lin_limits(lc_wr_lin_limit_info *out) {
  if (!out) return -EINVAL;
  out->max_key_versions = lcwr::kMaxKeyVersions;
  out->wave_key_versions = lcwr::kWaveKeyVersions;
  return 0;
}

namespace {

struct Version {
  int64_t value;
  int32_t kid;
  int32_t local;        // its index among the key's versions
  int32_t writer = -1;  // the write mop
  int32_t n_rw = 0;     // external readers whose txn writes the key (rule 5)
  std::vector<int32_t> readers;  // the txns with an external read of it
};

struct Touch {
  int32_t inv, comp;
  int32_t first, last;  // versions
};

struct Key {
  int64_t key;
  int64_t cyc_value = LC_WR_NIL;
  int32_t flags = 0, n_writes = 0, n_versions = 1, n_ext_reads = 0;
  int32_t nil = -1;       // the version (key, nil), once somebody read it
  int64_t n_init = 0;     // initial edges whose tail nobody read (they take part in no cycle and no txn edge)
  int64_t n_pairs = 0;
  std::vector<int32_t> vers;  // the key's versions, local order
  std::vector<Touch> touches;  // ascending by inv (txn order)
  std::vector<std::pair<int32_t, int32_t>> vedges;  // (tail, head) as local indices; sorted, unique once built
};

// Rule 6' on one key: Tarjan over its version edges, iteratively.  A version
// lies on a cycle iff its SCC has two members or it has a self-loop.
void mark_cycles(Key &k, const std::vector<Version> &vers) {
  const int32_t n = (int32_t)k.vers.size();
  std::vector<int32_t> off((size_t)n + 1, 0), adj(k.vedges.size());
  for (const auto &e : k.vedges) off[(size_t)e.first + 1]++;
  for (int32_t i = 0; i < n; i++) off[(size_t)i + 1] += off[(size_t)i];
  for (size_t i = 0; i < k.vedges.size(); i++) adj[i] = k.vedges[i].second;  // (sorted by tail: already grouped)
  std::vector<int32_t> index((size_t)n, -1), low((size_t)n, 0), next((size_t)n, 0), stack, call;
  std::vector<uint8_t> on_stack((size_t)n, 0);
  int32_t counter = 0;
  auto on_cycle = [&](int32_t v) {
    const int64_t val = vers[(size_t)k.vers[(size_t)v]].value;
    if (val == LC_WR_NIL) return;
    if (!(k.flags & LC_WR_K_CYCLIC) || val < k.cyc_value) k.cyc_value = val;
    k.flags |= LC_WR_K_CYCLIC;
  };
  for (int32_t r = 0; r < n; r++) {
    if (index[(size_t)r] >= 0) continue;
    call.push_back(r);
    while (!call.empty()) {
      const int32_t v = call.back();
      if (index[(size_t)v] < 0) {
        index[(size_t)v] = low[(size_t)v] = counter++;
        next[(size_t)v] = off[(size_t)v];
        stack.push_back(v);
        on_stack[(size_t)v] = 1;
      }
      if (next[(size_t)v] < off[(size_t)v + 1]) {
        const int32_t u = adj[(size_t)next[(size_t)v]++];
        if (index[(size_t)u] < 0) call.push_back(u);
        else if (on_stack[(size_t)u]) low[(size_t)v] = std::min(low[(size_t)v], index[(size_t)u]);
        continue;
      }
      call.pop_back();
      if (!call.empty()) low[(size_t)call.back()] = std::min(low[(size_t)call.back()], low[(size_t)v]);
      if (low[(size_t)v] != index[(size_t)v]) continue;
      const bool many = stack.back() != v;
      int32_t u;
      do {
        u = stack.back();
        stack.pop_back();
        on_stack[(size_t)u] = 0;
        if (many) on_cycle(u);
      } while (u != v);
    }
  }
  for (const auto &e : k.vedges)
    if (e.first == e.second) on_cycle(e.first);  // (a self-loop's version is never nil: nobody writes nil)
}

int wr_lin_host(const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops, uint32_t flags,
                const lc_wr_out *out, lc_wr_summary *sum, lc_wr_lin_key *lin_keys, lc_wr_lin_summary *lin_sum) {
  using namespace lcwr;
  const auto t0 = std::chrono::steady_clock::now();
  Prep p;
  const char *why = nullptr;
  if (!lin_flags_ok(flags) || !lin_keys) return -EINVAL;
  if (int rc = prepare(txns, n_txns, mops, n_mops, flags & LC_WR_WFR_KEYS, out, &p, &why)) return rc;
  if (!(flags & LC_WR_LINEARIZABLE_KEYS)) {
    lc_wr_summary s;
    if (int rc = lc_wr_check_host(txns, n_txns, mops, n_mops, flags, out, &s)) {
      if (rc == -ENOSPC && sum) *sum = s;
      return rc;
    }
    if (sum) *sum = s;
    lin_zero(lin_keys, s.n_keys, lin_sum);
    return 0;
  }
  const bool wfr = flags & LC_WR_WFR_KEYS;
  // the keys and the versions: every write and every known read names one
  std::unordered_map<int64_t, int32_t> key_id;
  std::unordered_map<std::pair<int64_t, int64_t>, int32_t, PairHash> ver_id;
  std::vector<Key> keys;
  std::vector<Version> vers;
  std::vector<int32_t> mop_key((size_t)n_mops), mop_ver((size_t)n_mops, -1);
  std::vector<uint8_t> last((size_t)n_mops, 0);
  for (int64_t m = 0; m < n_mops; m++) {
    const lc_wr_mop &o = mops[m];
    const auto kit = key_id.emplace(o.key, (int32_t)keys.size());
    if (kit.second) {
      keys.emplace_back();
      keys.back().key = o.key;
    }
    const int32_t kid = mop_key[(size_t)m] = kit.first->second;
    if (o.f == LC_WR_READ && !o.known) continue;
    const auto vit = ver_id.emplace(std::make_pair(o.key, o.value), (int32_t)vers.size());
    if (vit.second) {
      Key &k = keys[(size_t)kid];
      vers.emplace_back();
      vers.back().value = o.value;
      vers.back().kid = kid;
      vers.back().local = (int32_t)k.vers.size();
      k.vers.push_back(vit.first->second);
      if (o.value == LC_WR_NIL) k.nil = vit.first->second;
      else k.n_versions++;
    }
    mop_ver[(size_t)m] = vit.first->second;
    if (o.f != LC_WR_WRITE) continue;
    keys[(size_t)kid].n_writes++;
    Version &v = vers[(size_t)vit.first->second];
    if (v.writer >= 0) return -EINVAL;  // rule 1: two writes of one pair
    v.writer = (int32_t)m;
    const lc_wr_txn &x = txns[p.mop_txn[(size_t)m]];
    last[(size_t)m] = 1;
    for (int64_t j = m + 1; j < x.mop_off + x.mop_len; j++)
      if (mops[j].f == LC_WR_WRITE && mops[j].key == o.key) last[(size_t)m] = 0;
  }
  auto is_node = [&](int32_t t) { return txns[t].type != LC_WR_FAIL; };
  auto vedge = [&](int32_t a, int32_t b) {  // versions of one key
    keys[(size_t)vers[(size_t)a].kid].vedges.emplace_back(vers[(size_t)a].local, vers[(size_t)b].local);
  };
  // rules 2, 3 and 5; the wfr edges; the touches of rule 4' (the txns come ascending by inv)
  std::vector<int32_t> mop_flags((size_t)n_mops, 0), txn_flags((size_t)n_txns, 0);
  int64_t counts[kCounters] = {0};
  for (int64_t t = 0; t < n_txns; t++) {
    const lc_wr_txn &x = txns[t];
    if (x.type != LC_WR_OK) continue;
    int32_t tf = 0;
    const int64_t end = x.mop_off + x.mop_len;
    for (int64_t m = x.mop_off; m < end; m++) {
      const lc_wr_mop &o = mops[m];
      int64_t prev = -1;
      for (int64_t j = m - 1; j >= x.mop_off && prev < 0; j--)
        if (mops[j].key == o.key) prev = j;
      int64_t mb = -1;  // the txn's external write of the key, from here on
      for (int64_t j = m; j < end; j++)
        if (mops[j].f == LC_WR_WRITE && mops[j].key == o.key) mb = j;
      if (prev < 0) {  // the txn's first mop on the key: its touch
        const int32_t ext = o.f == LC_WR_READ ? mop_ver[(size_t)m] : -1;
        const int32_t wv = mb >= 0 ? mop_ver[(size_t)mb] : -1;
        keys[(size_t)mop_key[(size_t)m]].touches.push_back(
            Touch{(int32_t)x.inv_pos, (int32_t)x.comp_pos, ext >= 0 ? ext : wv, wv >= 0 ? wv : ext});
      }
      if (o.f != LC_WR_READ) continue;
      int32_t f = 0;
      if (prev < 0) f |= LC_WR_R_EXTERNAL;
      else if (mops[prev].value != o.value) f |= LC_WR_R_INTERNAL;
      Version &a = vers[(size_t)mop_ver[(size_t)m]];
      if (o.value != LC_WR_NIL) {
        if (a.writer < 0) {
          f |= LC_WR_R_PHANTOM;
        } else {
          const int32_t tw = p.mop_txn[(size_t)a.writer];
          if (txns[tw].type == LC_WR_FAIL) f |= LC_WR_R_G1A;
          if (tw != t && !last[(size_t)a.writer]) f |= LC_WR_R_G1B;
        }
      }
      for (int b = 0; b < 4; b++) counts[b] += (f >> b) & 1;
      mop_flags[(size_t)m] = f;
      tf |= f & LC_WR_R_ANOMALY;
      if (!(f & LC_WR_R_EXTERNAL)) continue;
      a.readers.push_back((int32_t)t);
      keys[(size_t)a.kid].n_ext_reads++;
      if (mb < 0) continue;
      if (++a.n_rw == 2) {
        counts[4]++;
        keys[(size_t)a.kid].flags |= LC_WR_K_LOST_UPDATE;
      }
      if (wfr) vedge(mop_ver[(size_t)m], mop_ver[(size_t)mb]);  // (a self-loop where they are one)
    }
    txn_flags[(size_t)t] = tf;
  }
  // the initial edges
  for (int64_t m = 0; m < n_mops; m++) {
    if (mops[m].f != LC_WR_WRITE || !is_node(p.mop_txn[(size_t)m])) continue;
    Key &k = keys[(size_t)mop_key[(size_t)m]];
    if (k.nil >= 0) vedge(k.nil, mop_ver[(size_t)m]);
    else k.n_init++;
  }
  // rule 4', the range form; then each key's edges as a set, and rule 6'
  int64_t max_versions = 0;
  for (Key &k : keys) {
    const size_t n = k.touches.size();
    std::vector<int32_t> sufmin(n + 1, INT32_MAX);  // the least comp from a touch on
    for (size_t i = n; i-- > 0;) sufmin[i] = std::min(sufmin[i + 1], k.touches[i].comp);
    auto by_inv = [](const Touch &a, int32_t pos) { return a.inv < pos; };
    for (size_t i = 0; i < n; i++) {
      const Touch &a = k.touches[i];
      const size_t lb = std::upper_bound(k.touches.begin(), k.touches.end(), a.comp,
                                         [](int32_t pos, const Touch &b) { return pos < b.inv; }) -
                        k.touches.begin();
      if (lb == n) continue;
      const size_t ub = std::lower_bound(k.touches.begin() + (ptrdiff_t)lb, k.touches.end(), sufmin[lb], by_inv) -
                        k.touches.begin();
      k.n_pairs += (int64_t)(ub - lb);
      for (size_t j = lb; j < ub; j++)
        if (a.last != k.touches[j].first) vedge(a.last, k.touches[j].first);
    }
    std::sort(k.vedges.begin(), k.vedges.end());
    k.vedges.erase(std::unique(k.vedges.begin(), k.vedges.end()), k.vedges.end());
    mark_cycles(k, vers);
    max_versions = std::max<int64_t>(max_versions, (int64_t)k.vers.size());
  }
  // rule 7'
  std::vector<lc_wr_edge> edges;
  auto emit = [&](int32_t from, int32_t to, int32_t type, int64_t key) {
    if (is_node(from) && is_node(to) && from != to) edges.push_back(lc_wr_edge{from, to, type, 0, key});
  };
  for (const Version &a : vers)
    if (a.writer >= 0)
      for (int32_t t : a.readers) emit(p.mop_txn[(size_t)a.writer], t, LC_AP_WR, keys[(size_t)a.kid].key);
  for (const Key &k : keys) {
    if (k.flags & LC_WR_K_CYCLIC) continue;
    for (const auto &e : k.vedges) {
      const Version &a = vers[(size_t)k.vers[(size_t)e.first]], &b = vers[(size_t)k.vers[(size_t)e.second]];
      if (b.writer < 0) continue;  // nil or a phantom at the head
      const int32_t w = p.mop_txn[(size_t)b.writer];
      if (a.writer >= 0) emit(p.mop_txn[(size_t)a.writer], w, LC_AP_WW, k.key);
      for (int32_t t : a.readers) emit(t, w, LC_AP_RW, k.key);
    }
  }
  const int64_t n_raw = (int64_t)edges.size();
  std::sort(edges.begin(), edges.end(), edge_less);
  edges.erase(std::unique(edges.begin(), edges.end(), edge_same), edges.end());
  const int64_t n_edges = (int64_t)edges.size();
  if (n_edges > out->edge_cap) {
    if (sum) {
      *sum = lc_wr_summary{};
      sum->n_edges = n_edges;
      sum->n_edges_raw = n_raw;
    }
    return -ENOSPC;
  }
  // nothing was written so far; from here nothing fails
  std::copy(mop_flags.begin(), mop_flags.end(), out->mop_flags);
  std::copy(txn_flags.begin(), txn_flags.end(), out->txn_flags);
  std::copy(edges.begin(), edges.end(), out->edges);
  std::vector<int32_t> order(keys.size());
  for (size_t k = 0; k < keys.size(); k++) order[k] = (int32_t)k;
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return keys[(size_t)a].key < keys[(size_t)b].key; });
  lc_wr_lin_summary ls{};
  for (size_t i = 0; i < order.size(); i++) {
    const Key &k = keys[(size_t)order[i]];
    out->keys[i] = lc_wr_key{k.key, (k.flags & LC_WR_K_CYCLIC) ? k.cyc_value : LC_WR_NIL, k.flags, k.n_writes,
                             k.n_versions, k.n_ext_reads};
    lin_keys[i] = lc_wr_lin_key{k.n_pairs, (int32_t)k.touches.size(), (int32_t)((int64_t)k.vedges.size() + k.n_init)};
    ls.n_touches += lin_keys[i].n_touches;
    ls.n_pairs += lin_keys[i].n_pairs;
    ls.n_vedges += lin_keys[i].n_vedges;
  }
  ls.max_key_versions = max_versions;
  lcgraph::real_time_host(txns, n_txns, out->byc, out->rt_lo, out->rt_hi);
  lc_wr_summary s;
  graph_and_summary(txns, n_txns, p, out, (int64_t)keys.size(), n_edges, counts, &s);
  s.n_edges_raw = n_raw;
  s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = s;
  if (lin_sum) *lin_sum = ls;
  return 0;
}

}  // namespace

extern "C" int lc_wr_check_lin_host(const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops,
                                    uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum, lc_wr_lin_key *lin_keys,
                                    lc_wr_lin_summary *lin_sum) {
  try {
    return wr_lin_host(txns, n_txns, mops, n_mops, flags, out, sum, lin_keys, lin_sum);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}
