// wr_host.cpp — lc_wr_check_host: the rules of include/lincheck_wr.h on the
// host, single-threaded, with hash maps; and the host parts of lc_wr_check:
// the contract, rule 9 (graph_host.cpp's code, which lc_append_check runs
// too) and the summary.  g++, no GPU.
#include <errno.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <unordered_map>

#include "wr.h"

namespace lcwr {

int prepare(const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops, uint32_t flags,
            const lc_wr_out *out, Prep *p, const char **err) {
#define LCWR_BAD(text) \
  do {                 \
    *err = text;       \
    return -EINVAL;    \
  } while (0)
  if (n_txns < 0 || n_mops < 0 || (n_txns > 0 && !txns) || (n_mops > 0 && !mops))
    LCWR_BAD("null array or negative count");
  if (flags & ~LC_WR_WFR_KEYS) LCWR_BAD("unknown flag");
  if (n_mops >= kMaxMops || n_txns >= kMaxMops) LCWR_BAD("2^31 - 1 or more txns or mops");
  if (null_out(out)) LCWR_BAD("null out");
  if (out->edge_cap < 0) LCWR_BAD("negative edge_cap");
  p->mop_txn.resize((size_t)n_mops);
  int64_t next = 0, prev_inv = -1;
  for (int64_t t = 0; t < n_txns; t++) {
    const lc_wr_txn &x = txns[t];
    if (const char *bad = check_txn(x, prev_inv, next, n_mops)) LCWR_BAD(bad);
    prev_inv = x.inv_pos;
    for (int64_t m = next; m < next + x.mop_len; m++) {
      const lc_wr_mop &o = mops[m];
      p->mop_txn[(size_t)m] = (int32_t)t;
      if (o.key == kReserved) LCWR_BAD("a key is INT64_MIN");
      if (o.f == LC_WR_WRITE) {
        if (o.value == kReserved) LCWR_BAD("a written value is LC_WR_NIL");
        if (o.known != 0) LCWR_BAD("a write with known set");
      } else if (o.f == LC_WR_READ) {
        if (o.known != (x.type == LC_WR_OK ? 1 : 0))
          LCWR_BAD("known is not 1 on an OK txn's read and 0 on another txn's");
      } else {
        LCWR_BAD("unknown mop f");
      }
    }
    next += x.mop_len;
    if (x.type == LC_WR_OK) p->n_ok++;
    if (x.type != LC_WR_FAIL) p->n_nodes++;
  }
  if (next != n_mops) LCWR_BAD("the txns' mop ranges do not tile the mops in order");
  return 0;
#undef LCWR_BAD
}

int graph_and_summary(const lc_wr_txn *txns, int64_t n_txns, const Prep &p, const lc_wr_out *out, int64_t n_keys,
                      int64_t n_edges, const int64_t *counts, lc_wr_summary *sum, bool no_scc,
                      lcgraph::MarkedPass *mp) {
  const auto t0 = std::chrono::steady_clock::now();
  lc_wr_summary s{};
  lcgraph::CycleCounts cc;
  if (no_scc)
    lcgraph::no_cycles(n_txns, out->scc, out->scc_class, out->cycle_off, out->cycle_scc, &cc);
  else if (mp) {
    if (int e = lcgraph::cycles_host_marked(txns, n_txns, out->edges, n_edges, out->byc, p.n_ok, out->rt_lo, out->rt_hi,
                                            mp, out->scc, out->scc_class, out->steps, out->cycle_off, out->cycle_scc,
                                            &cc))
      return e;
  } else
    lcgraph::cycles_host(txns, n_txns, p.n_nodes, out->edges, n_edges, out->byc, out->rt_lo, out->rt_hi, out->scc,
                         out->scc_class, out->steps, out->cycle_off, out->cycle_scc, &cc);
  std::copy(cc.n_class, cc.n_class + 8, s.n_class);
  bool lost = false;
  for (int64_t k = 0; k < n_keys; k++) {
    if (out->keys[k].flags & LC_WR_K_CYCLIC) s.n_cyclic_keys++;
    if (out->keys[k].flags & LC_WR_K_LOST_UPDATE) lost = true;
    s.n_versions += out->keys[k].n_versions;
  }
  s.n_internal = counts[0];
  s.n_phantom = counts[1];
  s.n_g1a = counts[2];
  s.n_g1b = counts[3];
  s.n_lost_update = counts[4];
  s.n_keys = n_keys;
  s.n_ok = p.n_ok;
  s.n_nodes = p.n_nodes;
  s.n_edges = n_edges;
  s.n_scc = cc.n_scc;
  s.n_cycles_returned = cc.n_cycles_returned;
  const bool bad = s.n_internal || s.n_phantom || s.n_g1a || s.n_g1b || s.n_cyclic_keys || lost || s.n_scc;
  s.valid = p.n_ok == 0 ? -1 : bad ? 0 : 1;
  s.host_graph_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = s;
  return 0;
}

}  // namespace lcwr

extern "C" int lc_wr_limits(lc_wr_limit_info *out) {
  if (!out) return -EINVAL;
  out->default_max_edges = lcwr::kDefaultMaxEdges;
  out->max_edges = lcwr::kDefaultMaxEdges;
  if (const char *e = getenv("LC_WR_MAX_EDGES")) {
    const long long v = atoll(e);
    if (v > 0) out->max_edges = v;
  }
  out->max_position = lcwr::kMaxPosition;
  out->max_mops = lcwr::kMaxDeviceMops;
  if (const char *e = getenv("LC_WR_MAX_MOPS")) {
    const long long v = atoll(e);
    if (v > 0 && v < lcwr::kMaxDeviceMops) out->max_mops = v;
  }
  return 0;
}

namespace {

// A version of rule 4.  Its wfr parent is one version at most: its value has
// one writer, whose txn has one external read of the key.
struct Version {
  int64_t key, value;
  int32_t kid;
  int32_t writer = -1;   // the write mop
  int32_t parent = -1;   // a version; itself: a self-loop
  int32_t n_rw = 0;      // external readers whose txn writes the key (rule 5)
  int32_t state = 0;     // rule 6's walk: 0 new, else the walk that met it; -1 done
  std::vector<int32_t> readers;   // the txns with an external read of it
  std::vector<int32_t> children;  // the write mops at the heads of its version edges
};

struct Key {
  int64_t key;
  int64_t cyc_value = LC_WR_NIL;
  int32_t flags = 0, n_writes = 0, n_versions = 1, n_ext_reads = 0;
  int32_t nil = -1;  // the version (key, nil), once somebody read it
};

int wr_host(const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops, uint32_t flags,
            const lc_wr_out *out, lc_wr_summary *sum) {
  using namespace lcwr;
  const auto t0 = std::chrono::steady_clock::now();
  Prep p;
  const char *why = nullptr;
  if (int rc = prepare(txns, n_txns, mops, n_mops, flags, out, &p, &why)) return rc;
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
      vers.emplace_back();
      vers.back().key = o.key;
      vers.back().value = o.value;
      vers.back().kid = kid;
      if (o.value == LC_WR_NIL) keys[(size_t)kid].nil = vit.first->second;
      else keys[(size_t)kid].n_versions++;
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
  // rules 2, 3 and 5, and rule 4's wfr edges as parents
  std::vector<int32_t> mop_flags((size_t)n_mops, 0), txn_flags((size_t)n_txns, 0);
  std::vector<int32_t> mop_par((size_t)n_mops, -1);  // on an external write: the version its txn read
  int64_t counts[kCounters] = {0};
  for (int64_t t = 0; t < n_txns; t++) {
    const lc_wr_txn &x = txns[t];
    if (x.type != LC_WR_OK) continue;
    int32_t tf = 0;
    for (int64_t m = x.mop_off; m < x.mop_off + x.mop_len; m++) {
      const lc_wr_mop &o = mops[m];
      if (o.f != LC_WR_READ) continue;
      int64_t prev = -1;
      for (int64_t j = m - 1; j >= x.mop_off && prev < 0; j--)
        if (mops[j].key == o.key) prev = j;
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
      int64_t mb = -1;  // the txn's external write of the key
      for (int64_t j = m + 1; j < x.mop_off + x.mop_len; j++)
        if (mops[j].f == LC_WR_WRITE && mops[j].key == o.key) mb = j;
      if (mb < 0) continue;
      if (++a.n_rw == 2) {
        counts[4]++;
        keys[(size_t)a.kid].flags |= LC_WR_K_LOST_UPDATE;
      }
      if (wfr) {
        mop_par[(size_t)mb] = mop_ver[(size_t)m];
        if (o.value != LC_WR_NIL) vers[(size_t)mop_ver[(size_t)mb]].parent = mop_ver[(size_t)m];
      }
    }
    txn_flags[(size_t)t] = tf;
  }
  // rule 6: walk the parents; a walk that meets itself has found a cycle
  for (size_t v0 = 0; v0 < vers.size(); v0++) {
    if (vers[v0].state) continue;
    const int32_t walk = (int32_t)v0 + 1;
    int32_t v = (int32_t)v0;
    while (v >= 0 && vers[(size_t)v].state == 0) {
      vers[(size_t)v].state = walk;
      v = vers[(size_t)v].parent;
    }
    if (v >= 0 && vers[(size_t)v].state == walk) {  // v lies on a new cycle
      Key &k = keys[(size_t)vers[(size_t)v].kid];
      int32_t u = v;
      do {
        if (!(k.flags & LC_WR_K_CYCLIC) || vers[(size_t)u].value < k.cyc_value) k.cyc_value = vers[(size_t)u].value;
        k.flags |= LC_WR_K_CYCLIC;
        u = vers[(size_t)u].parent;
      } while (u != v);
    }
    for (v = (int32_t)v0; v >= 0 && vers[(size_t)v].state == walk; v = vers[(size_t)v].parent)
      vers[(size_t)v].state = -1;
  }
  // rule 4's edges as children lists: nil -> b once, whichever way it arises
  auto is_node = [&](int32_t t) { return txns[t].type != LC_WR_FAIL; };
  for (int64_t m = 0; m < n_mops; m++) {
    if (mops[m].f != LC_WR_WRITE) continue;
    const Key &k = keys[(size_t)mop_key[(size_t)m]];
    if (is_node(p.mop_txn[(size_t)m]) && k.nil >= 0) vers[(size_t)k.nil].children.push_back((int32_t)m);
    const int32_t a = mop_par[(size_t)m];
    if (a >= 0 && a != mop_ver[(size_t)m] && vers[(size_t)a].value != LC_WR_NIL)
      vers[(size_t)a].children.push_back((int32_t)m);
  }
  // rule 7
  std::vector<lc_wr_edge> edges;
  auto emit = [&](int32_t from, int32_t to, int32_t type, int64_t key) {
    if (is_node(from) && is_node(to) && from != to) edges.push_back(lc_wr_edge{from, to, type, 0, key});
  };
  for (const Version &a : vers) {
    if (a.writer >= 0)
      for (int32_t t : a.readers) emit(p.mop_txn[(size_t)a.writer], t, LC_AP_WR, a.key);
    if (keys[(size_t)a.kid].flags & LC_WR_K_CYCLIC) continue;
    for (int32_t mb : a.children) {
      const int32_t w = p.mop_txn[(size_t)mb];
      if (a.writer >= 0) emit(p.mop_txn[(size_t)a.writer], w, LC_AP_WW, a.key);
      for (int32_t t : a.readers) emit(t, w, LC_AP_RW, a.key);
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
  for (size_t i = 0; i < order.size(); i++) {
    const Key &k = keys[(size_t)order[i]];
    out->keys[i] = lc_wr_key{k.key, (k.flags & LC_WR_K_CYCLIC) ? k.cyc_value : LC_WR_NIL, k.flags, k.n_writes,
                             k.n_versions, k.n_ext_reads};
  }
  lcgraph::real_time_host(txns, n_txns, out->byc, out->rt_lo, out->rt_hi);
  lc_wr_summary s;
  graph_and_summary(txns, n_txns, p, out, (int64_t)keys.size(), n_edges, counts, &s);
  s.n_edges_raw = n_raw;
  s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = s;
  return 0;
}

}  // namespace

extern "C" int lc_wr_check_host(const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops,
                                uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum) {
  try {
    return wr_host(txns, n_txns, mops, n_mops, flags, out, sum);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}
