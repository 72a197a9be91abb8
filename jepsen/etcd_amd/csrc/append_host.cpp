// append_host.cpp — lc_append_check_host: the rules of
// include/lincheck_append.h on the host, single-threaded, with hash maps and
// an iterative Tarjan; and the host parts of lc_append_check: the contract,
// the slow path for reads the device could not decide and the summary.  Rule
// 6's host form and rule 7 (SCCs, classes, witness cycles) are
// graph_host.cpp's, shared with lc_wr_check.  g++, no GPU.
#include <errno.h>
#include <stdlib.h>

#include <algorithm>
#include <chrono>
#include <new>
#include <unordered_map>
#include <unordered_set>

#include "append.h"

namespace lcap {

struct Writers::Impl {
  std::unordered_map<std::pair<int64_t, int64_t>, int32_t, PairHash> map;
};

Writers::~Writers() { delete impl; }

int Writers::build(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops) {
  impl = new Impl;
  last.assign((size_t)n_mops, 0);
  std::unordered_set<int64_t> seen;
  for (int64_t t = 0; t < n_txns; t++) {
    seen.clear();
    const int64_t b = txns[t].mop_off, e = b + txns[t].mop_len;
    for (int64_t m = e - 1; m >= b; m--)
      if (mops[m].f == LC_AP_APPEND && seen.insert(mops[m].key).second) last[m] = 1;
    for (int64_t m = b; m < e; m++)
      if (mops[m].f == LC_AP_APPEND && !impl->map.emplace(std::make_pair(mops[m].key, mops[m].value), (int32_t)m).second)
        return -EINVAL;
  }
  return 0;
}

int32_t Writers::find(int64_t key, int64_t element) const {
  const auto it = impl->map.find(std::make_pair(key, element));
  return it == impl->map.end() ? -1 : it->second;
}

int prepare(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops, const int64_t *values,
            int64_t n_values, const lc_ap_out *out, Prep *p, const char **err) {
#define LCAP_BAD(text) \
  do {                 \
    *err = text;       \
    return -EINVAL;    \
  } while (0)
  if (n_txns < 0 || n_mops < 0 || n_values < 0 || (n_txns > 0 && !txns) || (n_mops > 0 && !mops) ||
      (n_values > 0 && !values))
    LCAP_BAD("null array or negative count");
  if (n_mops >= kMaxMops || n_txns >= kMaxMops) LCAP_BAD("2^31 - 1 or more txns or mops");
  if (null_out(out)) LCAP_BAD("null out");
  p->mop_txn.resize((size_t)n_mops);
  p->txn_r0.resize((size_t)n_txns + 1);
  p->work_off.assign(1, 0);
  int64_t next = 0, prev_inv = -1;
  for (int64_t t = 0; t < n_txns; t++) {
    const lc_ap_txn &x = txns[t];
    if (const char *bad = check_txn(x, prev_inv, next, n_mops)) LCAP_BAD(bad);
    prev_inv = x.inv_pos;
    p->txn_r0[(size_t)t] = (int32_t)p->rd_mop.size();
    for (int64_t m = next; m < next + x.mop_len; m++) {
      const lc_ap_mop &o = mops[m];
      p->mop_txn[(size_t)m] = (int32_t)t;
      if (o.key == kReserved) LCAP_BAD("a key is INT64_MIN");
      if (o.f == LC_AP_APPEND) {
        if (o.value == kReserved) LCAP_BAD("an appended element is INT64_MIN");
        p->n_appends++;
      } else if (o.f == LC_AP_READ) {
        p->n_reads++;
        if (x.type == LC_AP_OK) {
          if (o.len < 0 || o.value < 0 || o.value > n_values - o.len) LCAP_BAD("a read's payload leaves values");
          p->rd_mop.push_back((int32_t)m);
          p->work_off.push_back(p->work_off.back() + o.len);
          if (p->work_off.back() >= kMaxMops) LCAP_BAD("the reads' total length is 2^31 - 1 or more");
        } else if (o.len != -1) {
          LCAP_BAD("a read of an INFO or FAIL txn with a len other than -1");
        }
      } else {
        LCAP_BAD("unknown mop f");
      }
    }
    next += x.mop_len;
    if (x.type == LC_AP_OK) p->n_ok++;
    if (x.type != LC_AP_FAIL) p->n_nodes++;
  }
  if (next != n_mops) LCAP_BAD("the txns' mop ranges do not tile the mops in order");
  p->txn_r0[(size_t)n_txns] = (int32_t)p->rd_mop.size();
  return 0;
#undef LCAP_BAD
}

int32_t first_dup_direct(const int64_t *order, int32_t len) {
  std::unordered_set<int64_t> seen;
  for (int32_t i = 0; i < len; i++)
    if (!seen.insert(order[i]).second) return i;
  return -1;
}

int64_t rules34_direct(const lc_ap_txn *txns, const lc_ap_mop *mops, const int64_t *values, const Prep &p,
                       const Writers &w, int64_t t, int32_t *mop_flags, int32_t *txn_flags) {
  struct State {
    int64_t read = -1;             // the latest read of the key in this txn
    std::vector<int64_t> appends;  // own appends since (or since the txn began)
  };
  std::unordered_map<int64_t, State> state;
  std::unordered_set<int64_t> seen;
  int64_t n = 0;
  int32_t tf = 0;
  const int64_t b = txns[t].mop_off, e = b + txns[t].mop_len;
  for (int64_t m = b; m < e; m++) {
    const lc_ap_mop &o = mops[m];
    State &s = state[o.key];
    if (o.f == LC_AP_APPEND) {
      s.appends.push_back(o.value);
      continue;
    }
    if (o.len < 0) continue;
    n++;
    int32_t f = mop_flags[m] & LC_AP_R_NONPREFIX;
    const int64_t *pl = values + o.value;
    seen.clear();
    for (int32_t i = 0; i < o.len; i++) {
      if (!seen.insert(pl[i]).second) f |= LC_AP_R_DUPLICATE;
      const int32_t wm = w.find(o.key, pl[i]);
      if (wm < 0) f |= LC_AP_R_PHANTOM;
      else if (txns[p.mop_txn[(size_t)wm]].type == LC_AP_FAIL) f |= LC_AP_R_G1A;
    }
    if (o.len > 0) {
      const int32_t wm = w.find(o.key, pl[o.len - 1]);
      if (wm >= 0 && p.mop_txn[(size_t)wm] != t && !w.last[(size_t)wm]) f |= LC_AP_R_G1B;
    }
    const int64_t a = (int64_t)s.appends.size();
    bool ok = true;
    if (s.read >= 0) {
      const lc_ap_mop &q = mops[s.read];
      ok = o.len == q.len + a && std::equal(pl, pl + q.len, values + q.value) &&
           std::equal(s.appends.begin(), s.appends.end(), pl + q.len);
    } else if (a > 0) {
      ok = o.len >= a && std::equal(s.appends.begin(), s.appends.end(), pl + (o.len - a));
    } else {
      f |= LC_AP_R_EXTERNAL;
    }
    if (!ok) f |= LC_AP_R_INTERNAL;
    s.read = m;
    s.appends.clear();
    mop_flags[m] = f;
    tf |= f & LC_AP_R_ANOMALY;
  }
  txn_flags[t] = tf;
  return n;
}

int graph_and_summary(const lc_ap_txn *txns, int64_t n_txns, const Prep &p, const lc_ap_out *out, int64_t n_keys,
                      int64_t n_edges, int64_t n_nonprefix, const int64_t *counts, lc_ap_summary *sum, bool no_scc,
                      lcgraph::MarkedPass *mp) {
  const auto t0 = std::chrono::steady_clock::now();
  lc_ap_summary s{};
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
  for (int64_t k = 0; k < n_keys; k++)
    if (out->keys[k].flags & LC_AP_K_INCOMPATIBLE) s.n_incompatible_order++;
  s.n_nonprefix = n_nonprefix;
  s.n_duplicate = counts[0];
  s.n_g1a = counts[1];
  s.n_phantom = counts[2];
  s.n_g1b = counts[3];
  s.n_internal = counts[4];
  s.n_keys = n_keys;
  s.n_ok = p.n_ok;
  s.n_nodes = p.n_nodes;
  s.n_edges = n_edges;
  s.n_scc = cc.n_scc;
  s.n_cycles_returned = cc.n_cycles_returned;
  const bool bad = s.n_incompatible_order || s.n_nonprefix || s.n_duplicate || s.n_g1a || s.n_phantom || s.n_g1b ||
                   s.n_internal || s.n_scc;
  s.valid = p.n_ok == 0 ? -1 : bad ? 0 : 1;
  s.host_graph_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = s;
  return 0;
}

}  // namespace lcap

extern "C" int lc_append_limits(lc_ap_limit_info *out) {
  if (!out) return -EINVAL;
  out->default_max_payload = lcap::kDefaultMaxPayload;
  out->max_payload = lcap::kDefaultMaxPayload;
  if (const char *e = getenv("LC_AP_MAX_PAYLOAD")) {
    const long long v = atoll(e);
    if (v > 0) out->max_payload = v;
  }
  out->max_position = lcap::kMaxPosition;
  out->max_mops = lcap::kMaxDeviceMops;
  if (const char *e = getenv("LC_AP_MAX_MOPS")) {
    const long long v = atoll(e);
    if (v > 0 && v < lcap::kMaxDeviceMops) out->max_mops = v;
  }
  return 0;
}

namespace {

int append_host(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops, const int64_t *values,
                int64_t n_values, const lc_ap_out *out, lc_ap_summary *sum) {
  using namespace lcap;
  const auto t0 = std::chrono::steady_clock::now();
  Prep p;
  const char *why = nullptr;
  if (int rc = prepare(txns, n_txns, mops, n_mops, values, n_values, out, &p, &why)) return rc;
  Writers w;
  if (int rc = w.build(txns, n_txns, mops, n_mops)) return rc;
  const int64_t n_real = (int64_t)p.rd_mop.size();
  // rule 2: the keys and their longest reads
  struct Key {
    int64_t key;
    int32_t longest = -1, len = 0;  // a real read's ordinal
  };
  std::unordered_map<int64_t, int32_t> key_id;
  std::vector<Key> keys;
  std::vector<int32_t> mop_key((size_t)n_mops);
  for (int64_t m = 0; m < n_mops; m++) {
    const auto it = key_id.emplace(mops[m].key, (int32_t)keys.size());
    if (it.second) keys.push_back(Key{mops[m].key});
    mop_key[(size_t)m] = it.first->second;
  }
  for (int64_t r = 0; r < n_real; r++) {
    Key &k = keys[(size_t)mop_key[(size_t)p.rd_mop[(size_t)r]]];
    const int32_t len = mops[p.rd_mop[(size_t)r]].len;
    if (k.longest < 0 || len > k.len) {
      k.longest = (int32_t)r;
      k.len = len;
    }
  }
  std::vector<int32_t> order((size_t)keys.size());
  for (size_t k = 0; k < keys.size(); k++) order[k] = (int32_t)k;
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return keys[(size_t)a].key < keys[(size_t)b].key; });
  std::vector<int32_t> rank((size_t)keys.size());
  for (size_t i = 0; i < order.size(); i++) rank[(size_t)order[i]] = (int32_t)i;
  // the orders' writers and first_*
  std::vector<std::vector<int32_t>> ord_w(keys.size());
  for (size_t i = 0; i < order.size(); i++) {
    const Key &k = keys[(size_t)order[i]];
    lc_ap_key &o = out->keys[i];
    o = lc_ap_key{k.key, -1, 0, 0, -1, -1, -1, 0};
    if (k.longest < 0) continue;
    const lc_ap_mop &rd = mops[p.rd_mop[(size_t)k.longest]];
    o.longest = p.rd_mop[(size_t)k.longest];
    o.len = rd.len;
    o.first_dup = first_dup_direct(values + rd.value, rd.len);
    std::vector<int32_t> &wr = ord_w[(size_t)order[i]];
    wr.resize((size_t)rd.len);
    for (int32_t j = 0; j < rd.len; j++) {
      const int32_t wm = w.find(k.key, values[rd.value + j]);
      wr[(size_t)j] = wm;
      if (wm < 0 && o.first_phantom < 0) o.first_phantom = j;
      if (wm >= 0 && txns[p.mop_txn[(size_t)wm]].type == LC_AP_FAIL && o.first_failed < 0) o.first_failed = j;
    }
  }
  // prefix reads
  for (int64_t m = 0; m < n_mops; m++) out->mop_flags[m] = 0;
  int64_t n_nonprefix = 0;
  for (int64_t r = 0; r < n_real; r++) {
    const int32_t m = p.rd_mop[(size_t)r];
    const int32_t kid = mop_key[(size_t)m];
    const lc_ap_mop &lg = mops[p.rd_mop[(size_t)keys[(size_t)kid].longest]];
    if (!std::equal(values + mops[m].value, values + mops[m].value + mops[m].len, values + lg.value)) {
      out->mop_flags[m] = LC_AP_R_NONPREFIX;
      out->keys[rank[(size_t)kid]].flags |= LC_AP_K_INCOMPATIBLE;
      n_nonprefix++;
    }
  }
  for (size_t i = 0; i < order.size(); i++) {
    lc_ap_key &o = out->keys[i];
    if ((o.flags & LC_AP_K_INCOMPATIBLE) || o.first_dup >= 0 || o.first_phantom >= 0) o.flags |= LC_AP_K_NO_ORDER;
  }
  // rules 3 and 4
  int64_t counts[kCounters] = {0};
  for (int64_t t = 0; t < n_txns; t++) {
    out->txn_flags[t] = 0;
    if (txns[t].type != LC_AP_OK) continue;
    rules34_direct(txns, mops, values, p, w, t, out->mop_flags, out->txn_flags);
    for (int64_t m = txns[t].mop_off; m < txns[t].mop_off + txns[t].mop_len; m++)
      for (int b = 0; b < 5; b++) counts[b] += (out->mop_flags[m] >> (b + 1)) & 1;
  }
  // rule 5
  auto node_of = [&](int32_t wm) {
    const int32_t t = p.mop_txn[(size_t)wm];
    return txns[t].type == LC_AP_FAIL ? -1 : t;
  };
  int64_t n_edges = 0;
  auto emit = [&](int32_t from, int32_t to, int32_t type, int64_t key) {
    if (from >= 0 && to >= 0 && from != to) out->edges[n_edges++] = lc_ap_edge{from, to, type, 0, key};
  };
  for (size_t i = 0; i < order.size(); i++) {
    if (out->keys[i].flags & LC_AP_K_NO_ORDER) continue;
    const std::vector<int32_t> &wr = ord_w[(size_t)order[i]];
    for (size_t j = 0; j + 1 < wr.size(); j++) emit(node_of(wr[j]), node_of(wr[j + 1]), LC_AP_WW, out->keys[i].key);
  }
  for (int64_t r = 0; r < n_real; r++) {
    const int32_t m = p.rd_mop[(size_t)r];
    const int32_t kid = mop_key[(size_t)m];
    if ((out->keys[rank[(size_t)kid]].flags & LC_AP_K_NO_ORDER) || !(out->mop_flags[m] & LC_AP_R_EXTERNAL)) continue;
    const std::vector<int32_t> &wr = ord_w[(size_t)kid];
    const int32_t len = mops[m].len, t = p.mop_txn[(size_t)m];
    if (len > 0) emit(node_of(wr[(size_t)len - 1]), t, LC_AP_WR, mops[m].key);
    if ((size_t)len < wr.size()) emit(t, node_of(wr[(size_t)len]), LC_AP_RW, mops[m].key);
  }
  std::sort(out->edges, out->edges + n_edges, edge_less);
  n_edges = std::unique(out->edges, out->edges + n_edges, edge_same) - out->edges;
  real_time_host(txns, n_txns, out->byc, out->rt_lo, out->rt_hi);
  lc_ap_summary s;
  graph_and_summary(txns, n_txns, p, out, (int64_t)keys.size(), n_edges, n_nonprefix, counts, &s);
  s.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = s;
  return 0;
}

}  // namespace

extern "C" int lc_append_check_host(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops,
                                    const int64_t *values, int64_t n_values, const lc_ap_out *out,
                                    lc_ap_summary *sum) {
  try {
    return append_host(txns, n_txns, mops, n_mops, values, n_values, out, sum);
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
}
