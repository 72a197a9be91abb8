// wr_lin_main.cpp — lc_wr_check_lin_host (csrc/wr_lin_host.cpp with
// csrc/wr_host.cpp and csrc/graph_host.cpp) as a stand-alone program for
// tests/test_wr_lin_host_sanitize.py, which builds it with the address and
// undefined-behaviour sanitizers.  It reads the cases the test wrote (argv[1]:
// n_cases, then per case n_txns, n_mops, flags, the txns, the mops) and
// generates some of its own: random txns whose reads name random values, so
// that stale reads, cycles through nil, phantoms at edges' heads and large
// successor runs occur.  One line per call: the code and the counts of both
// summaries, judged by the test.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../include/lincheck_wrlin.h"

namespace {

// An array of exactly n entries on the heap, n == 0 included: a write past
// any of them is the sanitizer's to find.
template <class T>
struct Exact {
  T *p;
  explicit Exact(size_t n) : p(new T[n]()) {}
  ~Exact() { delete[] p; }
  Exact(const Exact &) = delete;
  T &operator[](size_t i) { return p[i]; }
};

struct Arrays {
  Exact<int32_t> mop_flags, txn_flags, byc, lo, hi, scc, cls, cycle_scc;
  Exact<lc_wr_key> keys;
  Exact<lc_wr_lin_key> lin_keys;
  Exact<lc_wr_edge> edges;
  Exact<lc_wr_step> steps;
  Exact<int64_t> cycle_off;
  lc_wr_out out;
  Arrays(size_t nt, size_t nm, int64_t edge_cap)
      : mop_flags(nm), txn_flags(nt), byc(nt), lo(nt), hi(nt), scc(nt), cls(nt), cycle_scc(LC_AP_MAX_CYCLES),
        keys(nm), lin_keys(nm), edges((size_t)edge_cap), steps(nt), cycle_off(LC_AP_MAX_CYCLES + 1) {
    out = lc_wr_out{mop_flags.p, txn_flags.p, keys.p, edges.p, edge_cap, byc.p, lo.p, hi.p, scc.p, cls.p, steps.p,
                    cycle_off.p, cycle_scc.p};
  }
};

int run(const char *name, int idx, const std::vector<lc_wr_txn> &txns, const std::vector<lc_wr_mop> &mops,
        uint32_t flags) {
  // first with no room for edges at all, then with exactly the room asked for
  const int64_t nt = (int64_t)txns.size(), nm = (int64_t)mops.size();
  Arrays none(txns.size(), mops.size(), 0);
  lc_wr_summary s{};
  lc_wr_lin_summary ls{};
  int rc = lc_wr_check_lin_host(txns.data(), nt, mops.data(), nm, flags, &none.out, &s, none.lin_keys.p, &ls);
  if (rc == -ENOSPC) {
    const int64_t want = s.n_edges;
    Arrays a(txns.size(), mops.size(), want);
    rc = lc_wr_check_lin_host(txns.data(), nt, mops.data(), nm, flags, &a.out, &s, a.lin_keys.p, &ls);
    if (rc == 0 && s.n_edges != want) rc = -1000;
    int64_t sum = 0, pairs = 0;  // every output read once
    for (int64_t i = 0; i < s.n_edges; i++) sum += a.edges[(size_t)i].from + a.edges[(size_t)i].to;
    for (int64_t i = 0; i < s.n_keys; i++) {
      sum += a.keys[(size_t)i].n_versions + a.lin_keys[(size_t)i].n_vedges;
      pairs += a.lin_keys[(size_t)i].n_pairs;
    }
    for (int64_t i = 0; i < a.cycle_off[(size_t)s.n_cycles_returned]; i++) sum += a.steps[(size_t)i].txn;
    if (sum < 0) rc = -1001;
    if (rc == 0 && pairs != ls.n_pairs) rc = -1002;
  }
  printf("%s %d rc %d valid %d cyclic %lld phantom %lld keys %lld edges %lld raw %lld scc %lld touches %lld pairs %lld "
         "vedges %lld maxv %lld\n",
         name, idx, rc, rc ? 9 : s.valid, (long long)s.n_cyclic_keys, (long long)s.n_phantom, (long long)s.n_keys,
         (long long)s.n_edges, (long long)s.n_edges_raw, (long long)s.n_scc, (long long)ls.n_touches,
         (long long)ls.n_pairs, (long long)ls.n_vedges, (long long)ls.max_key_versions);
  return rc;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % n;
}

// n_txns txns of up to 4 mops over n_keys keys, each lasting up to `span`
// positions; a read names nil or any value of the key, written already or
// later, or (rarely) nobody's.
void generate(int n_txns, int n_keys, int span, std::vector<lc_wr_txn> *txns, std::vector<lc_wr_mop> *mops) {
  txns->clear();
  mops->clear();
  std::vector<int64_t> next((size_t)n_keys, 1);
  const int per_key = 4 * n_txns / n_keys + 1;
  int32_t pos = 0;
  for (int t = 0; t < n_txns; t++) {
    const uint32_t r = rnd(100);
    const int32_t type = r < 6 ? LC_WR_INFO : r < 12 ? LC_WR_FAIL : LC_WR_OK;
    lc_wr_txn x{(int64_t)mops->size(), pos, type == LC_WR_INFO ? -1 : pos + 1 + (int32_t)rnd((uint32_t)span), type,
                (int32_t)rnd(5)};
    pos += 2;
    for (int i = 0; i < x.mop_len; i++) {
      const int64_t k = rnd((uint32_t)n_keys);
      if (rnd(2)) {
        mops->push_back(lc_wr_mop{k, next[(size_t)k]++, LC_WR_WRITE, 0});
      } else if (type != LC_WR_OK) {
        mops->push_back(lc_wr_mop{k, 0, LC_WR_READ, 0});
      } else {
        const uint32_t c = rnd(10);
        const int64_t v = c == 0 ? LC_WR_NIL : c == 1 ? 1000000 + t : 1 + (int64_t)rnd((uint32_t)per_key);
        mops->push_back(lc_wr_mop{k, v, LC_WR_READ, 1});
      }
    }
    txns->push_back(x);
  }
  // a comp_pos is odd (every inv_pos is even) and nobody else's
  std::vector<uint8_t> used((size_t)pos + (size_t)span + 64 + 2 * txns->size(), 0);
  for (lc_wr_txn &x : *txns) {
    if (x.type == LC_WR_INFO) continue;
    int32_t c = x.comp_pos | 1;
    while (used[(size_t)c]) c += 2;
    used[(size_t)c] = 1;
    x.comp_pos = c;
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, f) != 1) return 2;
  std::vector<lc_wr_txn> txns;
  std::vector<lc_wr_mop> mops;
  for (int64_t c = 0; c < n_cases; c++) {
    int64_t hdr[3];
    if (fread(hdr, 8, 3, f) != 3) return 2;
    txns.resize((size_t)hdr[0]);
    mops.resize((size_t)hdr[1]);
    if (hdr[0] && fread(txns.data(), sizeof(lc_wr_txn), txns.size(), f) != txns.size()) return 2;
    if (hdr[1] && fread(mops.data(), sizeof(lc_wr_mop), mops.size(), f) != mops.size()) return 2;
    if (run("case", (int)c, txns, mops, (uint32_t)hdr[2])) return 1;
  }
  fclose(f);
  // (txns, keys, span): none, one, short and long successor runs, many keys, the largest
  static const int kShapes[][3] = {{0, 1, 12}, {1, 1, 12}, {7, 1, 12}, {40, 2, 12}, {200, 3, 6}, {200, 3, 120},
                                   {200, 40, 12}, {1500, 5, 40}};
  int idx = 0;
  for (const auto &sh : kShapes)
    for (uint32_t flags = 0; flags < 4; flags++) {
      generate(sh[0], sh[1], sh[2], &txns, &mops);
      if (run("gen", idx++, txns, mops, flags)) return 1;
    }
  // the contract's refusals: nothing may be written, nothing read out of bounds
  generate(40, 2, 12, &txns, &mops);
  std::vector<lc_wr_mop> twice = mops;
  for (size_t i = 0, first = twice.size(); i < twice.size(); i++)
    if (twice[i].f == LC_WR_WRITE) {
      if (first == twice.size()) first = i;
      else if (twice[i].key == twice[first].key) twice[i].value = twice[first].value;
    }
  if (run("twice", 0, txns, twice, 3) != -EINVAL) return 1;
  std::vector<lc_wr_txn> bad = txns;
  bad[3].mop_len += 1;
  if (run("tiling", 0, bad, mops, 3) != -EINVAL) return 1;
  if (run("flags", 0, txns, mops, 4) != -EINVAL) return 1;
  Arrays a(txns.size(), mops.size(), 0);
  if (lc_wr_check_lin_host(txns.data(), (int64_t)txns.size(), mops.data(), (int64_t)mops.size(), 3, &a.out, nullptr,
                           nullptr, nullptr) != -EINVAL)
    return 1;
  return 0;
}
