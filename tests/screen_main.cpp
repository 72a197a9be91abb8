// screen_main.cpp — lc_cycle_screen_host (csrc/screen_host.cpp) as a
// stand-alone program for tests/test_screen_host_sanitize.py, which builds it
// with the address and undefined-behaviour sanitizers.  It reads the cases the
// test wrote (argv[1]: n_cases, then per case n_txns, n_edges, the txns, the
// edges) and generates graphs of its own of up to 1,500 txns: random
// lifetimes, edges with and against txn order.  Every output array is sized
// exactly.  One line per call: the code and the summary's counts, judged by
// the test.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "../include/lincheck_screen.h"

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

int run(const char *name, int idx, const std::vector<lc_ap_txn> &txns, const std::vector<lc_ap_edge> &edges) {
  const size_t nt = txns.size();
  Exact<int32_t> lo(nt), hi(nt), mark(nt);
  const lc_screen_out out{lo.p, hi.p, mark.p};
  lc_screen_summary s{};
  const int rc = lc_cycle_screen_host(txns.data(), (int64_t)nt, edges.data(), (int64_t)edges.size(), &out, &s);
  long long sum_lo = 0, sum_hi = 0, marks = 0;  // every output read once
  if (rc == 0)
    for (size_t t = 0; t < nt; t++) {
      sum_lo += lo[t] % 1000;
      sum_hi += hi[t];
      marks += mark[t];
    }
  printf("%s %d rc %d clean %d rt %lld trim %lld label_rounds %d trim_rounds %d max_rounds %d lo %lld hi %lld marks %lld\n",
         name, idx, rc, rc ? 9 : s.clean, (long long)s.n_rt_members, (long long)s.n_trim_survivors, s.label_rounds,
         s.trim_rounds, s.max_rounds, sum_lo, sum_hi, marks);
  return rc;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % n;
}

// n_txns txns invoked at even positions and completed at odd ones up to
// 2 * width later; n_edges edges between nodes at most 2 * width apart, one in
// `back` against txn order.
void generate(int n_txns, int n_edges, int width, int back, std::vector<lc_ap_txn> *txns,
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

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, f) != 1) return 2;
  std::vector<lc_ap_txn> txns;
  std::vector<lc_ap_edge> edges;
  for (int64_t c = 0; c < n_cases; c++) {
    int64_t n[2];
    if (fread(n, 8, 2, f) != 2) return 2;
    txns.resize((size_t)n[0]);
    edges.resize((size_t)n[1]);
    if (n[0] && fread(txns.data(), sizeof(lc_ap_txn), (size_t)n[0], f) != (size_t)n[0]) return 2;
    if (n[1] && fread(edges.data(), sizeof(lc_ap_edge), (size_t)n[1], f) != (size_t)n[1]) return 2;
    run("case", (int)c, txns, edges);
  }
  fclose(f);
  // (n_txns, n_edges, width, back)
  const int shapes[][4] = {{0, 0, 1, 0},     {1, 0, 1, 0},       {2, 3, 1, 2},       {64, 100, 4, 0},
                           {65, 200, 4, 3},  {300, 900, 8, 10},  {300, 900, 30, 2},  {1000, 3000, 6, 50},
                           {1500, 0, 6, 0},  {1500, 6000, 10, 0}, {1500, 6000, 10, 40}, {1500, 3000, 200, 4}};
  int i = 0;
  for (const auto &sh : shapes) {
    generate(sh[0], sh[1], sh[2], sh[3], &txns, &edges);
    run("gen", i++, txns, edges);
  }
  // refusals: nothing may be written, whatever the arrays' size
  generate(40, 80, 4, 4, &txns, &edges);
  std::vector<lc_ap_txn> bad_txns = txns;
  std::swap(bad_txns[3], bad_txns[4]);
  run("unsorted-txns", 0, bad_txns, edges);
  std::vector<lc_ap_edge> bad_edges = edges;
  std::swap(bad_edges[0], bad_edges[1]);
  run("unsorted-edges", 0, txns, bad_edges);
  bad_edges = edges;
  bad_edges.back().to = 40;
  run("edge-out-of-range", 0, txns, bad_edges);
  return 0;
}
