// watch_main.cpp — lc_watch_check_host (csrc/watch_host.cpp) as a stand-alone
// program for tests/test_watch_host_sanitize.py, which builds it with the
// address and undefined-behaviour sanitizers.  It reads the cases the test
// wrote (argv[1]: n_cases, then per case n_threads, n_values, n_nonmonotonic,
// the threads, the values) and generates some of its own: logs a few edits
// apart over few symbols, so that classes, collisions of length, long snakes
// and scripts of every shape occur.  One line per call: the code and the
// summary's counts, judged by the test.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../include/lincheck_watch.h"

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
  Exact<int32_t> cls;
  Exact<int64_t> distance;
  Exact<lc_wt_delta> deltas;
  Exact<lc_wt_edit> edits;
  lc_wt_out out;
  Arrays(size_t nt, int64_t edit_cap) : cls(nt), distance(nt), deltas(nt), edits((size_t)edit_cap) {
    out = lc_wt_out{cls.p, distance.p, deltas.p, edits.p, edit_cap};
  }
};

int run(const char *name, int idx, const std::vector<lc_wt_thread> &threads, const std::vector<int64_t> &values,
        int64_t n_nonmonotonic, uint32_t flags) {
  // the inputs sized exactly too
  Exact<lc_wt_thread> th(threads.size());
  Exact<int64_t> vals(values.size());
  for (size_t i = 0; i < threads.size(); i++) th[i] = threads[i];
  for (size_t i = 0; i < values.size(); i++) vals[i] = values[i];
  const int64_t nt = (int64_t)threads.size(), nv = (int64_t)values.size();
  // first with no room for edits at all, then with exactly the room asked for
  Arrays none(threads.size(), 0);
  lc_wt_summary s{};
  int rc = lc_watch_check_host(th.p, nt, vals.p, nv, n_nonmonotonic, flags, &none.out, &s);
  int64_t dist_sum = 0;
  if (rc == -ENOSPC) {
    const int64_t want = s.n_edits;
    Arrays a(threads.size(), want);
    rc = lc_watch_check_host(th.p, nt, vals.p, nv, n_nonmonotonic, flags, &a.out, &s);
    if (rc == 0 && s.n_edits != want) rc = -1000;
    int64_t sum = 0;  // every output read once
    for (int64_t i = 0; i < s.n_edits; i++) sum += a.edits[(size_t)i].at + a.edits[(size_t)i].op;
    for (int64_t i = 0; i < s.n_deltas; i++) sum += a.deltas[(size_t)i].script_len;
    for (int64_t i = 0; i < nt; i++) dist_sum += a.distance[(size_t)i] + 0 * a.cls[(size_t)i];
    if (sum < 0) rc = -1001;
  } else if (rc == 0) {
    for (int64_t i = 0; i < nt; i++) dist_sum += none.distance[(size_t)i] + 0 * none.cls[(size_t)i];
  }
  printf("%s %d rc %d valid %d canonical %d size %lld threads %lld classes %lld deltas %lld edits %lld noscript %lld "
         "collisions %lld reveq %d dist %lld\n",
         name, idx, rc, rc ? 9 : s.valid, rc ? -9 : s.canonical, (long long)s.canonical_size, (long long)s.n_threads,
         (long long)s.n_classes, (long long)s.n_deltas, (long long)s.n_edits, (long long)s.n_no_script,
         (long long)s.n_collisions, s.revisions_equal, (long long)dist_sum);
  return rc;
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t n) {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 33) % n;
}

// n_threads logs off one base log of `len` values over `syms` symbols: a third
// equal to it, the rest up to `edits` single edits away.
void generate(int n_threads, int len, int syms, int edits, std::vector<lc_wt_thread> *threads,
              std::vector<int64_t> *values) {
  threads->clear();
  values->clear();
  std::vector<int64_t> base((size_t)len);
  for (int64_t &v : base) v = rnd((uint32_t)syms);
  for (int t = 0; t < n_threads; t++) {
    std::vector<int64_t> log = base;
    if (rnd(3) != 0)
      for (int e = (int)rnd((uint32_t)edits + 1); e > 0; e--) {
        const size_t at = rnd((uint32_t)log.size() + 1);
        if (rnd(2) && at < log.size()) log.erase(log.begin() + (long)at);
        else log.insert(log.begin() + (long)at, rnd((uint32_t)syms));
      }
    threads->push_back(lc_wt_thread{(int64_t)values->size(), (int64_t)log.size(), 7, 100 + t});
    values->insert(values->end(), log.begin(), log.end());
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, f) != 1) return 2;
  std::vector<lc_wt_thread> threads;
  std::vector<int64_t> values;
  for (int64_t c = 0; c < n_cases; c++) {
    int64_t hdr[3];
    if (fread(hdr, 8, 3, f) != 3) return 2;
    threads.resize((size_t)hdr[0]);
    values.resize((size_t)hdr[1]);
    if (hdr[0] && fread(threads.data(), sizeof(lc_wt_thread), threads.size(), f) != threads.size()) return 2;
    if (hdr[1] && fread(values.data(), sizeof(int64_t), values.size(), f) != values.size()) return 2;
    if (run("case", (int)c, threads, values, hdr[2], 0)) return 1;
  }
  fclose(f);
  // {threads, length, symbols, edits}
  static const int kShapes[][4] = {{0, 0, 1, 0},  {1, 5, 2, 0},    {2, 0, 2, 1},     {5, 1, 1, 2},
                                   {9, 40, 2, 4}, {33, 300, 3, 6}, {8, 5000, 2, 40}, {4, 20000, 1000, 3}};
  int idx = 0;
  for (const auto &sh : kShapes) {
    generate(sh[0], sh[1], sh[2], sh[3], &threads, &values);
    if (run("gen", idx++, threads, values, 0, 0)) return 1;
  }
  // the contract's refusals: nothing may be written, nothing read out of bounds
  generate(5, 10, 2, 2, &threads, &values);
  std::vector<lc_wt_thread> bad = threads;
  bad[3].thread = bad[1].thread;
  if (run("twice", 0, bad, values, 0, 0) != -EINVAL) return 1;
  bad = threads;
  bad[4].len += 1;  // (the last log: it now runs past n_values)
  if (run("past", 0, bad, values, 0, 0) != -EINVAL) return 1;
  bad = threads;
  bad[2].off = -1;
  if (run("negative", 0, bad, values, 0, 0) != -EINVAL) return 1;
  bad = threads;
  bad[2].len = 0x7FFFFFFF;
  if (run("long", 0, bad, values, 0, 0) != -EINVAL) return 1;
  if (run("flags", 0, threads, values, 0, 2) != -EINVAL) return 1;
  return 0;
}
