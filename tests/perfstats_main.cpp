// perfstats_main.cpp — csrc/perfstats_host.cpp under the address and
// undefined-behaviour sanitizers (tests/test_perfstats_host_sanitize.py builds
// and runs this program).  It reads the cases the test wrote, calls
// lc_perf_stats_host once without room (-ENOSPC gives the buckets' counts) and
// once with every array sized exactly, and prints each call's counts; then
// the refusals.  One line per call: a name, a number, then key value pairs.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "perfstats.h"

namespace {

template <class T>
bool get(FILE *f, T *p, size_t n = 1) {
  return n == 0 || fread(p, sizeof(T), n, f) == n;
}

// the arrays, each allocated to its exact size (a vector of size 0 has no room at all)
struct Room {
  std::vector<int64_t> by_f, rate, quant, quant_n, latency;
  std::vector<int32_t> comp_pos;
  lc_ps_out out{};
  Room(int64_t n, const lc_ps_params &p, int64_t rate_cap, int64_t quant_cap, bool points)
      : by_f((size_t)(p.n_f > 0 ? p.n_f : 1) * 4),
        rate((size_t)(p.n_f > 0 ? p.n_f : 1) * 3 * (size_t)rate_cap),
        quant((size_t)(p.n_f > 0 ? p.n_f : 1) * (size_t)quant_cap * (size_t)(p.n_q > 0 && p.n_q <= 8 ? p.n_q : 0)),
        quant_n((size_t)(p.n_f > 0 ? p.n_f : 1) * (size_t)quant_cap),
        latency(points ? (size_t)n : 0),
        comp_pos(points ? (size_t)n : 0) {
    static int64_t nothing[1];  // a table of no entries still has an address
    out.by_f = by_f.data();
    out.rate = rate.empty() ? nothing : rate.data();
    out.quant = quant.empty() ? nothing : quant.data();
    out.quant_n = quant_n.empty() ? nothing : quant_n.data();
    static int32_t no_pos[1];
    out.comp_pos = points ? (comp_pos.empty() ? no_pos : comp_pos.data()) : nullptr;
    out.latency_ns = points ? (latency.empty() ? nothing : latency.data()) : nullptr;
    out.rate_cap = rate_cap;
    out.quant_cap = quant_cap;
  }
};

int run(const char *name, int64_t i, const std::vector<lc_ps_event> &ev, const lc_ps_params &p, bool points) {
  lc_ps_summary s{};
  int rc;
  {
    Room none((int64_t)ev.size(), p, 0, 0, false);
    rc = lc_perf_stats_host(ev.data(), (int64_t)ev.size(), &p, &none.out, &s);
  }
  int64_t latsum = 0, quantsum = 0, paired = 0;
  if (rc == -ENOSPC) {
    Room room((int64_t)ev.size(), p, s.n_rate_buckets, s.n_quant_buckets, points);
    rc = lc_perf_stats_host(ev.data(), (int64_t)ev.size(), &p, &room.out, &s);
    for (size_t k = 0; k < room.comp_pos.size(); k++)
      if (room.comp_pos[k] >= 0) {
        paired++;
        latsum += room.latency[k] % 1000003;
      }
    for (int64_t q : room.quant)
      if (q != LC_PS_NONE) quantsum += q % 1000003;
  }
  printf("%s %lld rc %d valid %d client %lld pairs %lld pending %lld ignored %lld mismatched %lld count %lld ok %lld "
         "fail %lld info %lld tmax %lld nrate %lld nquant %lld paired %lld latsum %lld quantsum %lld\n",
         name, (long long)i, rc, s.valid, (long long)s.n_client, (long long)s.n_pairs, (long long)s.n_pending,
         (long long)s.n_ignored_completions, (long long)s.n_mismatched_f, (long long)s.count, (long long)s.ok,
         (long long)s.fail, (long long)s.info, (long long)s.t_max, (long long)s.n_rate_buckets,
         (long long)s.n_quant_buckets, (long long)paired, (long long)latsum, (long long)quantsum);
  return rc;
}

lc_ps_params params(int32_t n_f, int32_t n_q, int64_t rate_dt, int64_t quant_dt) {
  lc_ps_params p{};
  p.n_f = n_f;
  p.n_q = n_q;
  const double qs[LC_PS_MAX_Q] = {0.5, 0.95, 0.99, 1.0, 0.0, 0.25, 0.75, 0.999};
  for (int k = 0; k < LC_PS_MAX_Q; k++) p.q[k] = qs[k];
  p.rate_dt_ns = rate_dt;
  p.quant_dt_ns = quant_dt;
  return p;
}

lc_ps_event event(int64_t t, int32_t process, uint16_t f, uint8_t type) {
  lc_ps_event e{};
  e.time = t;
  e.process = process;
  e.f = f;
  e.type = type;
  return e;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int64_t n_cases = 0;
  if (!get(f, &n_cases)) return 2;
  for (int64_t i = 0; i < n_cases; i++) {
    int64_t n = 0;
    lc_ps_params p{};
    if (!get(f, &n) || !get(f, &p)) return 2;
    std::vector<lc_ps_event> ev((size_t)n);
    if (!get(f, ev.data(), ev.size())) return 2;
    run("case", i, ev, p, i % 2 == 0);
  }
  fclose(f);
  // generated here: one process holding everything; every event its own process; crashes
  for (int g = 0; g < 6; g++) {
    std::vector<lc_ps_event> ev;
    uint64_t x = 0x9E3779B97F4A7C15ull * (uint64_t)(g + 1);
    const int n = g == 0 ? 0 : 50 + 333 * g;
    int64_t t = 0;
    for (int k = 0; k < n; k++) {
      x ^= x << 13, x ^= x >> 7, x ^= x << 17;
      t += (int64_t)(x % 1000);
      const int32_t process = g == 1 ? 0 : g == 2 ? k : (x >> 20) % 16 == 0 ? -1 : (int32_t)((x >> 24) % (uint64_t)(3 * g));
      ev.push_back(event(t, process, (uint16_t)((x >> 40) % 5), (uint8_t)((x >> 50) % 4)));
    }
    run("gen", g, ev, params(5, g == 3 ? 0 : g == 4 ? 8 : 4, 1000 + g, 2999), g != 5);
  }
  // the refusals: nothing is written (the arrays have no room at all)
  const std::vector<lc_ps_event> ok = {event(0, 0, 0, LC_EV_INVOKE), event(7, 0, 0, LC_EV_OK)};
  run("time", 0, {event(-1, 0, 0, LC_EV_OK)}, params(1, 4, 10, 10), true);
  run("type", 0, {event(0, 0, 0, 4)}, params(1, 4, 10, 10), true);
  run("f", 0, {event(0, 0, 1, LC_EV_OK)}, params(1, 4, 10, 10), true);
  run("nf", 0, ok, params(0, 4, 10, 10), true);
  run("nq", 0, ok, params(1, 9, 10, 10), true);
  run("dt", 0, ok, params(1, 4, 0, 10), true);
  lc_ps_params bad_q = params(1, 4, 10, 10);
  bad_q.q[2] = 1.5;
  run("q", 0, ok, bad_q, true);
  run("maxf", 0, ok, params((int32_t)lcps::kMaxF + 1, 4, 10, 10), true);
  run("table", 0, {event(0, 0, 0, LC_EV_INVOKE), event(lcps::kMaxTableEntries, 0, 0, LC_EV_OK)}, params(1, 4, 1, 1),
      true);
  return 0;
}
