// perfstats_dev.cpp — lc_perf_stats' driver (include/lincheck_perf.h): the
// records copied to the context's first device and scanned there; once t_max
// has sized the tables, the process sort, the pair pass, the group sorts and
// the selection (perfstats.hip).  The tables' rows are placed into the
// caller's, and by_f, the totals and the verdict read off the rate table, by
// the host code's own function (perfstats.h).
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "perfstats.h"
#include "runtime.h"

using namespace lcrt;

namespace {

int perf_stats_device(lc_ctx *c, const lc_ps_event *ev, int64_t n, const lc_ps_params *p, const lc_ps_out *out,
                      lc_ps_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  const char *why = nullptr;
  if (int rc = lcps::check_params(ev, n, p, out, &why)) {
    set_err(c, std::string("lc_perf_stats: ") + why);
    return rc;
  }
  auto by_host = [&] {  // (its refusals are the device path's, with the same texts)
    const int rc = lc_perf_stats_host(ev, n, p, out, sum);
    if (rc == -EINVAL) {
      int bad = 0;
      for (int64_t i = 0; i < n; i++) bad |= lcps::bad_event(ev[i], p->n_f);
      set_err(c, std::string("lc_perf_stats: ") + lcps::bad_text(bad));
    } else if (rc) {
      set_err(c, rc == -ENOSPC  ? "lc_perf_stats: rate_cap or quant_cap below the buckets' count"
                 : rc == -E2BIG ? "lc_perf_stats: a table above lc_perf_stats_limits' max_table_entries"
                                : "lc_perf_stats: the host code failed");
    }
    return rc;
  };
  if (n < 2) return by_host();  // nothing to pair
  SideState &s = c->pfs;
  hipStream_t st;
  if (int e = side_begin(c, s, 6, sizeof(lcps::Status), &st)) return e;
  // e0 .. e1: the records' copy; k0 .. k1: the scan; k2 .. k3: everything after it
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], k0 = s.ev[2], k1 = s.ev[3], k2 = s.ev[4], k3 = s.ev[5];
  lcps::Status &h = *s.words<lcps::Status>();
  lc_ps_limit_info lim;
  lc_perf_stats_limits(&lim);
  const size_t ne = (size_t)n;
  const bool points = out->comp_pos != nullptr;
  lcps::Ws w{};
  w.n_events = n;
  w.n_f = p->n_f;
  w.n_q = p->n_q;
  std::copy_n(p->q, LC_PS_MAX_Q, w.q);
  w.rate_dt = p->rate_dt_ns;
  w.quant_dt = p->quant_dt_ns;
  w.lds_entries = lim.lds_entries;
  // the largest group key is n_f * n_quant <= max_table_entries: its bits bound the sorts' storage
  int max_group_bits = 1;
  while ((int64_t(1) << max_group_bits) <= lim.max_table_entries) max_group_bits++;
  w.temp_bytes = lcps::sort_temp_bytes(n, max_group_bits);
  // What the scan writes comes first, so that the tables, whose sizes t_max
  // decides, move nothing of it when they are carved.
  size_t keep = 0;
  auto layout = [&](Carver ws, int64_t hist_entries, int64_t quant_entries) {
    w.ev = ws.take<lc_ps_event>(ne);
    w.pkey_in = ws.take<uint32_t>(ne);
    w.ppos_in = ws.take<int32_t>(ne);
    w.comp_pos = ws.take<int32_t>(points ? ne : 0);
    w.latency = ws.take<int64_t>(points ? ne : 0);
    w.status = ws.take<lcps::Status>(1);
    keep = ws.size;
    w.pkey = ws.take<uint32_t>(ne);
    w.ppos = ws.take<int32_t>(ne);
    w.gkey = ws.take<uint32_t>(ne);
    w.gkey2 = ws.take<uint32_t>(ne);
    w.glat = ws.take<int64_t>(ne);
    w.glat2 = ws.take<int64_t>(ne);
    w.temp = ws.take<char>(w.temp_bytes);
    w.hist = ws.take<unsigned long long>((size_t)hist_entries);
    w.quant = ws.take<int64_t>((size_t)quant_entries);
    if (!points) w.comp_pos = nullptr, w.latency = nullptr;  // (the kernels' test)
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}, 0, 0))) return e;
  layout(Carver{s.arena.p}, 0, 0);
  HIP_TRY(c, hipEventRecord(e0, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.ev), ev, sizeof(lc_ps_event) * ne, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipEventRecord(e1, st));
  HIP_TRY(c, hipMemsetAsync(w.status, 0, sizeof(lcps::Status), st));  // no count of an earlier call survives
  HIP_TRY(c, hipEventRecord(k0, st));
  HIP_TRY(c, lcps::launch_scan(w, st));
  HIP_TRY(c, hipEventRecord(k1, st));
  HIP_TRY(c, hipMemcpyAsync(&h, w.status, sizeof(lcps::Status), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h.bad) {
    set_err(c, std::string("lc_perf_stats: ") + lcps::bad_text(h.bad));
    return -EINVAL;
  }
  if (h.n_client == 0) return by_host();
  const int64_t t_max = (int64_t)h.t_max;
  w.n_client = (int64_t)h.n_client;
  if (int rc = lcps::check_tables(t_max, p, out, &w.n_rate, &w.n_quant, &why)) {
    set_err(c, std::string("lc_perf_stats: ") + why);
    if (rc == -ENOSPC) lcps::summary_for_room(sum, n, w.n_client, t_max, w.n_rate, w.n_quant);
    return rc;
  }
  const int64_t nf = p->n_f, nq = p->n_q;
  const int64_t rate_entries = nf * 3 * w.n_rate, groups = nf * w.n_quant, quant_entries = groups * nq;
  w.hist_entries = rate_entries + groups;
  int group_bits = 1;
  while ((int64_t(1) << group_bits) <= groups) group_bits++;
  const size_t need = layout(Carver{}, w.hist_entries, quant_entries);
  if (need > s.arena.cap) {  // the arena grows; what the scan wrote moves along
    char *np = nullptr;
    if (hipMalloc(reinterpret_cast<void **>(&np), need) != hipSuccess) {
      set_err(c, "lc_perf_stats: hipMalloc: out of device memory for the tables");
      return -ENOMEM;
    }
    hipError_t e = hipMemcpyAsync(np, s.arena.p, keep, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
      (void)hipFree(np);
      set_err(c, std::string("lc_perf_stats: moving the arena: ") + hipGetErrorString(e));
      return -EIO;
    }
    (void)hipFree(s.arena.p);
    s.arena.p = np;
    s.arena.cap = need;
  }
  layout(Carver{s.arena.p}, w.hist_entries, quant_entries);

  std::vector<int64_t> tables((size_t)(w.hist_entries + quant_entries));
  HIP_TRY(c, hipEventRecord(k2, st));
  HIP_TRY(c, hipMemsetAsync(w.hist, 0, sizeof(int64_t) * (size_t)w.hist_entries, st));
  HIP_TRY(c, lcps::launch_process_sort(w, st));
  HIP_TRY(c, lcps::launch_pairs(w, st));
  if (nq > 0) {
    HIP_TRY(c, lcps::launch_group_sort(w, group_bits, st));
    HIP_TRY(c, lcps::launch_select(w, st));
  }
  HIP_TRY(c, hipEventRecord(k3, st));
  HIP_TRY(c, hipMemcpyAsync(&h, w.status, sizeof(lcps::Status), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(tables.data(), w.hist, sizeof(int64_t) * (size_t)w.hist_entries, hipMemcpyDeviceToHost,
                            st));
  if (quant_entries)
    HIP_TRY(c, hipMemcpyAsync(tables.data() + w.hist_entries, w.quant, sizeof(int64_t) * (size_t)quant_entries,
                              hipMemcpyDeviceToHost, st));
  if (points) {
    HIP_TRY(c, hipMemcpyAsync(out->comp_pos, w.comp_pos, sizeof(int32_t) * ne, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(out->latency_ns, w.latency, sizeof(int64_t) * ne, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  lc_ps_summary sm{};
  sm.n_events = n;
  sm.n_client = w.n_client;
  sm.n_pairs = (int64_t)h.n_pairs;
  sm.n_pending = (int64_t)h.n_pending;
  sm.n_ignored_completions = (int64_t)h.n_ignored;
  sm.n_mismatched_f = (int64_t)h.n_mismatched;
  sm.t_max = t_max;
  sm.n_rate_buckets = w.n_rate;
  sm.n_quant_buckets = w.n_quant;
  lcps::place_tables(p, tables.data(), tables.data() + rate_entries, tables.data() + w.hist_entries, w.n_rate,
                     w.n_quant, out, &sm);
  sm.h2d_ms = elapsed_ms(e0, e1);
  sm.kernel_ms = elapsed_ms(k0, k1) + elapsed_ms(k2, k3);
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  return 0;
}

}  // namespace

extern "C" int lc_perf_stats(lc_ctx *c, const lc_ps_event *ev, int64_t n_events, const lc_ps_params *params,
                             const lc_ps_out *out, lc_ps_summary *sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_perf_stats", [&] { return perf_stats_device(c, ev, n_events, params, out, sum); });
}
