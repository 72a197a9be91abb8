// screen_dev.cpp — lc_cycle_screen's driver (include/lincheck_screen.h): the
// txns and edges copied to the context's first device, real time's byc and
// rt_hi made there (txngraph.hip), then the label rounds and the trim rounds
// (screen.hip) in batches of kBatch, the host reading the phase's control
// words once per batch.  screen_resident is the same for the checkers'
// drivers (lc_append_check_screened, lc_wr_check_screened), whose txns, edges
// and ranges already stand on the device.
#include <algorithm>
#include <chrono>
#include <string>

#include "runtime.h"
#include "screen.h"

using namespace lcrt;

namespace {

constexpr size_t kCountersLen = lcscreen::kCounters * lcscreen::kCounterShards * lcscreen::kCounterStride;
struct Pinned {
  lcscreen::Control ctl;
  int64_t counters[kCountersLen];
};

// The screen's own arrays (everything but its inputs and real time's).
void carve_own(Carver &ws, lcscreen::Ws &w, size_t nt, size_t ne, size_t temp_bytes, uint8_t **d_temp) {
  w.e_from = ws.take<int32_t>(ne);
  w.e_to = ws.take<int32_t>(ne);
  w.first = ws.take<int32_t>(nt);
  for (int b = 0; b < 2; b++) {
    w.h[b] = ws.take<int32_t>(nt);
    w.k[b] = ws.take<int32_t>(nt);
    w.alive[b] = ws.take<uint8_t>(nt);
  }
  w.s_rev = ws.take<int32_t>(nt);
  w.p_inc = ws.take<int32_t>(nt);
  w.has_in = ws.take<uint8_t>(nt);
  w.has_out = ws.take<uint8_t>(nt);
  w.mark = ws.take<int32_t>(nt);
  w.counters = ws.take<int64_t>(kCountersLen);
  w.ctl = ws.take<lcscreen::Control>(1);
  *d_temp = ws.take<uint8_t>(temp_bytes);
}

// Nothing of an earlier call survives: no marks, no counts, both phases at round 0.
int reset_own(lc_ctx *c, const lcscreen::Ws &w, hipStream_t st) {
  const size_t nt = (size_t)w.n_txns;
  HIP_TRY(c, hipMemsetAsync(w.has_in, 0, nt, st));
  HIP_TRY(c, hipMemsetAsync(w.has_out, 0, nt, st));
  HIP_TRY(c, hipMemsetAsync(w.counters, 0, sizeof(int64_t) * kCountersLen, st));
  HIP_TRY(c, hipMemsetAsync(w.ctl, 0, sizeof(lcscreen::Control), st));
  return 0;
}

// The setup, the label rounds, the flags, the trim rounds and the marks over
// a workspace whose inputs (txns, edges, byc, rt_hi) stand on the device; the
// counters and control words end in h, every field of *sm but the times is
// written, and *lb names the label buffer that holds the result.
int run_rounds(lc_ctx *c, const lcscreen::Ws &w, Pinned &h, uint8_t *d_temp, size_t temp_bytes, hipStream_t st,
               lc_screen_summary *sm, int *lb) {
  HIP_TRY(c, lcscreen::launch_setup(w, st));
  const int32_t max_rounds = lcscreen::max_rounds();
  // A phase's rounds, kBatch at a time, until the device has seen a quiet
  // round or round max_rounds is through.  After a quiet round both buffers
  // hold the same; after giving up the last round's is max_rounds & 1.
  auto run_phase = [&](const lcscreen::Phase &ph, auto launch_round) -> int {
    for (int32_t r = 1; r <= max_rounds;) {
      for (int i = 0; i < lcscreen::kBatch && r <= max_rounds; i++, r++) HIP_TRY(c, launch_round(r));
      HIP_TRY(c, hipMemcpyAsync(&h.ctl, w.ctl, sizeof(lcscreen::Control), hipMemcpyDeviceToHost, st));
      HIP_TRY(c, hipStreamSynchronize(st));
      if (ph.done) break;
      if (ph.rounds != r - 1) {
        set_err(c, "lc_cycle_screen: the device counted other rounds than were launched");
        return -EIO;
      }
    }
    return 0;
  };
  if (int e = run_phase(h.ctl.label, [&](int r) { return lcscreen::launch_label_round(w, r, d_temp, temp_bytes, st); }))
    return e;
  const bool labelled = h.ctl.label.done;
  *lb = labelled ? 0 : (max_rounds & 1);
  HIP_TRY(c, lcscreen::launch_flags(w, *lb, st));
  bool trimmed = false;
  if (labelled) {
    if (int e = run_phase(h.ctl.trim, [&](int r) { return lcscreen::launch_trim_round(w, r, st); })) return e;
    trimmed = h.ctl.trim.done;
    HIP_TRY(c, lcscreen::launch_marks(w, trimmed ? 0 : (max_rounds & 1), st));
  }
  HIP_TRY(c, hipMemcpyAsync(h.counters, w.counters, sizeof(int64_t) * kCountersLen, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  *sm = lc_screen_summary{};
  sm->max_rounds = max_rounds;
  sm->label_rounds = h.ctl.label.rounds;
  sm->trim_rounds = h.ctl.trim.rounds;
  sm->n_rt_members = lcscreen::sum_counters(h.counters, 0);
  sm->n_trim_survivors = lcscreen::sum_counters(h.counters, 1);
  sm->clean = !(labelled && trimmed) ? -1 : (sm->n_rt_members == 0 && sm->n_trim_survivors == 0);
  return 0;
}

int screen_device(lc_ctx *c, const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
                  const lc_screen_out *out, lc_screen_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  int64_t n_ok = 0;
  const char *why = nullptr;
  if (lcscreen::validate(txns, n_txns, edges, n_edges, out, &n_ok, &why)) {
    set_err(c, std::string("lc_cycle_screen: ") + why);
    return -EINVAL;
  }
  if (n_txns == 0) return lc_cycle_screen_host(txns, n_txns, edges, n_edges, out, sum);
  const size_t nt = (size_t)n_txns, ne = (size_t)n_edges;
  SideState &s = c->scs;
  hipStream_t st;
  if (int e = side_begin(c, s, 4, sizeof(Pinned), &st)) return e;
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], k0 = s.ev[2], k1 = s.ev[3];
  Pinned &h = *s.words<Pinned>();
  const size_t temp_bytes = std::max(lcscreen::scan_temp_bytes(n_txns), lcscreen::rt_temp_bytes(n_txns));
  lcscreen::Ws w{};
  w.n_txns = n_txns;
  w.n_edges = n_edges;
  w.n_ok = n_ok;
  lcscreen::RtArrays rt{};
  int64_t *d_count = nullptr;
  uint8_t *d_temp = nullptr;
  auto layout = [&](Carver ws) {
    w.txns = ws.take<lc_ap_txn>(nt);
    w.edges = ws.take<lc_ap_edge>(ne);
    rt.carve(ws, nt);
    d_count = ws.take<int64_t>(1);
    carve_own(ws, w, nt, ne, temp_bytes, &d_temp);
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}))) return e;
  layout(Carver{s.arena.p});
  w.byc = rt.byc;
  w.rt_hi = rt.rt_hi;
  HIP_TRY(c, hipEventRecord(e0, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.txns), txns, sizeof(lc_ap_txn) * nt, hipMemcpyHostToDevice, st));
  if (ne) HIP_TRY(c, hipMemcpyAsync(writable(w.edges), edges, sizeof(lc_ap_edge) * ne, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipEventRecord(e1, st));
  if (int e = reset_own(c, w, st)) return e;
  HIP_TRY(c, hipEventRecord(k0, st));
  HIP_TRY(c, lcscreen::launch_real_time(w.txns, n_txns, n_ok, rt, d_count, d_temp, temp_bytes, st));
  lc_screen_summary sm;
  int lb = 0;
  if (int e = run_rounds(c, w, h, d_temp, temp_bytes, st, &sm, &lb)) return e;
  HIP_TRY(c, hipEventRecord(k1, st));
  HIP_TRY(c, hipMemcpyAsync(out->reach_lo, w.h[lb], sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->reach_hi, w.k[lb], sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->mark, w.mark, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  sm.h2d_ms = elapsed_ms(e0, e1);
  sm.kernel_ms = elapsed_ms(k0, k1);
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  return 0;
}

}  // namespace

// The screen for a checker's driver (append_dev.cpp, wr_dev.cpp): the txns,
// the unique edges and real time's byc and rt_hi stand on the device, on the
// stream the driver works on; the screen's own arrays are carved from its own
// arena.  The driver wants the summary, and the marks (h_mark, host memory,
// n_txns words) where it restricts the host pass to them (clean == 0).
int lcscreen::screen_resident(lc_ctx *c, hipStream_t st, const lc_ap_txn *d_txns, int64_t n_txns, int64_t n_ok,
                              const lc_ap_edge *d_edges, int64_t n_edges, const int32_t *d_byc, const int32_t *d_rt_hi,
                              lc_screen_summary *scr, int32_t *h_mark) {
  const auto t0 = std::chrono::steady_clock::now();
  SideState &s = c->scs;
  hipStream_t st0;
  if (int e = side_begin(c, s, 4, sizeof(Pinned), &st0)) return e;
  const hipEvent_t k0 = s.ev[2], k1 = s.ev[3];
  Pinned &h = *s.words<Pinned>();
  const size_t temp_bytes = lcscreen::scan_temp_bytes(n_txns);
  lcscreen::Ws w{};
  w.txns = d_txns;
  w.edges = d_edges;
  w.byc = d_byc;
  w.rt_hi = d_rt_hi;
  w.n_txns = n_txns;
  w.n_edges = n_edges;
  w.n_ok = n_ok;
  uint8_t *d_temp = nullptr;
  auto layout = [&](Carver ws) {
    carve_own(ws, w, (size_t)n_txns, (size_t)n_edges, temp_bytes, &d_temp);
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}))) return e;
  layout(Carver{s.arena.p});
  if (int e = reset_own(c, w, st)) return e;
  HIP_TRY(c, hipEventRecord(k0, st));
  int lb = 0;
  if (int e = run_rounds(c, w, h, d_temp, temp_bytes, st, scr, &lb)) return e;
  HIP_TRY(c, hipEventRecord(k1, st));
  // the marks only where the host pass will follow them (no mark is written where the labels gave up)
  if (h_mark && scr->clean == 0)
    HIP_TRY(c, hipMemcpyAsync(h_mark, w.mark, sizeof(int32_t) * (size_t)n_txns, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  scr->kernel_ms = elapsed_ms(k0, k1);
  scr->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return 0;
}

extern "C" int lc_cycle_screen(lc_ctx *c, const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges,
                               int64_t n_edges, const lc_screen_out *out, lc_screen_summary *sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_cycle_screen",
                      [&] { return screen_device(c, txns, n_txns, edges, n_edges, out, sum); });
}
