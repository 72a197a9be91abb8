// append_dev.cpp — lc_append_check's driver (include/lincheck_append.h): the
// arrays copied to the context's first device; rules 1 to 6 there
// (append.hip, txngraph.hip); the reads the device left open, rule 7 and the summary on the
// host (append_host.cpp).
#include <algorithm>
#include <chrono>
#include <string>

#include "append.h"
#include "runtime.h"
#include "screen.h"
#include "cycles.h"

using namespace lcrt;

namespace {

constexpr size_t kCountersLen = lcap::kCounters * lcap::kCounterShards * lcap::kCounterStride;
struct Pinned {
  int32_t status[4];
  int64_t count[4];  // set slots, edges, (OK txns), keys
  int64_t counters[kCountersLen];
};

int append_device(lc_ctx *c, const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops, int64_t n_mops,
                  const int64_t *values, int64_t n_values, const lc_ap_out *out, lc_ap_summary *sum,
                  lc_screen_summary *scr,  // scr: null, or lc_append_check_screened's
                  lc_cycle_search_summary *srch = nullptr,
                  bool restricted = false) {  // lc_append_check_restricted: rule 7 over the screen's marks
  const auto t0 = std::chrono::steady_clock::now();
  lcap::Prep p;
  const char *why = nullptr;
  if (lcap::prepare(txns, n_txns, mops, n_mops, values, n_values, out, &p, &why)) {
    set_err(c, std::string("lc_append_check: ") + why);
    return -EINVAL;
  }
  if (n_txns == 0) {
    const int e = lc_append_check_host(txns, n_txns, mops, n_mops, values, n_values, out, sum);
    if (!e && scr) *scr = lcscreen::empty_summary();
    if (!e && srch) *srch = lccyc::search_summary(nullptr);
    return e;
  }
  const size_t nt = (size_t)n_txns, nm = (size_t)n_mops, nr = p.rd_mop.size();
  const int64_t n_work = p.work_off[nr];
  lc_ap_limit_info lim;
  lc_append_limits(&lim);
  if (n_values > lim.max_payload || n_work > lim.max_payload) {
    set_err(c, "lc_append_check: the payload exceeds lc_append_limits' max_payload");
    return -E2BIG;
  }
  if (n_mops > lim.max_mops) {  // (the key table's slot index is an int32)
    set_err(c, "lc_append_check: more mops than lc_append_limits' max_mops");
    return -E2BIG;
  }
  SideState &s = c->aps;
  hipStream_t st;
  if (int e = side_begin(c, s, 6, sizeof(Pinned), &st)) return e;
  // e0 .. e1: the inputs' copies; k0 .. k1 and k2 .. e2: the kernels' two runs
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], e2 = s.ev[2], k0 = s.ev[3], k1 = s.ev[4], k2 = s.ev[5];
  Pinned &h = *s.words<Pinned>();
  const uint64_t wcap = lcap::table_capacity(p.n_appends), kcap = lcap::table_capacity(n_mops);
  const size_t n_slots = 2 * nr + (size_t)n_work, n_edge_room = 2 * nr + (size_t)p.n_appends;
  const size_t temp_bytes = std::max({lcap::edge_temp_bytes((int64_t)n_slots), lcap::rt_temp_bytes(n_txns),
                                      lcap::key_temp_bytes(kcap)});
  lcap::Ws w{};
  w.n_txns = n_txns;
  w.n_mops = n_mops;
  w.n_real = (int64_t)nr;
  w.n_work = n_work;
  w.wcap = wcap;
  w.kcap = kcap;
  // beside w: the edge lists, the key table's occupied slots, the counts (set
  // slots, edges, OK txns, keys), real time's arrays, rocprim's temporary storage
  lc_ap_edge *d_edges_a = nullptr, *d_edges_b = nullptr;
  int32_t *d_kslots = nullptr;
  lcap::RtArrays rt{};
  int64_t *d_count = nullptr;
  uint8_t *d_temp = nullptr;
  auto layout = [&](Carver ws) {
    w.txns = ws.take<lc_ap_txn>(nt);
    w.mops = ws.take<lc_ap_mop>(nm);
    w.values = ws.take<int64_t>((size_t)n_values);
    w.work_off = ws.take<int64_t>(nr + 1);
    w.mop_txn = ws.take<int32_t>(nm);
    w.rd_mop = ws.take<int32_t>(nr);
    w.txn_r0 = ws.take<int32_t>(nt + 1);
    w.wtab = ws.take<unsigned long long>(wcap);
    w.stamp = ws.take<int32_t>(wcap);
    w.ktab = ws.take<int64_t>(kcap);
    w.kbest = ws.take<unsigned long long>(kcap);
    w.kfirst = ws.take<int32_t>(3 * kcap);
    w.kflags = ws.take<int32_t>(kcap);
    w.mop_kslot = ws.take<int32_t>(nm);
    w.mop_last = ws.take<uint8_t>(nm);
    w.ord_w = ws.take<int32_t>((size_t)n_work);
    w.nonprefix = ws.take<uint8_t>(nr);
    w.mop_flags = ws.take<int32_t>(nm);
    w.txn_flags = ws.take<int32_t>(nt);
    w.slots = ws.take<lc_ap_edge>(n_slots);
    // rule 5 bounds the set slots by n_edge_room: the wr / rw slots are two per read, and a ww slot is
    // set only inside an order without repeats and phantoms, whose entries are distinct appends of its key
    d_edges_a = ws.take<lc_ap_edge>(n_edge_room);
    d_edges_b = ws.take<lc_ap_edge>(n_edge_room);
    d_kslots = ws.take<int32_t>(kcap);
    w.keys = ws.take<lc_ap_key>(nm);
    w.counters = ws.take<int64_t>(kCountersLen);
    d_count = ws.take<int64_t>(4);
    w.status = ws.take<int32_t>(4);
    rt.carve(ws, nt);
    d_temp = ws.take<uint8_t>(temp_bytes);
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}))) return e;
  layout(Carver{s.arena.p});
  HIP_TRY(c, hipEventRecord(e0, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.txns), txns, sizeof(lc_ap_txn) * nt, hipMemcpyHostToDevice, st));
  if (nm) {
    HIP_TRY(c, hipMemcpyAsync(writable(w.mops), mops, sizeof(lc_ap_mop) * nm, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(writable(w.mop_txn), p.mop_txn.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice,
                              st));
  }
  if (n_values)
    HIP_TRY(c, hipMemcpyAsync(writable(w.values), values, sizeof(int64_t) * (size_t)n_values, hipMemcpyHostToDevice,
                              st));
  if (nr)
    HIP_TRY(c, hipMemcpyAsync(writable(w.rd_mop), p.rd_mop.data(), sizeof(int32_t) * nr, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.txn_r0), p.txn_r0.data(), sizeof(int32_t) * (nt + 1), hipMemcpyHostToDevice,
                            st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.work_off), p.work_off.data(), sizeof(int64_t) * (nr + 1),
                            hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipEventRecord(e1, st));
  // nothing of an earlier call survives: empty tables (every empty word is
  // all ones), no flags, no edge slots, no counts
  HIP_TRY(c, hipMemsetAsync(w.wtab, 0xFF, sizeof(unsigned long long) * wcap, st));
  HIP_TRY(c, hipMemsetAsync(w.stamp, 0xFF, sizeof(int32_t) * wcap, st));
  HIP_TRY(c, hipMemsetAsync(w.ktab, 0xFF, sizeof(int64_t) * kcap, st));
  HIP_TRY(c, hipMemsetAsync(w.kbest, 0, sizeof(unsigned long long) * kcap, st));
  HIP_TRY(c, hipMemsetAsync(w.kfirst, 0xFF, sizeof(int32_t) * 3 * kcap, st));
  HIP_TRY(c, hipMemsetAsync(w.kflags, 0, sizeof(int32_t) * kcap, st));
  if (nm) HIP_TRY(c, hipMemsetAsync(w.mop_flags, 0, sizeof(int32_t) * nm, st));
  HIP_TRY(c, hipMemsetAsync(w.txn_flags, 0, sizeof(int32_t) * nt, st));  // (no kernel writes them without mops)
  if (nm) HIP_TRY(c, hipMemsetAsync(w.mop_last, 0, nm, st));
  if (nr) HIP_TRY(c, hipMemsetAsync(w.nonprefix, 0, nr, st));
  if (n_slots) HIP_TRY(c, hipMemsetAsync(w.slots, 0xFF, sizeof(lc_ap_edge) * n_slots, st));
  HIP_TRY(c, hipMemsetAsync(w.counters, 0, sizeof(int64_t) * kCountersLen, st));
  HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(int64_t) * 4, st));
  HIP_TRY(c, hipMemsetAsync(w.status, 0, sizeof(int32_t) * 4, st));
  HIP_TRY(c, hipEventRecord(k0, st));
  if (nm) HIP_TRY(c, lcap::launch_rules(w, d_kslots, d_count + 3, d_temp, temp_bytes, st));
  if (n_slots)
    HIP_TRY(c, lcap::launch_edge_select(w.slots, (int64_t)n_slots, d_edges_a, d_count, d_temp, temp_bytes, st));
  HIP_TRY(c, lcap::launch_real_time(w.txns, n_txns, p.n_ok, rt, d_count + 2, d_temp, temp_bytes, st));
  HIP_TRY(c, hipEventRecord(k1, st));
  HIP_TRY(c, hipMemcpyAsync(h.status, w.status, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h.count, d_count, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h.counters, w.counters, sizeof(int64_t) * kCountersLen, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h.status[0]) {
    set_err(c, "lc_append_check: two appends of one (key, element) (mop " + std::to_string(h.status[1]) + " is one)");
    return -EINVAL;
  }
  const int64_t n_sel = h.count[0], n_keys = h.count[3];
  if (n_sel > (int64_t)n_edge_room || n_keys > n_mops) {  // (more edges than rule 5 allows: a bug, not an input)
    set_err(c, "lc_append_check: inconsistent edge or key count");
    return -EIO;
  }
  h.count[1] = 0;
  HIP_TRY(c, hipEventRecord(k2, st));
  if (n_sel > 0) HIP_TRY(c, lcap::launch_edge_sort(d_edges_a, d_edges_b, n_sel, d_count + 1, d_temp, temp_bytes, st));
  HIP_TRY(c, hipEventRecord(e2, st));
  if (n_sel > 0) HIP_TRY(c, hipMemcpyAsync(h.count + 1, d_count + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (nm) HIP_TRY(c, hipMemcpyAsync(out->mop_flags, w.mop_flags, sizeof(int32_t) * nm, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->txn_flags, w.txn_flags, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  if (n_keys)
    HIP_TRY(c, hipMemcpyAsync(out->keys, w.keys, sizeof(lc_ap_key) * (size_t)n_keys, hipMemcpyDeviceToHost, st));
  if (p.n_ok) HIP_TRY(c, hipMemcpyAsync(out->byc, rt.byc, sizeof(int32_t) * (size_t)p.n_ok, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->rt_lo, rt.rt_lo, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->rt_hi, rt.rt_hi, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int64_t n_edges = h.count[1];
  // the screen, on the edges and ranges where they stand: a clean graph spares rule 7
  lc_screen_summary scs{};
  std::vector<int32_t> mark(restricted ? nt : 0);
  if (scr)
    if (int e = lcscreen::screen_resident(c, st, w.txns, n_txns, p.n_ok, d_edges_a, n_edges, rt.byc, rt.rt_hi, &scs,
                                          restricted ? mark.data() : nullptr))
      return e;
  if (n_edges > 0) {  // only the unique edges reach the caller
    HIP_TRY(c, hipMemcpyAsync(out->edges, d_edges_a, sizeof(lc_ap_edge) * (size_t)n_edges, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
  }
  // the key records: ascending by key; first_dup of an order with two
  // phantoms from its definition (the device sees repeats of written elements)
  std::sort(out->keys, out->keys + n_keys, [](const lc_ap_key &a, const lc_ap_key &b) { return a.key < b.key; });
  for (int64_t k = 0; k < n_keys; k++) {
    lc_ap_key &kr = out->keys[k];
    if (!(kr.flags & lcap::kKeyTwoPhantoms)) continue;
    kr.flags &= ~lcap::kKeyTwoPhantoms;
    kr.first_dup = lcap::first_dup_direct(values + mops[kr.longest].value, kr.len);
  }
  // exact but not fast: the txns the device left open (a history without
  // non-prefix reads and twice-phantom orders has none)
  int64_t counts[lcap::kCounters], n_nonprefix = 0;
  for (int b = 0; b < lcap::kCounters; b++) counts[b] = lcap::sum_counters(h.counters, b);
  const int64_t n_slow = counts[5];
  if (n_slow) {
    lcap::Writers wr;
    if (wr.build(txns, n_txns, mops, n_mops)) {
      set_err(c, "lc_append_check: the host found two appends of one pair where the device found none");
      return -EIO;
    }
    for (int64_t t = 0; t < n_txns; t++) {
      if (!(out->txn_flags[t] & lcap::kTxnSlow)) continue;
      lcap::rules34_direct(txns, mops, values, p, wr, t, out->mop_flags, out->txn_flags);
      for (int64_t m = txns[t].mop_off; m < txns[t].mop_off + txns[t].mop_len; m++) {
        n_nonprefix += out->mop_flags[m] & LC_AP_R_NONPREFIX;
        for (int b = 0; b < 5; b++) counts[b] += (out->mop_flags[m] >> (b + 1)) & 1;
      }
    }
  }
  lc_ap_summary sm;
  // not proved clean, and neither phase gave up: every member of an SCC is marked
  lcgraph::MarkedPass mp, *marked = restricted && scs.clean == 0 ? &mp : nullptr;
  if (marked) lccyc::device_pass(c, mark.data(), marked);
  if (int e = lcap::graph_and_summary(txns, n_txns, p, out, n_keys, n_edges, n_nonprefix, counts, &sm,
                                      scr && scs.clean == 1, marked))
    return e;
  sm.n_slow_reads = n_slow;
  sm.h2d_ms = elapsed_ms(e0, e1);
  sm.kernel_ms = elapsed_ms(k0, k1);
  sm.kernel_ms += elapsed_ms(k2, e2);
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  if (scr) *scr = scs;
  if (srch) *srch = lccyc::search_summary(marked);
  return 0;
}

}  // namespace

extern "C" int lc_append_check(lc_ctx *c, const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops,
                               int64_t n_mops, const int64_t *values, int64_t n_values, const lc_ap_out *out,
                               lc_ap_summary *sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_append_check",
                      [&] { return append_device(c, txns, n_txns, mops, n_mops, values, n_values, out, sum, nullptr); });
}

extern "C" int lc_append_check_screened(lc_ctx *c, const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops,
                                        int64_t n_mops, const int64_t *values, int64_t n_values, const lc_ap_out *out,
                                        lc_ap_summary *sum, lc_screen_summary *scr) {
  if (!c) return -EINVAL;
  lc_screen_summary local;
  return no_bad_alloc(c, "lc_append_check_screened", [&] {
    return append_device(c, txns, n_txns, mops, n_mops, values, n_values, out, sum, scr ? scr : &local);
  });
}

extern "C" int lc_append_check_restricted(lc_ctx *c, const lc_ap_txn *txns, int64_t n_txns, const lc_ap_mop *mops,
                                          int64_t n_mops, const int64_t *values, int64_t n_values,
                                          const lc_ap_out *out, lc_ap_summary *sum, lc_screen_summary *scr,
                                          lc_cycle_search_summary *srch) {
  if (!c) return -EINVAL;
  lc_screen_summary local;
  return no_bad_alloc(c, "lc_append_check_restricted", [&] {
    return append_device(c, txns, n_txns, mops, n_mops, values, n_values, out, sum, scr ? scr : &local, srch, true);
  });
}
