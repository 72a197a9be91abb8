// wr_dev.cpp — lc_wr_check's driver (include/lincheck_wr.h): the arrays
// copied to the context's first device; rules 1 to 8 there (wr.hip, and
// txngraph.hip's launchers for the edges and real time); rule 9 and the summary
// on the host (wr_host.cpp, graph_host.cpp).
#include <algorithm>
#include <chrono>
#include <string>

#include "runtime.h"
#include "screen.h"
#include "cycles.h"
#include "wr.h"
#include "wr_lin.h"

using namespace lcrt;

namespace {

constexpr size_t kCountersLen = lcwr::kCounters * lcwr::kCounterShards * lcwr::kCounterStride;
struct Pinned {
  int32_t status[4];
  int64_t count[4];  // edges selected, unique edges, OK txns, keys
  int64_t items;     // the rw items
  int64_t counters[kCountersLen];
};

int wr_device(lc_ctx *c, const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops,
              uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum,
              lc_screen_summary *scr,  // scr: null, or lc_wr_check_screened's
              lc_cycle_search_summary *srch = nullptr,
              bool restricted = false) {  // lc_wr_check_restricted: rule 9 over the screen's marks
  const auto t0 = std::chrono::steady_clock::now();
  lcwr::Prep p;
  const char *why = nullptr;
  if (lcwr::prepare(txns, n_txns, mops, n_mops, flags, out, &p, &why)) {
    set_err(c, std::string("lc_wr_check: ") + why);
    return -EINVAL;
  }
  if (n_txns == 0) {
    const int e = lc_wr_check_host(txns, n_txns, mops, n_mops, flags, out, sum);
    if (!e && scr) *scr = lcscreen::empty_summary();
    if (!e && srch) *srch = lccyc::search_summary(nullptr);
    return e;
  }
  lc_wr_limit_info lim;
  lc_wr_limits(&lim);
  if (n_mops > lim.max_mops) {  // (a table slot's index is an int32)
    set_err(c, "lc_wr_check: more mops than lc_wr_limits' max_mops");
    return -E2BIG;
  }
  const size_t nt = (size_t)n_txns, nm = (size_t)n_mops;
  SideState &s = c->wrs;
  hipStream_t st;
  if (int e = side_begin(c, s, 6, sizeof(Pinned), &st)) return e;
  // e0 .. e1: the inputs' copies; k0 .. k1 and k2 .. e2: the kernels' two runs
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], e2 = s.ev[2], k0 = s.ev[3], k1 = s.ev[4], k2 = s.ev[5];
  Pinned &h = *s.words<Pinned>();
  // both tables: entries are at most one per mop
  const uint64_t vcap = lcwr::table_capacity(n_mops), kcap = vcap;
  int rounds = 1;  // rule 6: 2^rounds above the versions' number (at most one per mop)
  while (rounds < 32 && (int64_t(1) << rounds) <= n_mops) rounds++;
  rounds++;
  const size_t temp_bytes = std::max(lcwr::scan_temp_bytes(vcap, kcap), lcwr::rt_temp_bytes(n_txns));
  lcwr::Ws w{};
  w.n_txns = n_txns;
  w.n_mops = n_mops;
  w.flags = flags;
  w.vcap = vcap;
  w.kcap = kcap;
  // beside w: the key table's occupied slots, the counts (edges selected,
  // unique edges, OK txns, keys), real time's arrays, rocprim's temporary
  // storage; then, sized by the rw items, the two edge buffers and theirs
  lc_wr_edge *d_edges_b = nullptr;
  int32_t *d_kslots = nullptr;
  lcwr::RtArrays rt{};
  int64_t *d_count = nullptr;
  uint8_t *d_temp = nullptr, *d_etemp = nullptr;
  // Everything the rules need comes first, so that the edge buffers, whose
  // size the device finds out, move nothing when they are carved again.
  auto layout = [&](Carver ws, int64_t n_items) {
    w.txns = ws.take<lc_wr_txn>(nt);
    w.mops = ws.take<lc_wr_mop>(nm);
    w.mop_txn = ws.take<int32_t>(nm);
    w.vtab = ws.take<unsigned long long>(vcap);
    w.vwriter = ws.take<int32_t>(vcap);
    w.vnread = ws.take<int32_t>(vcap);
    w.vnrw = ws.take<int32_t>(vcap);
    w.vnchild = ws.take<int32_t>(vcap);
    w.ptr_a = ws.take<int32_t>(vcap);
    w.ptr_b = ws.take<int32_t>(vcap);
    w.rd_off = ws.take<int32_t>(vcap + 1);
    w.ch_off = ws.take<int32_t>(vcap + 1);
    w.rd_cur = ws.take<int32_t>(vcap);
    w.ch_cur = ws.take<int32_t>(vcap);
    w.rc = ws.take<int64_t>(vcap + 1);
    w.item_off = ws.take<int64_t>(vcap + 1);
    w.readers = ws.take<int32_t>(nm);
    w.children = ws.take<int32_t>(2 * nm);
    w.ktab = ws.take<int64_t>(kcap);
    w.kflags = ws.take<int32_t>(kcap);
    w.kcount = ws.take<int32_t>(3 * kcap);
    w.kcyc = ws.take<unsigned long long>(kcap);
    w.mop_kslot = ws.take<int32_t>(nm);
    w.mop_vslot = ws.take<int32_t>(nm);
    w.mop_last = ws.take<uint8_t>(nm);
    w.mop_par = ws.take<int32_t>(nm);
    w.mop_nil = ws.take<int32_t>(nm);
    w.mop_flags = ws.take<int32_t>(nm);
    w.txn_flags = ws.take<int32_t>(nt);
    d_kslots = ws.take<int32_t>(kcap);
    w.keys = ws.take<lc_wr_key>(nm);
    w.counters = ws.take<int64_t>(kCountersLen);
    d_count = ws.take<int64_t>(4);
    w.status = ws.take<int32_t>(4);
    rt.carve(ws, nt);
    d_temp = ws.take<uint8_t>(temp_bytes);
    const size_t n_slots = nm + (size_t)n_items;
    w.slots = ws.take<lc_wr_edge>(n_slots);
    d_edges_b = ws.take<lc_wr_edge>(n_slots);
    d_etemp = ws.take<uint8_t>(lcwr::edge_temp_bytes((int64_t)n_slots));
    return ws.size;
  };
  // The copies in and everything up to the synchronisation that brings the
  // status and the number of rw items, with room for `room` of them.
  auto first_run = [&](int64_t room) -> int {
    if (int e = ensure(c, s.arena, layout(Carver{}, room))) return e;
    layout(Carver{s.arena.p}, room);
    HIP_TRY(c, hipEventRecord(e0, st));
    HIP_TRY(c, hipMemcpyAsync(writable(w.txns), txns, sizeof(lc_wr_txn) * nt, hipMemcpyHostToDevice, st));
    if (nm) {
      HIP_TRY(c, hipMemcpyAsync(writable(w.mops), mops, sizeof(lc_wr_mop) * nm, hipMemcpyHostToDevice, st));
      HIP_TRY(c, hipMemcpyAsync(writable(w.mop_txn), p.mop_txn.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice,
                                st));
    }
    HIP_TRY(c, hipEventRecord(e1, st));
    // nothing of an earlier call survives: empty tables (every empty word is
    // all ones), no writers, parents or pointers (-1), no counts, no flags
    HIP_TRY(c, hipMemsetAsync(w.vtab, 0xFF, sizeof(unsigned long long) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.vwriter, 0xFF, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.vnread, 0, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.vnrw, 0, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.vnchild, 0, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.ptr_a, 0xFF, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.ptr_b, 0xFF, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.rd_cur, 0, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.ch_cur, 0, sizeof(int32_t) * vcap, st));
    HIP_TRY(c, hipMemsetAsync(w.rc, 0, sizeof(int64_t) * (vcap + 1), st));
    HIP_TRY(c, hipMemsetAsync(w.item_off, 0, sizeof(int64_t) * (vcap + 1), st));
    HIP_TRY(c, hipMemsetAsync(w.ktab, 0xFF, sizeof(int64_t) * kcap, st));
    HIP_TRY(c, hipMemsetAsync(w.kflags, 0, sizeof(int32_t) * kcap, st));
    HIP_TRY(c, hipMemsetAsync(w.kcount, 0, sizeof(int32_t) * 3 * kcap, st));
    HIP_TRY(c, hipMemsetAsync(w.kcyc, 0xFF, sizeof(unsigned long long) * kcap, st));
    if (nm) {
      HIP_TRY(c, hipMemsetAsync(w.mop_last, 0, nm, st));
      HIP_TRY(c, hipMemsetAsync(w.mop_par, 0xFF, sizeof(int32_t) * nm, st));
      HIP_TRY(c, hipMemsetAsync(w.mop_nil, 0xFF, sizeof(int32_t) * nm, st));
      HIP_TRY(c, hipMemsetAsync(w.mop_flags, 0, sizeof(int32_t) * nm, st));
      HIP_TRY(c, hipMemsetAsync(w.slots, 0xFF, sizeof(lc_wr_edge) * nm, st));  // (the items' slots: once counted)
    }
    HIP_TRY(c, hipMemsetAsync(w.txn_flags, 0, sizeof(int32_t) * nt, st));  // (no kernel writes them without mops)
    HIP_TRY(c, hipMemsetAsync(w.counters, 0, sizeof(int64_t) * kCountersLen, st));
    HIP_TRY(c, hipMemsetAsync(d_count, 0, sizeof(int64_t) * 4, st));
    HIP_TRY(c, hipMemsetAsync(w.status, 0, sizeof(int32_t) * 4, st));
    HIP_TRY(c, hipEventRecord(k0, st));
    if (nm) HIP_TRY(c, lcwr::launch_rules(w, rounds, d_kslots, d_count + 3, d_temp, temp_bytes, st));
    HIP_TRY(c, lcwr::launch_real_time(w.txns, n_txns, p.n_ok, rt, d_count + 2, d_temp, temp_bytes, st));
    HIP_TRY(c, hipEventRecord(k1, st));
    HIP_TRY(c, hipMemcpyAsync(h.status, w.status, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h.count, d_count, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&h.items, w.item_off + vcap, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h.counters, w.counters, sizeof(int64_t) * kCountersLen, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return 0;
  };
  // the first run guesses one rw item per mop (the arena keeps what earlier calls needed)
  int64_t room = std::min<int64_t>(n_mops, std::max<int64_t>(lim.max_edges - n_mops, 0));
  if (int e = first_run(room)) return e;
  if (h.status[0]) {
    set_err(c, "lc_wr_check: two writes of one (key, value) (mop " + std::to_string(h.status[1]) + " is one)");
    return -EINVAL;
  }
  const int64_t n_items = h.items, n_keys = h.count[3];
  if (n_items < 0 || n_keys > n_mops) {
    set_err(c, "lc_wr_check: inconsistent item or key count");
    return -EIO;
  }
  if (n_items > lim.max_edges - n_mops) {
    set_err(c, "lc_wr_check: " + std::to_string(n_mops + n_items) + " candidate edges exceed lc_wr_limits' max_edges (" +
                   std::to_string(lim.max_edges) + ")");
    return -E2BIG;
  }
  if (n_items > room) {
    // More rw items than the guess.  Where the arena holds them the buffers
    // are carved again in place (they lie last); where it must grow, a new
    // arena has lost the first run's arrays, and the run is made again.
    if (layout(Carver{}, n_items) <= s.arena.cap) {
      layout(Carver{s.arena.p}, n_items);
    } else {
      if (int e = first_run(n_items)) return e;
      if (h.status[0] || h.items != n_items) {
        set_err(c, "lc_wr_check: the second run disagrees with the first");
        return -EIO;
      }
    }
  }
  const size_t n_slots = nm + (size_t)n_items;
  const size_t etemp_bytes = lcwr::edge_temp_bytes((int64_t)n_slots);
  h.count[1] = 0;
  HIP_TRY(c, hipEventRecord(k2, st));
  if (n_items) HIP_TRY(c, hipMemsetAsync(w.slots + nm, 0xFF, sizeof(lc_wr_edge) * (size_t)n_items, st));
  HIP_TRY(c, lcwr::launch_items(w, n_items, st));
  int64_t n_sel = 0;
  if (n_slots) {
    HIP_TRY(c, lcwr::launch_edge_select(w.slots, (int64_t)n_slots, d_edges_b, d_count, d_etemp, etemp_bytes, st));
    HIP_TRY(c, hipMemcpyAsync(h.count, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    n_sel = h.count[0];
    if (n_sel < 0 || n_sel > (int64_t)n_slots) {
      set_err(c, "lc_wr_check: inconsistent edge count");
      return -EIO;
    }
    // sorted into the slots' place, unique back into the other buffer
    if (n_sel > 0) HIP_TRY(c, lcwr::launch_edge_sort(d_edges_b, w.slots, n_sel, d_count + 1, d_etemp, etemp_bytes, st));
  }
  HIP_TRY(c, hipEventRecord(e2, st));
  if (n_sel > 0) HIP_TRY(c, hipMemcpyAsync(h.count + 1, d_count + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int64_t n_edges = h.count[1];
  if (n_edges < 0 || n_edges > n_sel) {
    set_err(c, "lc_wr_check: inconsistent unique edge count");
    return -EIO;
  }
  if (n_edges > out->edge_cap) {
    set_err(c, "lc_wr_check: " + std::to_string(n_edges) + " edges, edge_cap " + std::to_string(out->edge_cap));
    if (sum) {
      *sum = lc_wr_summary{};
      sum->n_edges = n_edges;
      sum->n_edges_raw = n_sel;
    }
    return -ENOSPC;
  }
  // the screen, on the edges and ranges where they stand: a clean graph spares rule 9
  lc_screen_summary scs{};
  std::vector<int32_t> mark(restricted ? nt : 0);
  if (scr)
    if (int e = lcscreen::screen_resident(c, st, w.txns, n_txns, p.n_ok, d_edges_b, n_edges, rt.byc, rt.rt_hi, &scs,
                                          restricted ? mark.data() : nullptr))
      return e;
  if (nm) HIP_TRY(c, hipMemcpyAsync(out->mop_flags, w.mop_flags, sizeof(int32_t) * nm, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->txn_flags, w.txn_flags, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  if (n_keys)
    HIP_TRY(c, hipMemcpyAsync(out->keys, w.keys, sizeof(lc_wr_key) * (size_t)n_keys, hipMemcpyDeviceToHost, st));
  if (p.n_ok) HIP_TRY(c, hipMemcpyAsync(out->byc, rt.byc, sizeof(int32_t) * (size_t)p.n_ok, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->rt_lo, rt.rt_lo, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->rt_hi, rt.rt_hi, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  if (n_edges > 0)  // only the unique edges reach the caller
    HIP_TRY(c, hipMemcpyAsync(out->edges, d_edges_b, sizeof(lc_wr_edge) * (size_t)n_edges, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  std::sort(out->keys, out->keys + n_keys, [](const lc_wr_key &a, const lc_wr_key &b) { return a.key < b.key; });
  int64_t counts[lcwr::kCounters];
  for (int b = 0; b < lcwr::kCounters; b++) counts[b] = lcwr::sum_counters(h.counters, b);
  lc_wr_summary sm;
  // not proved clean, and neither phase gave up: every member of an SCC is marked
  lcgraph::MarkedPass mp, *marked = restricted && scs.clean == 0 ? &mp : nullptr;
  if (marked) lccyc::device_pass(c, mark.data(), marked);
  if (int e = lcwr::graph_and_summary(txns, n_txns, p, out, n_keys, n_edges, counts, &sm, scr && scs.clean == 1,
                                      marked))
    return e;
  sm.n_edges_raw = n_sel;
  sm.h2d_ms = elapsed_ms(e0, e1);
  sm.kernel_ms = elapsed_ms(k0, k1);
  sm.kernel_ms += elapsed_ms(k2, e2);
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  if (scr) *scr = scs;
  if (srch) *srch = lccyc::search_summary(marked);
  return 0;
}

// lc_wr_check_lin with the lin bit set (include/lincheck_wrlin.h): wr_device's
// course with wr_lin.hip's rules 4', 6' and 7' in the place of wr.hip's 4, 6
// and 7.  The workspace, the pinned words and the first six events are
// lc_wr_check's; two more of the state's events time the lin steps.
int wr_lin_device(lc_ctx *c, const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops,
                  uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum, lc_wr_lin_key *lin_keys,
                  lc_wr_lin_summary *lin_sum) {
  const auto t0 = std::chrono::steady_clock::now();
  lcwr::Prep p;
  const char *why = nullptr;
  if (!lcwr::lin_flags_ok(flags) || !lin_keys) {
    set_err(c, !lin_keys ? "lc_wr_check_lin: null lin_keys" : "lc_wr_check_lin: unknown flag");
    return -EINVAL;
  }
  if (lcwr::prepare(txns, n_txns, mops, n_mops, flags & LC_WR_WFR_KEYS, out, &p, &why)) {
    set_err(c, std::string("lc_wr_check_lin: ") + why);
    return -EINVAL;
  }
  if (n_txns == 0) return lc_wr_check_lin_host(txns, n_txns, mops, n_mops, flags, out, sum, lin_keys, lin_sum);
  if (!(flags & LC_WR_LINEARIZABLE_KEYS)) {  // lc_wr_check itself, and records of zeros
    lc_wr_summary sm;
    const int e = wr_device(c, txns, n_txns, mops, n_mops, flags, out, &sm, nullptr);
    if (e && e != -ENOSPC) return e;
    if (sum) *sum = sm;
    if (!e) lcwr::lin_zero(lin_keys, sm.n_keys, lin_sum);
    return e;
  }
  lc_wr_limit_info lim;
  lc_wr_limits(&lim);
  if (n_mops > lim.max_mops) {  // (a table slot's index is an int32)
    set_err(c, "lc_wr_check_lin: more mops than lc_wr_limits' max_mops");
    return -E2BIG;
  }
  const size_t nt = (size_t)n_txns, nm = (size_t)n_mops;
  SideState &s = c->wrs;
  hipStream_t st;
  if (int e = side_begin(c, s, 8, sizeof(Pinned), &st)) return e;
  // e0 .. e1: the inputs' copies; k0 .. k1 and k2 .. e2: the kernels' two runs; l0 .. l1 inside the first
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], e2 = s.ev[2], k0 = s.ev[3], k1 = s.ev[4], k2 = s.ev[5];
  const hipEvent_t l0 = s.ev[6], l1 = s.ev[7];
  Pinned &h = *s.words<Pinned>();
  const uint64_t vcap = lcwr::table_capacity(n_mops), kcap = vcap;
  const size_t temp_bytes = std::max(lcwr::lin_temp_bytes(n_mops, vcap, kcap), lcwr::rt_temp_bytes(n_txns));
  const size_t mat_words = (size_t)lcwr::lin_matrix_words(n_mops);
  lcwr::Ws w{};
  lcwr::LinWs l{};
  w.n_txns = n_txns;
  w.n_mops = n_mops;
  w.flags = flags;
  w.vcap = vcap;
  w.kcap = kcap;
  l.mat_words = (int64_t)mat_words;
  lc_wr_edge *d_edges_b = nullptr;
  int32_t *d_kslots = nullptr;
  lcwr::RtArrays rt{};
  int64_t *d_count = nullptr;
  uint8_t *d_temp = nullptr, *d_etemp = nullptr;
  // What is zeroed lies in one run (zero0 .. zero1), what is set to all ones in
  // another (ones0 .. ones1); the edge buffers, whose size the device finds
  // out, come last and move nothing when they are carved again.  Of Ws, the
  // pointer arrays of rule 6 and the children groups are not used (null).
  char *zero0 = nullptr, *zero1 = nullptr, *ones0 = nullptr, *ones1 = nullptr;
  auto layout = [&](Carver ws, int64_t n_items) {
    w.txns = ws.take<lc_wr_txn>(nt);
    w.mops = ws.take<lc_wr_mop>(nm);
    w.mop_txn = ws.take<int32_t>(nm);
    zero0 = reinterpret_cast<char *>(ws.take<int64_t>(0));
    w.vnread = ws.take<int32_t>(vcap);
    w.vnrw = ws.take<int32_t>(vcap);
    w.vnchild = ws.take<int32_t>(vcap);
    w.rd_cur = ws.take<int32_t>(vcap);
    w.rc = ws.take<int64_t>(vcap + 1);
    w.item_off = ws.take<int64_t>(vcap + 1);
    w.kflags = ws.take<int32_t>(kcap);
    w.kcount = ws.take<int32_t>(3 * kcap);
    w.mop_last = ws.take<uint8_t>(nm);
    w.mop_flags = ws.take<int32_t>(nm);
    w.txn_flags = ws.take<int32_t>(nt);
    w.counters = ws.take<int64_t>(kCountersLen);
    d_count = ws.take<int64_t>(4);
    w.status = ws.take<int32_t>(4);
    l.vlocal = ws.take<int32_t>(vcap);
    l.kv = ws.take<int32_t>(kcap + 1);
    l.kwords = ws.take<int64_t>(kcap + 1);
    l.kntouch = ws.take<int32_t>(kcap + 1);
    l.knvedges = ws.take<int32_t>(kcap);
    l.kninit = ws.take<int32_t>(kcap);
    l.twfr = ws.take<uint8_t>(nm);
    l.npairs = ws.take<int64_t>(nm + 1);
    l.mat = ws.take<unsigned long long>(mat_words);
    zero1 = reinterpret_cast<char *>(ws.take<int64_t>(0));
    ones0 = zero1;
    w.vtab = ws.take<unsigned long long>(vcap);
    w.vwriter = ws.take<int32_t>(vcap);
    w.ptr_a = ws.take<int32_t>(vcap);  // (wr_txn_kernel notes its wfr parents there)
    w.ktab = ws.take<int64_t>(kcap);
    w.kcyc = ws.take<unsigned long long>(kcap);
    w.mop_par = ws.take<int32_t>(nm);  // (as ptr_a)
    ones1 = reinterpret_cast<char *>(ws.take<int64_t>(0));
    w.rd_off = ws.take<int32_t>(vcap + 1);
    w.readers = ws.take<int32_t>(nm);
    w.mop_kslot = ws.take<int32_t>(nm);
    w.mop_vslot = ws.take<int32_t>(nm);
    d_kslots = ws.take<int32_t>(kcap);
    w.keys = ws.take<lc_wr_key>(nm);
    l.kvoff = ws.take<int32_t>(kcap + 1);
    l.kmoff = ws.take<int64_t>(kcap + 1);
    l.ktoff = ws.take<int32_t>(kcap + 1);
    l.vlist = ws.take<int32_t>(nm);
    l.tkey = ws.take<unsigned long long>(nm);
    l.skey = ws.take<unsigned long long>(nm);
    l.pair_off = ws.take<int64_t>(nm + 1);
    for (int32_t **a : {&l.tidx, &l.sidx, &l.tcomp, &l.tfirst, &l.tlast, &l.s_comp, &l.s_first, &l.s_last, &l.r_ks,
                        &l.r_comp, &l.r_suf, &l.plo})
      *a = ws.take<int32_t>(nm);
    l.lin_keys = ws.take<lc_wr_lin_key>(nm);
    rt.carve(ws, nt);
    d_temp = ws.take<uint8_t>(temp_bytes);
    const size_t n_slots = nm + (size_t)n_items;
    w.slots = ws.take<lc_wr_edge>(n_slots);
    d_edges_b = ws.take<lc_wr_edge>(n_slots);
    d_etemp = ws.take<uint8_t>(lcwr::edge_temp_bytes((int64_t)n_slots));
    return ws.size;
  };
  auto first_run = [&](int64_t room) -> int {
    if (int e = ensure(c, s.arena, layout(Carver{}, room))) return e;
    layout(Carver{s.arena.p}, room);
    HIP_TRY(c, hipEventRecord(e0, st));
    HIP_TRY(c, hipMemcpyAsync(writable(w.txns), txns, sizeof(lc_wr_txn) * nt, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(writable(w.mops), mops, sizeof(lc_wr_mop) * nm, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipMemcpyAsync(writable(w.mop_txn), p.mop_txn.data(), sizeof(int32_t) * nm, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(e1, st));
    // nothing of an earlier call survives
    HIP_TRY(c, hipMemsetAsync(zero0, 0, (size_t)(zero1 - zero0), st));
    HIP_TRY(c, hipMemsetAsync(ones0, 0xFF, (size_t)(ones1 - ones0), st));
    HIP_TRY(c, hipMemsetAsync(w.slots, 0xFF, sizeof(lc_wr_edge) * nm, st));  // (the items' slots: once counted)
    HIP_TRY(c, hipEventRecord(k0, st));
    HIP_TRY(c, lcwr::launch_lin_rules(w, l, d_kslots, d_count + 3, d_temp, temp_bytes, l0, l1, st));
    HIP_TRY(c, lcwr::launch_real_time(w.txns, n_txns, p.n_ok, rt, d_count + 2, d_temp, temp_bytes, st));
    HIP_TRY(c, hipEventRecord(k1, st));
    HIP_TRY(c, hipMemcpyAsync(h.status, w.status, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h.count, d_count, sizeof(int64_t) * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(&h.items, w.item_off + vcap, sizeof(int64_t), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(h.counters, w.counters, sizeof(int64_t) * kCountersLen, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return 0;
  };
  if (nm == 0) {  // txns without mops: nothing for the lin kernels; the host code is the same answer
    return lc_wr_check_lin_host(txns, n_txns, mops, n_mops, flags, out, sum, lin_keys, lin_sum);
  }
  int64_t room = std::min<int64_t>(n_mops, std::max<int64_t>(lim.max_edges - n_mops, 0));
  if (int e = first_run(room)) return e;
  if (h.status[0]) {
    set_err(c, "lc_wr_check_lin: two writes of one (key, value) (mop " + std::to_string(h.status[1]) + " is one)");
    return -EINVAL;
  }
  if (h.status[2]) {
    set_err(c, "lc_wr_check_lin: a key with " + std::to_string(h.status[3]) + " versions, above lc_wr_lin_limits' " +
                   "max_key_versions (" + std::to_string(lcwr::kMaxKeyVersions) + ")");
    return -E2BIG;
  }
  const int64_t n_items = h.items, n_keys = h.count[3], max_versions = h.status[3];
  if (n_items < 0 || n_keys > n_mops) {
    set_err(c, "lc_wr_check_lin: inconsistent item or key count");
    return -EIO;
  }
  if (n_items > lim.max_edges - n_mops) {
    set_err(c, "lc_wr_check_lin: " + std::to_string(n_mops + n_items) +
                   " candidate edges exceed lc_wr_limits' max_edges (" + std::to_string(lim.max_edges) + ")");
    return -E2BIG;
  }
  if (n_items > room) {  // as wr_device: carved again in place, or the run made again in a larger arena
    if (layout(Carver{}, n_items) <= s.arena.cap) {
      layout(Carver{s.arena.p}, n_items);
    } else {
      if (int e = first_run(n_items)) return e;
      if (h.status[0] || h.status[2] || h.items != n_items) {
        set_err(c, "lc_wr_check_lin: the second run disagrees with the first");
        return -EIO;
      }
    }
  }
  const size_t n_slots = nm + (size_t)n_items;
  const size_t etemp_bytes = lcwr::edge_temp_bytes((int64_t)n_slots);
  h.count[1] = 0;
  HIP_TRY(c, hipEventRecord(k2, st));
  if (n_items) HIP_TRY(c, hipMemsetAsync(w.slots + nm, 0xFF, sizeof(lc_wr_edge) * (size_t)n_items, st));
  HIP_TRY(c, lcwr::launch_lin_items(w, l, n_items, st));
  HIP_TRY(c, lcwr::launch_edge_select(w.slots, (int64_t)n_slots, d_edges_b, d_count, d_etemp, etemp_bytes, st));
  HIP_TRY(c, hipMemcpyAsync(h.count, d_count, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int64_t n_sel = h.count[0];
  if (n_sel < 0 || n_sel > (int64_t)n_slots) {
    set_err(c, "lc_wr_check_lin: inconsistent edge count");
    return -EIO;
  }
  if (n_sel > 0) HIP_TRY(c, lcwr::launch_edge_sort(d_edges_b, w.slots, n_sel, d_count + 1, d_etemp, etemp_bytes, st));
  HIP_TRY(c, hipEventRecord(e2, st));
  if (n_sel > 0) HIP_TRY(c, hipMemcpyAsync(h.count + 1, d_count + 1, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  const int64_t n_edges = h.count[1];
  if (n_edges < 0 || n_edges > n_sel) {
    set_err(c, "lc_wr_check_lin: inconsistent unique edge count");
    return -EIO;
  }
  if (n_edges > out->edge_cap) {
    set_err(c, "lc_wr_check_lin: " + std::to_string(n_edges) + " edges, edge_cap " + std::to_string(out->edge_cap));
    if (sum) {
      *sum = lc_wr_summary{};
      sum->n_edges = n_edges;
      sum->n_edges_raw = n_sel;
    }
    return -ENOSPC;
  }
  HIP_TRY(c, hipMemcpyAsync(out->mop_flags, w.mop_flags, sizeof(int32_t) * nm, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->txn_flags, w.txn_flags, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  std::vector<lc_wr_key> keys((size_t)n_keys);
  std::vector<lc_wr_lin_key> lks((size_t)n_keys);
  if (n_keys) {
    HIP_TRY(c, hipMemcpyAsync(keys.data(), w.keys, sizeof(lc_wr_key) * (size_t)n_keys, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(lks.data(), l.lin_keys, sizeof(lc_wr_lin_key) * (size_t)n_keys, hipMemcpyDeviceToHost,
                              st));
  }
  if (p.n_ok) HIP_TRY(c, hipMemcpyAsync(out->byc, rt.byc, sizeof(int32_t) * (size_t)p.n_ok, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->rt_lo, rt.rt_lo, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(out->rt_hi, rt.rt_hi, sizeof(int32_t) * nt, hipMemcpyDeviceToHost, st));
  if (n_edges > 0)
    HIP_TRY(c, hipMemcpyAsync(out->edges, d_edges_b, sizeof(lc_wr_edge) * (size_t)n_edges, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  // both records ascending by key: the device wrote them in slot order
  std::vector<int32_t> order((size_t)n_keys);
  for (size_t i = 0; i < order.size(); i++) order[i] = (int32_t)i;
  std::sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return keys[(size_t)a].key < keys[(size_t)b].key; });
  lc_wr_lin_summary ls{};
  for (size_t i = 0; i < order.size(); i++) {
    out->keys[i] = keys[(size_t)order[i]];
    lin_keys[i] = lks[(size_t)order[i]];
    ls.n_touches += lin_keys[i].n_touches;
    ls.n_pairs += lin_keys[i].n_pairs;
    ls.n_vedges += lin_keys[i].n_vedges;
  }
  ls.max_key_versions = max_versions;
  int64_t counts[lcwr::kCounters];
  for (int b = 0; b < lcwr::kCounters; b++) counts[b] = lcwr::sum_counters(h.counters, b);
  lc_wr_summary sm;
  if (int e = lcwr::graph_and_summary(txns, n_txns, p, out, n_keys, n_edges, counts, &sm)) return e;
  sm.n_edges_raw = n_sel;
  sm.h2d_ms = elapsed_ms(e0, e1);
  sm.kernel_ms = elapsed_ms(k0, k1);
  sm.kernel_ms += elapsed_ms(k2, e2);
  ls.lin_kernel_ms = elapsed_ms(l0, l1);
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  if (lin_sum) *lin_sum = ls;
  return 0;
}

}  // namespace

extern "C" int lc_wr_check_lin(lc_ctx *c, const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops,
                               uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum, lc_wr_lin_key *lin_keys,
                               lc_wr_lin_summary *lin_sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_wr_check_lin", [&] {
    return wr_lin_device(c, txns, n_txns, mops, n_mops, flags, out, sum, lin_keys, lin_sum);
  });
}

extern "C" int lc_wr_check(lc_ctx *c, const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops, int64_t n_mops,
                           uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_wr_check",
                      [&] { return wr_device(c, txns, n_txns, mops, n_mops, flags, out, sum, nullptr); });
}

extern "C" int lc_wr_check_screened(lc_ctx *c, const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops,
                                    int64_t n_mops, uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum,
                                    lc_screen_summary *scr) {
  if (!c) return -EINVAL;
  lc_screen_summary local;
  return no_bad_alloc(c, "lc_wr_check_screened", [&] {
    return wr_device(c, txns, n_txns, mops, n_mops, flags, out, sum, scr ? scr : &local);
  });
}

extern "C" int lc_wr_check_restricted(lc_ctx *c, const lc_wr_txn *txns, int64_t n_txns, const lc_wr_mop *mops,
                                      int64_t n_mops, uint32_t flags, const lc_wr_out *out, lc_wr_summary *sum,
                                      lc_screen_summary *scr, lc_cycle_search_summary *srch) {
  if (!c) return -EINVAL;
  lc_screen_summary local;
  return no_bad_alloc(c, "lc_wr_check_restricted", [&] {
    return wr_device(c, txns, n_txns, mops, n_mops, flags, out, sum, scr ? scr : &local, srch, true);
  });
}
