// setfull_dev.cpp — lc_set_full's driver (include/lincheck_setfull.h): the
// arrays copied to the context's first device, the element table built, then
// one mark pass and one element pass per tile (setfull.hip).  The duplicates'
// multiplicities, where the device saw any, the summary and the verdict are
// the host's (setfull_host.cpp).
#include <algorithm>
#include <chrono>
#include <string>
#include <vector>

#include "runtime.h"
#include "setfull.h"
#include "txngraph.h"

using namespace lcrt;

namespace {

// one counter (the phantoms), sharded as the Elle checkers' are (sum_counters)
static_assert(lcsf::kCounterShards == lctg::kCounterShards && lcsf::kCounterStride == lctg::kCounterStride,
              "lc_set_full's counter geometry is txngraph.h's");
constexpr size_t kCountersLen = lcsf::kCounterShards * lcsf::kCounterStride;
struct Pinned {
  int32_t status[4];
  int64_t counters[kCountersLen];
};

int set_full_device(lc_ctx *c, const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads, int64_t n_reads,
                    const int64_t *read_values, int64_t n_values, int32_t linearizable, lc_sf_element *out,
                    lc_sf_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  const char *why = nullptr;
  if (lcsf::check_contract(adds, n_adds, reads, n_reads, read_values, n_values, &why)) {
    set_err(c, std::string("lc_set_full: ") + why);
    return -EINVAL;
  }
  if (n_adds > 0 && !out) {
    set_err(c, "lc_set_full: null out");
    return -EINVAL;
  }
  if (n_adds == 0 || n_reads == 0) {  // nothing for the device to do
    const int rc = lc_set_full_host(adds, n_adds, reads, n_reads, read_values, n_values, linearizable, out, sum);
    if (rc == -EINVAL) set_err(c, "lc_set_full: two adds of one value");
    return rc;
  }
  SideState &s = c->sfs;
  hipStream_t st;
  if (int e = side_begin(c, s, 3, sizeof(Pinned), &st)) return e;
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], e2 = s.ev[2];  // the inputs' copies, then the kernels
  Pinned &h = *s.words<Pinned>();
  lc_sf_limit_info lim;
  lc_set_full_limits(&lim);
  const size_t ne = (size_t)n_adds, nr = (size_t)n_reads;
  const int64_t wpr = (n_reads + 31) / 32;
  int64_t tile_rows = lim.tile_bytes / (wpr * 4);  // a tile holds at least one row
  tile_rows = std::max<int64_t>(1, std::min(tile_rows, n_adds));
  const int64_t n_tiles = (n_adds + tile_rows - 1) / tile_rows;
  const uint64_t cap = lcsf::table_capacity(n_adds);
  std::vector<int64_t> work_off(nr + 1);
  work_off[0] = 0;
  for (size_t r = 0; r < nr; r++) work_off[r + 1] = work_off[r] + reads[r].len;
  lcsf::Ws w{};
  w.n_adds = n_adds;
  w.n_reads = n_reads;
  w.n_work = work_off[nr];
  w.cap = cap;
  w.wpr = wpr;
  auto layout = [&](Carver ws) {
    w.adds = ws.take<lc_sf_add>(ne);
    w.reads = ws.take<lc_sf_read>(nr);
    w.values = ws.take<int64_t>((size_t)n_values);
    w.work_off = ws.take<int64_t>(nr + 1);
    w.tab_key = ws.take<int64_t>(cap);
    w.tab_ent = ws.take<lcsf::Ent>(cap);
    w.r_inv = ws.take<int32_t>(nr);
    w.r_ok = ws.take<int32_t>(nr);
    w.bitmap = ws.take<uint32_t>((size_t)(tile_rows * wpr));
    w.dup_seen = ws.take<uint8_t>(ne);
    w.counters = ws.take<int64_t>(kCountersLen);
    w.status = ws.take<int32_t>(4);
    w.out = ws.take<lc_sf_element>(ne);
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}))) return e;
  layout(Carver{s.arena.p});
  HIP_TRY(c, hipEventRecord(e0, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.adds), adds, sizeof(lc_sf_add) * ne, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.reads), reads, sizeof(lc_sf_read) * nr, hipMemcpyHostToDevice, st));
  if (n_values)
    HIP_TRY(c, hipMemcpyAsync(writable(w.values), read_values, sizeof(int64_t) * (size_t)n_values,
                              hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(writable(w.work_off), work_off.data(), sizeof(int64_t) * (nr + 1),
                            hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipEventRecord(e1, st));
  // no counter or mark of an earlier call survives
  HIP_TRY(c, hipMemsetAsync(w.counters, 0, sizeof(int64_t) * kCountersLen, st));
  HIP_TRY(c, hipMemsetAsync(w.status, 0, sizeof(int32_t) * 4, st));
  HIP_TRY(c, hipMemsetAsync(w.dup_seen, 0, ne, st));
  HIP_TRY(c, lcsf::launch_table(w, st));
  for (int64_t r0 = 0; r0 < n_adds; r0 += tile_rows)
    HIP_TRY(c, lcsf::launch_tile(w, r0, std::min(r0 + tile_rows, n_adds), st));
  HIP_TRY(c, hipEventRecord(e2, st));
  HIP_TRY(c, hipMemcpyAsync(h.status, w.status, sizeof(int32_t) * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(h.counters, w.counters, sizeof(int64_t) * kCountersLen, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  if (h.status[0]) {
    set_err(c, "lc_set_full: two adds of one value (element " + std::to_string(h.status[1]) + " is one)");
    return -EINVAL;
  }
  HIP_TRY(c, hipMemcpyAsync(out, w.out, sizeof(lc_sf_element) * ne, hipMemcpyDeviceToHost, st));
  std::vector<uint8_t> marked;
  if (h.status[2]) {
    marked.resize(ne);
    HIP_TRY(c, hipMemcpyAsync(marked.data(), w.dup_seen, ne, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  // duplicates, exact but not fast: the multiplicities of the marked elements
  // in one pass over the payload (a history without duplicates never takes it)
  if (h.status[2])
    if (int rc = lcsf::count_duplicates(adds, n_adds, reads, n_reads, read_values, marked.data(), out)) return rc;
  if (sum) {
    lcsf::summarize(out, n_adds, linearizable, sum);
    sum->n_phantom = lctg::sum_counters(h.counters, 0);
    sum->n_tiles = n_tiles;
    sum->h2d_ms = elapsed_ms(e0, e1);
    sum->kernel_ms = elapsed_ms(e1, e2);
    sum->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  return 0;
}

}  // namespace

extern "C" int lc_set_full(lc_ctx *c, const lc_sf_add *adds, int64_t n_adds, const lc_sf_read *reads,
                           int64_t n_reads, const int64_t *read_values, int64_t n_values, int32_t linearizable,
                           lc_sf_element *out, lc_sf_summary *sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_set_full", [&] {
    return set_full_device(c, adds, n_adds, reads, n_reads, read_values, n_values, linearizable, out, sum);
  });
}
