// watch_dev.cpp — lc_watch_check's driver (include/lincheck_watch.h): the
// logs copied to the context's first device; the hashes, the exact compares,
// the forward passes and the backtracks there (watch.hip); between them the
// host's steps over the threads, which are few (watch_host.cpp): the class
// rounds, the canonical log, the batches, the deltas' order and the summary.
#include <algorithm>
#include <chrono>
#include <string>

#include "runtime.h"
#include "watch.h"

using namespace lcrt;

namespace {

int watch_device(lc_ctx *c, const lc_wt_thread *threads, int64_t n_threads, const int64_t *values, int64_t n_values,
                 int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out, lc_wt_summary *sum) {
  const auto t0 = std::chrono::steady_clock::now();
  const char *why = nullptr;
  if (lcwt::validate(threads, n_threads, values, n_values, n_nonmonotonic, flags, out, &why)) {
    set_err(c, std::string("lc_watch_check: ") + why);
    return -EINVAL;
  }
  if (n_threads < 2)  // nothing to compare
    return lc_watch_check_host(threads, n_threads, values, n_values, n_nonmonotonic, flags, out, sum);
  const lcwt::Limits lim = lcwt::limits();
  for (int64_t t = 0; t < n_threads; t++)
    if (threads[t].len > lcwt::kMaxDeviceLen) {
      set_err(c, "lc_watch_check: a log longer than lc_watch_limits' max_device_len");
      return -E2BIG;
    }
  const size_t nt = (size_t)n_threads, nv = (size_t)n_values;
  SideState &s = c->wts;
  hipStream_t st;
  if (int e = side_begin(c, s, 4, 0, &st)) return e;
  // e0 .. e1: the inputs' copies; k0 .. k1: around each run of kernels in turn
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], k0 = s.ev[2], k1 = s.ev[3];

  // The inputs and the threads' tables come first, so that the traces and the
  // edits, whose sizes the compares decide, move nothing when they are carved.
  int64_t *d_values = nullptr, *d_off = nullptr;
  int32_t *d_len = nullptr, *d_dist = nullptr, *d_trace = nullptr;
  lcwt::Hash *d_hash = nullptr;
  lcwt::Pair *d_pairs = nullptr;
  lcwt::PairRes *d_res = nullptr;
  lcwt::Item *d_items = nullptr;
  lc_wt_edit *d_edits = nullptr;
  size_t keep = 0;  // the bytes in front of the traces
  auto layout = [&](Carver ws, int64_t trace_entries, int64_t edit_entries) {
    d_values = ws.take<int64_t>(nv);
    d_off = ws.take<int64_t>(nt);
    d_len = ws.take<int32_t>(nt);
    d_hash = ws.take<lcwt::Hash>(nt);
    d_pairs = ws.take<lcwt::Pair>(nt);
    d_res = ws.take<lcwt::PairRes>(nt);
    d_items = ws.take<lcwt::Item>(nt);
    d_dist = ws.take<int32_t>(nt);
    keep = ws.size;
    d_trace = ws.take<int32_t>((size_t)trace_entries);
    d_edits = ws.take<lc_wt_edit>((size_t)edit_entries);
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}, 0, 0))) return e;
  layout(Carver{s.arena.p}, 0, 0);

  double kernel_ms = 0;
  std::vector<int64_t> h_off(nt);
  std::vector<int32_t> h_len(nt);
  for (size_t t = 0; t < nt; t++) {
    h_off[t] = threads[t].off;
    h_len[t] = (int32_t)threads[t].len;
  }
  HIP_TRY(c, hipEventRecord(e0, st));
  if (nv) HIP_TRY(c, hipMemcpyAsync(d_values, values, sizeof(int64_t) * nv, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_off, h_off.data(), sizeof(int64_t) * nt, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_len, h_len.data(), sizeof(int32_t) * nt, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipEventRecord(e1, st));

  // the hashes, which propose the classes
  std::vector<lcwt::Hash> hashes(nt);
  HIP_TRY(c, hipEventRecord(k0, st));
  HIP_TRY(c, lcwt::launch_hashes(d_values, d_off, d_len, (int)n_threads, d_hash, st));
  HIP_TRY(c, hipEventRecord(k1, st));
  HIP_TRY(c, hipMemcpyAsync(hashes.data(), d_hash, sizeof(lcwt::Hash) * nt, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  kernel_ms += elapsed_ms(k0, k1);
  const double h2d_ms = elapsed_ms(e0, e1);

  // One run of the compare kernel: log b of every pair against log a.
  std::vector<lcwt::Pair> h_pairs;
  std::vector<lcwt::PairRes> h_res;
  auto compare = [&](const std::vector<std::pair<int32_t, int32_t>> &ba) -> int {
    h_pairs.clear();
    for (const auto &pr : ba)
      h_pairs.push_back(lcwt::Pair{threads[pr.second].off, threads[pr.first].off, (int32_t)threads[pr.second].len,
                                   (int32_t)threads[pr.first].len});
    h_res.resize(h_pairs.size());
    HIP_TRY(c, hipMemcpyAsync(d_pairs, h_pairs.data(), sizeof(lcwt::Pair) * h_pairs.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(k0, st));
    HIP_TRY(c, lcwt::launch_compare(d_values, d_pairs, (int)h_pairs.size(), d_res, st));
    HIP_TRY(c, hipEventRecord(k1, st));
    HIP_TRY(c, hipMemcpyAsync(h_res.data(), d_res, sizeof(lcwt::PairRes) * h_res.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kernel_ms += elapsed_ms(k0, k1);
    return 0;
  };

  // rule 2: a round per representative that a group of one hash needs (one, without collisions)
  lcwt::ClassRounds cr;
  cr.init(threads, n_threads, hashes.data(), lim.mask, lim.mask_hi);
  while (!cr.pairs().empty()) {
    if (int e = compare(cr.pairs())) return e;
    std::vector<uint8_t> equal(h_res.size());
    for (size_t i = 0; i < h_res.size(); i++) equal[i] = h_res[i].p == h_pairs[i].a_len;  // (one length)
    cr.feed(equal);
  }
  int64_t size = 0, n_classes = 0;
  const int32_t canon = lcwt::pick_canonical(threads, n_threads, cr.cls, &size, &n_classes);

  // rule 4: every other class's threads against the canonical log
  std::vector<lcwt::Diff> diffs;
  std::vector<std::pair<int32_t, int32_t>> against;
  for (int64_t t = 0; t < n_threads; t++)
    if (cr.cls[(size_t)t] != canon) against.emplace_back((int32_t)t, canon);
  std::vector<lcwt::Item> h_items;
  if (!against.empty()) {
    if (int e = compare(against)) return e;
    const lc_wt_thread &A = threads[canon];
    for (size_t i = 0; i < against.size(); i++) {
      const lc_wt_thread &B = threads[against[i].first];
      const int64_t p = h_res[i].p, sfx = h_res[i].s;
      if (p < 0 || sfx < 0 || p + sfx > std::min(A.len, B.len) || (p + sfx == A.len && A.len == B.len)) {
        set_err(c, "lc_watch_check: inconsistent prefix or suffix");
        return -EIO;
      }
      diffs.push_back(lcwt::Diff{against[i].first, false, 0, p, sfx});
      lcwt::Item it{};
      it.a_off = A.off + p;
      it.b_off = B.off + p;
      it.base = p;
      it.n = (int32_t)(A.len - p - sfx);
      it.m = (int32_t)(B.len - p - sfx);
      it.dcap = (int32_t)std::min<int64_t>(lim.max_d, (int64_t)it.n + it.m);
      h_items.push_back(it);
    }
  }
  // The batches: threads in input order while their traces fit the budget, one
  // thread at least.  Offsets are the batch's own.
  const int64_t budget = lim.trace_bytes / (int64_t)sizeof(int32_t);
  std::vector<size_t> batch_end;
  int64_t max_trace = 0, max_edits = 0;
  for (size_t i = 0; i < h_items.size();) {
    int64_t tr = 0, ed = 0;
    size_t j = i;
    while (j < h_items.size() && (j == i || tr + lcwt::trace_entries(h_items[j].dcap) <= budget)) {
      h_items[j].trace_off = tr;
      h_items[j].edit_off = ed;
      tr += lcwt::trace_entries(h_items[j].dcap);
      ed += h_items[j].dcap;
      j++;
    }
    max_trace = std::max(max_trace, tr);
    max_edits = std::max(max_edits, ed);
    batch_end.push_back(j);
    i = j;
  }
  if (!h_items.empty()) {
    const size_t need = layout(Carver{}, max_trace, max_edits);
    if (need > s.arena.cap) {  // the arena grows; what lies in front of the traces moves along
      char *np = nullptr;
      if (hipMalloc(reinterpret_cast<void **>(&np), need) != hipSuccess) {
        set_err(c, "lc_watch_check: hipMalloc: out of device memory for the traces");
        return -ENOMEM;
      }
      hipError_t e = hipMemcpyAsync(np, s.arena.p, keep, hipMemcpyDeviceToDevice, st);
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) {
        (void)hipFree(np);
        set_err(c, std::string("lc_watch_check: moving the arena: ") + hipGetErrorString(e));
        return -EIO;
      }
      (void)hipFree(s.arena.p);
      s.arena.p = np;
      s.arena.cap = need;
    }
    layout(Carver{s.arena.p}, max_trace, max_edits);
  }
  // rule 5: forward, then — while the scripts so far fit the caller's room — backtrack
  std::vector<lc_wt_edit> staged;
  std::vector<int64_t> staged_off(h_items.size(), -1);
  std::vector<int32_t> h_dist(h_items.size());
  int64_t n_edits = 0;
  for (size_t bi = 0, i0 = 0; bi < batch_end.size(); i0 = batch_end[bi++]) {
    const size_t nb = batch_end[bi] - i0;
    HIP_TRY(c, hipMemcpyAsync(d_items, h_items.data() + i0, sizeof(lcwt::Item) * nb, hipMemcpyHostToDevice, st));
    HIP_TRY(c, hipEventRecord(k0, st));
    HIP_TRY(c, lcwt::launch_forward(d_values, d_items, (int)nb, d_trace, d_dist, st));
    HIP_TRY(c, hipEventRecord(k1, st));
    HIP_TRY(c, hipMemcpyAsync(h_dist.data() + i0, d_dist, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kernel_ms += elapsed_ms(k0, k1);
    for (size_t i = i0; i < i0 + nb; i++) {
      if (h_dist[i] > h_items[i].dcap || h_dist[i] < -1 || h_dist[i] == 0) {
        set_err(c, "lc_watch_check: inconsistent distance");
        return -EIO;
      }
      if (h_dist[i] > 0) n_edits += h_dist[i];
    }
    if (n_edits > out->edit_cap) continue;  // -ENOSPC below, once every distance is known
    HIP_TRY(c, hipEventRecord(k0, st));
    HIP_TRY(c, lcwt::launch_backtrack(d_values, d_items, (int)nb, d_trace, d_dist, d_edits, st));
    HIP_TRY(c, hipEventRecord(k1, st));
    for (size_t i = i0; i < i0 + nb; i++) {
      if (h_dist[i] <= 0) continue;
      staged_off[i] = (int64_t)staged.size();
      staged.resize(staged.size() + (size_t)h_dist[i]);
    }
    for (size_t i = i0; i < i0 + nb; i++)  // (staged no longer moves)
      if (h_dist[i] > 0)
        HIP_TRY(c, hipMemcpyAsync(staged.data() + staged_off[i], d_edits + h_items[i].edit_off,
                                  sizeof(lc_wt_edit) * (size_t)h_dist[i], hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    kernel_ms += elapsed_ms(k0, k1);
  }
  if (n_edits > out->edit_cap) {
    set_err(c, "lc_watch_check: " + std::to_string(n_edits) + " edits, edit_cap " + std::to_string(out->edit_cap));
    if (sum) {
      *sum = lc_wt_summary{};
      sum->n_edits = n_edits;
    }
    return -ENOSPC;
  }
  // rule 6: what stopped at max_d is the host's
  int64_t n_by_host = 0;
  for (size_t i = 0; i < h_items.size(); i++) {
    if (h_dist[i] > 0) {
      diffs[i].dist = h_dist[i];
      continue;
    }
    const lcwt::Item &it = h_items[i];
    diffs[i].no_script = true;
    diffs[i].dist = lcwt::myers_host(values + it.a_off, it.n, values + it.b_off, it.m, -1, 0, nullptr, nullptr);
    n_by_host++;
  }
  std::vector<int64_t> staged_by_thread(nt, -1);
  for (size_t i = 0; i < h_items.size(); i++) staged_by_thread[(size_t)diffs[i].thread] = staged_off[i];
  lc_wt_summary sm{};
  if (int e = lcwt::place_and_summarize(threads, n_threads, n_nonmonotonic, cr.cls, canon, size, n_classes,
                                        cr.n_collisions, &diffs, out, &sm)) {
    set_err(c, "lc_watch_check: the scripts' count changed");  // (their room was checked above)
    return e == -ENOSPC ? -EIO : e;
  }
  for (size_t i = 0; i < diffs.size(); i++) {
    const lc_wt_delta &d = out->deltas[i];
    if (d.script_len > 0)
      std::copy_n(staged.data() + staged_by_thread[(size_t)d.thread], (size_t)d.script_len, out->edits + d.script_off);
  }
  sm.n_by_host = n_by_host;
  sm.h2d_ms = h2d_ms;
  sm.kernel_ms = kernel_ms;
  sm.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (sum) *sum = sm;
  return 0;
}

}  // namespace

extern "C" int lc_watch_check(lc_ctx *c, const lc_wt_thread *threads, int64_t n_threads, const int64_t *values,
                              int64_t n_values, int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out,
                              lc_wt_summary *sum) {
  if (!c) return -EINVAL;
  return no_bad_alloc(c, "lc_watch_check", [&] {
    return watch_device(c, threads, n_threads, values, n_values, n_nonmonotonic, flags, out, sum);
  });
}
