// whole_gpu.cpp — LC_FLAG_WHOLE_GPU: keys the tiers left :unknown at the
// configuration budget (one workgroup's HBM sets were not enough) are
// searched again by the frontier exchange (include/lincheck_fx.h), whose
// budget bounds each return's configuration sets, as the oracle's does; its
// result replaces the tiers' (verdict, fail op, explored, frontier).
// fetch(k, records) and store(k, result) move a key between the caller's
// memory (host or device) and the engine.
//
// * Fewer such keys than the context has GPUs: each key's search spans every
//   GPU of the context — one rank per GPU over RCCL (lc_fx_open_devices),
//   the frontier partitioned by hash owner while it is large.
//   Device contexts that share one GPU (LC_VIRTUAL_DEVICES) run their ranks
//   in process instead (RCCL refuses two ranks on one device).
// * Otherwise keys are independent (register.clj:108): up to kFxEngines
//   single-GPU engines per GPU search different keys at once (one key's
//   levels are latency-bound, so concurrent searches fill a GPU the way one
//   cannot), as many as the GPU's free memory holds.
//
// Keys left :unknown because more than LC_MAX_WINDOW ops were open at once
// (crashed writes/CAS pile up in the tiers' windows) are searched again too,
// the same way: there the crashed ops of a key are counted per class instead
// of holding a window slot each (fx.hip, "Counted classes"; owner_of hashes a
// class by its absolute count, so the multi-GPU engine partitions them too).
//
// A failure of the re-search (an allocation, say) is this key's alone: it
// keeps the tiers' :unknown, the error text goes to lc_last_error, and the
// call still succeeds — as jepsen.independent loses only the key whose check
// throws.
#include <algorithm>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "runtime.h"

using namespace lcrt;

namespace {
constexpr size_t kFxEngines = 4;  // oversized keys searched at once
}

int lcrt::whole_gpu(lc_ctx *c, const std::vector<int64_t> &todo, const lc_opts *opts,
                    const std::function<int(int64_t, std::vector<lc_op> &)> &fetch,
                    const std::function<int(int64_t, const lc_key_result &)> &store) {
  if (todo.empty()) return 0;
  std::vector<int> ids;  // the context's distinct GPUs
  for (const Dev &d : c->devs)
    if (std::find(ids.begin(), ids.end(), d.id) == ids.end()) ids.push_back(d.id);
  const int nranks = (int)c->devs.size();
  std::atomic<int> failed{0};
  auto note = [&](int64_t k, const std::string &what) {
    failed++;
    set_err(c, "LC_FLAG_WHOLE_GPU: key " + std::to_string(k) + " kept :unknown: " + what);
  };
  if (nranks > 1 && todo.size() < (size_t)nranks) {
    if (!c->fx_all && !c->fx_all_failed) {
      lc_fx_params fp{};
      fp.part_above = -1;
      fp.repl_below = -1;
      int e;
      if ((int)ids.size() == nranks) {
        e = lc_fx_open_devices(&fp, ids.data(), (int32_t)ids.size(), &c->fx_all);
      } else {
        fp.device = ids[0];
        fp.virtual_ranks = nranks;
        e = lc_fx_open(&fp, nullptr, &c->fx_all);
      }
      if (e) {
        c->fx_all = nullptr;
        c->fx_all_failed = true;  // (e.g. no librccl) the single-GPU engines below take over
        set_err(c, "LC_FLAG_WHOLE_GPU: multi-GPU frontier exchange unavailable (" +
                       std::to_string(e) + "); searching keys one GPU each");
      }
    }
    if (c->fx_all) {
      std::vector<lc_op> recs;
      for (int64_t k : todo) {
        if (int x = fetch(k, recs)) return x;
        lc_key_result r;
        if (int x = lc_fx_check(c->fx_all, recs.data(), (int64_t)recs.size(), opts, &r)) {
          note(k, std::string("lc_fx_check: ") + lc_fx_last_error(c->fx_all) + " (" +
                      std::to_string(x) + ")");
          continue;
        }
        if (int x = store(k, r)) return x;
      }
      return 0;
    }
  }
  // key-parallel: engines per GPU, bounded by its free memory (lists and
  // tables take up to ~352 B per configuration of the budget, two one-word table sets included)
  const int64_t budget = opts && opts->max_configs_per_key > 0 ? opts->max_configs_per_key
                                                                : kDefaultBudget;
  const double per_engine = 352.0 * (double)(budget + 1) + (64 << 20);
  for (int id : ids) {
    int have = 0;
    for (const auto &e : c->fxs) have += e.second == id;
    size_t fr = 0, tot = 0;
    (void)hipSetDevice(id);
    int want = (int)kFxEngines;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess)
      want = (int)std::max<double>(1.0, std::min<double>(want, 0.8 * (double)fr / per_engine + have));
    const int per_dev = (int)std::min<size_t>((size_t)want, (todo.size() + ids.size() - 1) / ids.size());
    for (; have < per_dev; have++) {
      lc_fx_params fp{};
      fp.device = id;
      fp.virtual_ranks = 1;
      fp.part_above = -1;
      fp.repl_below = -1;
      lc_fx *f = nullptr;
      if (int e = lc_fx_open(&fp, nullptr, &f)) {
        set_err(c, "LC_FLAG_WHOLE_GPU: lc_fx_open failed (" + std::to_string(e) + ")");
        break;
      }
      c->fxs.emplace_back(f, id);
    }
  }
  const int ne = (int)c->fxs.size();
  if (ne == 0) {
    for (int64_t k : todo) note(k, "no frontier-exchange engine could be opened");
    return 0;
  }
  std::atomic<size_t> next{0};
  std::vector<int> erc(ne, 0);
  auto run = [&](int e) {
    (void)hipSetDevice(c->fxs[e].second);
    std::vector<lc_op> recs;
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= todo.size()) break;
      const int64_t k = todo[i];
      lc_key_result r;
      if ((erc[e] = fetch(k, recs))) break;
      if (int x = lc_fx_check(c->fxs[e].first, recs.data(), (int64_t)recs.size(), opts, &r)) {
        note(k, std::string("lc_fx_check: ") + lc_fx_last_error(c->fxs[e].first) + " (" +
                    std::to_string(x) + ")");
        continue;
      }
      if ((erc[e] = store(k, r))) break;
    }
  };
  std::vector<std::thread> th;
  for (int e = 0; e < std::min<int>(ne, (int)todo.size()); e++) th.emplace_back(run, e);
  for (auto &t : th) t.join();
  for (int e = 0; e < ne; e++)
    if (erc[e]) return erc[e];
  return 0;
}

// The keys the tiers left :unknown at the configuration budget, and those
// with more than LC_MAX_WINDOW ops open at once.
void lcrt::unknown_keys(const lc_key_result *res, int64_t n_keys, std::vector<int64_t> &budget,
                        std::vector<int64_t> &window) {
  for (int64_t k = 0; k < n_keys; k++)
    if (res[k].verdict == LC_UNKNOWN && res[k].reason == LC_REASON_CONFIG_BUDGET) budget.push_back(k);
    else if (res[k].verdict == LC_UNKNOWN && res[k].reason == LC_REASON_WINDOW_OVERFLOW)
      window.push_back(k);
}

// LC_FLAG_WHOLE_GPU after a device call: the results and the keys' records
// are in device memory: read back the verdicts, and each key the frontier
// exchange takes.  d_cert: the call's certificates (null: none wanted).
int lcrt::whole_gpu_device(lc_ctx *c, const lc_op *d_ops, const int64_t *d_key_off, int64_t n_keys,
                           const lc_opts *opts, lc_key_result *d_out, int32_t *d_cert, hipStream_t st) {
  std::vector<lc_key_result> res((size_t)n_keys);
  int64_t base = 0;
  HIP_TRY(c, hipMemcpyAsync(res.data(), d_out, sizeof(lc_key_result) * (size_t)n_keys,
                            hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&base, d_key_off, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  std::vector<int64_t> todo, todo_w;
  unknown_keys(res.data(), n_keys, todo, todo_w);
  auto fetch = [&](int64_t k, std::vector<lc_op> &v) {
    int64_t se[2];
    if (hipMemcpy(se, d_key_off + k, sizeof se, hipMemcpyDeviceToHost) != hipSuccess) return -EIO;
    v.resize((size_t)(se[1] - se[0]));
    if (!v.empty() && hipMemcpy(v.data(), d_ops + (se[0] - base), sizeof(lc_op) * v.size(),
                                hipMemcpyDeviceToHost) != hipSuccess)
      return -EIO;
    return 0;
  };
  auto store = [&](int64_t k, const lc_key_result &r) {
    if (d_cert) {
      const int32_t none[4] = {LC_CERT_NONE, -1, -1, 0};
      if (hipMemcpy(d_cert + 4 * k, none, sizeof none, hipMemcpyHostToDevice) != hipSuccess) return -EIO;
    }
    return hipMemcpy(d_out + k, &r, sizeof r, hipMemcpyHostToDevice) == hipSuccess ? 0 : -EIO;
  };
  int rc = whole_gpu(c, todo, opts, fetch, store);
  if (!rc) rc = whole_gpu(c, todo_w, opts, fetch, store);
  return rc;
}
