// frontiers_dev.cpp — lc_check_frontiers (include/lincheck_fx.h) and
// lc_check_frontiers_counted (include/lincheck_counted.h): the frontier of
// every key just before one of its returns, dumped by the search tiers'
// kernels on the context's first device.  Both begin as the side checkers do
// (side_begin): a live resident grid leaves before their work runs.  Their
// scratch is the context's lc_check buffers (a context is not re-entrant).
#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "runtime.h"

using namespace lcrt;

namespace {

// The argument checks lc_check_frontiers and lc_check_frontiers_counted
// share (`bad`: the call's own buffer and size test).
int frontier_args(lc_ctx *c, const char *fn, bool bad, const int64_t *key_off, int64_t n_keys) {
  if (bad) {
    set_err(c, std::string(fn) + ": null buffer, negative n_keys or max_per_key < 1");
    return -EINVAL;
  }
  return n_keys == 0 ? 0 : check_offsets(c, fn, key_off, n_keys);
}

// Their inputs on the context's first GPU: the records in d_ops, the offsets
// and the stops in d_off (stops at d_off + n_keys + 1), through the staging
// buffer when pageable and small (as lc_check's); d_status zeroed.
int frontier_upload(lc_ctx *c, Dev &d, const lc_op *ops, const int64_t *key_off, int64_t n_keys,
                    const int64_t *stop_op) {
  const int64_t r0 = key_off[0], nrec = key_off[n_keys] - r0;
  int e = ensure(c, d.d_ops, sizeof(lc_op) * (size_t)nrec);
  if (!e) e = ensure(c, d.d_off, sizeof(int64_t) * (size_t)(2 * n_keys + 1));
  if (e) return e;
  int64_t *d_off = d.d_off.p, *d_stop = d_off + (n_keys + 1);
  hipStream_t st = d.stream;
  const void *src_ops = ops + r0, *src_off = key_off, *src_stop = stop_op;
  const size_t ops_b = sizeof(lc_op) * (size_t)nrec, off_b = sizeof(int64_t) * (size_t)(n_keys + 1),
               stop_b = sizeof(int64_t) * (size_t)n_keys;
  if (ops_b + off_b + stop_b + 512 <= kStageMax && !is_pinned(c, ops + r0, ops_b)) {
    char *sb = stage_buf(c, d);
    if (!sb) return -ENOMEM;
    char *so = sb, *sf = so + up256(ops_b), *ss = sf + up256(off_b);
    std::memcpy(so, src_ops, ops_b);
    std::memcpy(sf, src_off, off_b);
    std::memcpy(ss, src_stop, stop_b);
    src_ops = so;
    src_off = sf;
    src_stop = ss;
  }
  HIP_TRY(c, hipMemcpyAsync(d.d_ops.p, src_ops, ops_b, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_off, src_off, off_b, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemcpyAsync(d_stop, src_stop, stop_b, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipMemsetAsync(d.d_status, 0, sizeof(lcdev::KStatus), st));
  d.status_dirty = true;
  return 0;
}

// lc_check_frontiers_counted behind its argument checks.
int frontiers_counted(lc_ctx *c, const lc_op *ops, const int64_t *key_off, int64_t n_keys,
                      const int64_t *stop_op, const lcdev::KParams &p, lc_counted_config *out,
                      int32_t max_per_key, int32_t *n_out, int64_t *n_total, int64_t *pending) {
  const int64_t r0 = key_off[0];
  // the keys the device may search (the others: -1)
  std::vector<CountedKey> keys((size_t)n_keys);
  std::vector<int32_t> list;
  for (int64_t k = 0; k < n_keys; k++) {
    n_out[k] = -1;
    n_total[k] = -1;
    keys[k] = counted_classes_of(ops + key_off[k], key_off[k + 1] - key_off[k], stop_op[k]);
    if (keys[k].take) list.push_back((int32_t)k);
  }
  int32_t n_list = (int32_t)list.size();
  if (n_list == 0) return 0;
  hipStream_t st;
  if (int e = side_begin(c, &st)) return e;
  Dev &d = c->devs[0];
  // scratch: the compact configurations, then every key's tables, in d_gws
  const size_t cfg_bytes = sizeof(lcdev::CountedCfg) * (size_t)max_per_key * (size_t)n_keys;
  const size_t key_bytes = sizeof(lcdev::CountedKeyOut) * (size_t)n_keys;
  int e = ensure(c, d.d_gws, cfg_bytes + key_bytes);
  if (!e) e = ensure(c, d.d_jit, sizeof(int32_t) * (size_t)n_keys);
  if (!e) e = ensure(c, d.d_jit2, sizeof(int32_t) * (size_t)n_keys);
  if (!e) e = frontier_upload(c, d, ops, key_off, n_keys, stop_op);
  if (e) return e;
  int64_t *d_off = d.d_off.p, *d_stop = d_off + (n_keys + 1);
  int32_t *d_list = d.d_jit.p, *d_next = d.d_jit2.p;
  lcdev::CountedCfg *d_cfg = reinterpret_cast<lcdev::CountedCfg *>(d.d_gws.p);
  lcdev::CountedKeyOut *d_key = reinterpret_cast<lcdev::CountedKeyOut *>(
      reinterpret_cast<char *>(d.d_gws.p) + cfg_bytes);
  HIP_TRY(c, hipMemcpyAsync(d_list, list.data(), sizeof(int32_t) * (size_t)n_list,
                            hipMemcpyHostToDevice, st));
  // counted_tier's ladder of set capacities
  const int by_value = !env_is_off("LC_COUNTED_BY_VALUE");
  for (int tier = 0; tier < kHbmTiers && n_list > 0; tier++) {
    const int waves = std::min<int>(kHbmWaves[tier], n_list);
    if ((e = ensure(c, d.d_ws, lcdev::hbm_tier_ws_bytes(waves, kHbmCap[tier])))) return e;
    if (tier > 0) {
      HIP_TRY(c, hipMemsetAsync(&d.d_status->n_overflow2, 0, sizeof(int32_t), st));
      HIP_TRY(c, hipMemsetAsync(&d.d_status->hbm_next, 0, sizeof(int32_t), st));
    }
    HIP_TRY(c, lcdev::launch_counted_frontier(d.d_ops.p, d_off, d_stop, d_list, n_list, p, d.d_ws.p,
                                              waves, kHbmCap[tier], d_cfg, max_per_key, d_key, d_next,
                                              &d.d_status->n_overflow2, &d.d_status->hbm_next,
                                              tier == kHbmTiers - 1, by_value, st));
    if ((e = read_status(c, d, st))) return e;
    n_list = tier < kHbmTiers - 1 ? d.h_status->n_overflow2 : 0;
    std::swap(d_list, d_next);
  }
  std::vector<lcdev::CountedCfg> cfg((size_t)max_per_key * (size_t)n_keys);
  std::vector<lcdev::CountedKeyOut> kout((size_t)n_keys);
  HIP_TRY(c, hipMemsetAsync(d.d_status, 0, sizeof(lcdev::KStatus), st));
  HIP_TRY(c, hipMemcpyAsync(cfg.data(), d_cfg, cfg_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(kout.data(), d_key, key_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  d.status_dirty = false;
  // Expansion to record indices: the pending window slots through the key's
  // slot table; of class c, members [linearized, called) — deadline order
  // linearizes a class's crashed members in call order, which is record order.
  std::vector<int64_t> pend;
  for (const int32_t k : list) {
    const lcdev::CountedKeyOut &ko = kout[k];
    const CountedKey &ck = keys[k];
    const int64_t n_k = key_off[k + 1] - key_off[k];
    bool ok = ko.n >= -1 && ko.n <= max_per_key && ko.total >= ko.n &&
              (ko.n <= 0 || ko.n_classes == (int32_t)ck.members.size());
    for (int32_t j = 0; ok && j < ko.n; j++) {
      const lcdev::CountedCfg &g = cfg[(size_t)k * max_per_key + j];
      pend.clear();
      uint64_t slots = g.word;
      for (size_t ci = 0; ci < ck.members.size(); ci++) {
        const uint64_t field = ((1ull << ko.width[ci]) - 1) << ko.shift[ci];
        const int64_t lin = (int64_t)((g.word & field) >> ko.shift[ci]), called = ko.called[ci];
        slots &= ~field;
        ok = ok && lin <= called && called <= (int64_t)ck.members[ci].size();
        for (int64_t m = lin; ok && m < called; m++) pend.push_back(ck.members[ci][m]);
      }
      for (; ok && slots; slots &= slots - 1) {
        const int32_t rec = ko.slot_rec[__builtin_ctzll(slots)];
        ok = rec >= 0 && rec < n_k;
        pend.push_back(rec);
      }
      if (!ok) break;
      std::sort(pend.begin(), pend.end());
      lc_counted_config &o = out[(size_t)k * max_per_key + j];
      o.version = g.version;
      o.value = g.value;
      o.n_pending = (int64_t)pend.size();
      o.pending_at = (int64_t)max_per_key * (key_off[k] - r0) + (int64_t)j * n_k;
      ok = o.n_pending <= n_k;
      if (ok) std::copy(pend.begin(), pend.end(), pending + o.pending_at);
    }
    if (!ok) {  // (the device's tables and the host's classes disagree: a bug, not an input)
      set_err(c, "lc_check_frontiers_counted: inconsistent frontier of key " + std::to_string(k));
      return -EIO;
    }
    n_out[k] = ko.n;
    n_total[k] = ko.total;
  }
  return 0;
}

}  // namespace

extern "C" {

int lc_check_frontiers(lc_ctx *c, const lc_op *ops, const int64_t *key_off, int64_t n_keys,
                       const int64_t *stop_op, const lc_opts *opts, lc_fx_config *out,
                       int32_t max_per_key, int32_t *n_out) {
  if (!c) return -EINVAL;
  if (int rc = frontier_args(c, "lc_check_frontiers",
                             n_keys < 0 || max_per_key < 1 ||
                                 (n_keys > 0 && (!ops || !key_off || !stop_op || !out || !n_out)),
                             key_off, n_keys))
    return rc;
  if (n_keys == 0) return 0;
  lcdev::KParams p;
  if (int rc = opts_to_params(c, opts, &p)) return rc;
  hipStream_t st;
  if (int rc = side_begin(c, &st)) return rc;
  Dev &d = c->devs[0];
  const size_t cfg_bytes = sizeof(lc_fx_config) * (size_t)max_per_key * (size_t)n_keys;
  int e = ensure(c, d.d_gws, cfg_bytes);
  if (!e) e = ensure(c, d.d_jit, sizeof(int32_t) * (size_t)n_keys);
  if (!e) e = ensure(c, d.d_jit2, sizeof(int32_t) * (size_t)n_keys);
  if (!e) e = frontier_upload(c, d, ops, key_off, n_keys, stop_op);
  if (e) return e;
  int64_t *d_off = d.d_off.p, *d_stop = d_off + (n_keys + 1);
  int32_t *d_n = d.d_jit.p, *d_retry = d.d_jit2.p;
  lc_fx_config *d_cfg = reinterpret_cast<lc_fx_config *>(d.d_gws.p);
  const lc_op *d_ops = d.d_ops.p;
  HIP_TRY(c, lcdev::launch_frontier_dump(d_ops, d_off, d_stop, n_keys, p, d_cfg, max_per_key, d_n,
                                         d_retry, &d.d_status->n_overflow, st));
  if ((e = read_status(c, d, st))) return e;
  // keys whose search outgrew the LDS regions: again over HBM tables (the
  // first HBM tier's 16k configurations per set), one wavefront per key
  if (const int32_t n_retry = d.h_status->n_overflow) {
    const int waves = std::min<int>(n_retry, 256);
    if ((e = ensure(c, d.d_ws, lcdev::hbm_tier_ws_bytes(waves, kHbmCap[0])))) return e;
    HIP_TRY(c, lcdev::launch_frontier_dump_hbm(d_ops, d_off, d_stop, d_retry, n_retry, p, d.d_ws.p, waves,
                                               kHbmCap[0], d_cfg, max_per_key, d_n,
                                               &d.d_status->hbm_next, st));
  }
  HIP_TRY(c, hipMemsetAsync(d.d_status, 0, sizeof(lcdev::KStatus), st));
  HIP_TRY(c, hipMemcpyAsync(n_out, d_n, sizeof(int32_t) * (size_t)n_keys, hipMemcpyDeviceToHost, st));
  // one copy of every key's slots (C5's 94 keys x 10: 0.5 MB) rather than one
  // per key; slots past a key's count keep the device's scratch
  HIP_TRY(c, hipMemcpyAsync(out, d_cfg, cfg_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  d.status_dirty = false;
  return 0;
}

int lc_check_frontiers_counted(lc_ctx *c, const lc_op *ops, const int64_t *key_off, int64_t n_keys,
                               const int64_t *stop_op, const lc_opts *opts, lc_counted_config *out,
                               int32_t max_per_key, int32_t *n_out, int64_t *n_total,
                               int64_t *pending, int64_t pending_cap) {
  if (!c) return -EINVAL;
  if (int rc = frontier_args(c, "lc_check_frontiers_counted",
                             n_keys < 0 || max_per_key < 1 ||
                                 (n_keys > 0 && (!ops || !key_off || !stop_op || !out || !n_out ||
                                                 !n_total || !pending)),
                             key_off, n_keys))
    return rc;
  if (n_keys == 0) return 0;
  if (n_keys > INT32_MAX) {  // (the device's key lists are int32)
    set_err(c, "lc_check_frontiers_counted: more than 2^31 - 1 keys");
    return -EINVAL;
  }
  const int64_t r0 = key_off[0], nrec = key_off[n_keys] - r0;
  if (nrec > INT64_MAX / max_per_key || pending_cap < (int64_t)max_per_key * nrec) {
    set_err(c, "lc_check_frontiers_counted: pending_cap " + std::to_string(pending_cap) +
                   " is less than max_per_key * records");
    return -EINVAL;
  }
  lcdev::KParams p;
  if (int rc = opts_to_params(c, opts, &p)) return rc;
  try {
    return frontiers_counted(c, ops, key_off, n_keys, stop_op, p, out, max_per_key, n_out, n_total,
                             pending);
  } catch (const std::bad_alloc &) {  // (the host's tables: sized by the caller's arguments)
    set_err(c, "lc_check_frontiers_counted: out of host memory");
    return -ENOMEM;
  }
}

}  // extern "C"
