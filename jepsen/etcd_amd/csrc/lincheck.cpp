// lincheck.cpp — host runtime behind include/lincheck.h.
//
// Replaces, as one unit, the checker built at
//   /root/reference/src/jepsen/etcd/register.clj:108-112
// (independent/checker over checker/linearizable with VersionedRegister).
// jepsen.independent checks keys concurrently on a bounded JVM thread pool;
// here all keys of a call go to the GPUs in one batch: contiguous,
// cost-balanced key ranges per device (one host thread + one HIP stream per
// device).  Per device: the version-order tier over every key (one launch,
// one sync when it decides them all), then the JIT-search tier over the keys
// it hands over, then HBM-tier re-runs of the few keys whose frontier outgrew
// LDS.  No collective is needed: keys are independent and results land in
// the caller's array.  There is no CPU fallback: without a usable GPU lc_open
// fails with -ENODEV.
//
// This file is the context and the device side of the register path: the
// tiers over keys whose arrays are on a device (run_device) and
// lc_check_device.  lc_check from host memory is check_host.cpp, the
// frontier calls frontiers_dev.cpp, LC_FLAG_WHOLE_GPU whole_gpu.cpp, the
// planners and packers plan_host.cpp (plain C++); the side checkers
// (lc_check_events, lc_set_full, lc_append_check) have their drivers in
// *_dev.cpp.  runtime.h is what all of those share with this file.
#include <errno.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "runtime.h"

#ifndef LC_BUILD_ID
#define LC_BUILD_ID "unknown"
#endif

using namespace lcrt;

namespace {

// Timing events.  hipEventDisableSystemFence skips
// the event's own system-scope fence (cache writeback + invalidate) when it
// is recorded; kernel completion already releases the kernel's writes to
// device memory, and the one host-visible word the host reads after such an
// event (h_handoff) is made visible by its writer with a system-scope fence
// (fast_tier_handoff, check_kernel.hip).
constexpr unsigned kEventFlags = hipEventDisableSystemFence;
// LC_FLAG_SEARCH_WITNESS: the witness search's workspace at most (512 KB of
// cache per wave, 49 B per record of the longest listed key)
constexpr size_t kWitnessWsBytes = size_t(2) << 30;
// HBM tier lists up to these sizes get a workgroup of 16 (4) wavefronts per
// key; longer lists a wavefront per key.  Measured (tools/hbm_probe.py,
// DESIGN.md §4): 16 wins on 512 crash-heavy keys (4.9 s vs 13.1 s with 4,
// 40 s with 1), 4 on 1000-2000 version-less keys (71 vs 113 vs 119 ms),
// 1 on 10,000 (331 vs 355 ms with 4).
// 8-wave workgroups (two per CU) up to 512 keys, 4-wave ones beyond: version-
// less 1,000-op keys at concurrency 20 (tools/coop8_ab.py), HBM tier ms:
//   keys        64    256    400    512    700   1000
//   4 waves   11.6   11.8   12.0   12.1   12.7   13.5
//   8 waves    9.1    9.1    9.2    9.4   15.3   18.0
//   16 waves   9.0    9.1   14.6   16.4   21.6   30.0
constexpr int kHbmCoop8MaxKeys = 512;
constexpr int kHbmCoop16Resident = 256;   // 16-wave workgroups resident: one per CU
constexpr int kHbmCoop4Resident = 1024;   // 4-wave workgroups: four per CU (LDS tables)
constexpr int kJitDirectMaxKeys = 1024;  // 4 cooperative workgroups per CU x 256 CUs
// Gap tier: at most this many workgroups, and this much workspace (each
// workgroup needs 92 B per record of the longest key handed over).  Dynamic
// LDS for the matching arrays: up to kGapLdsFull per workgroup for whole-key
// decisions (occupancy), up to kGapLdsProbe for counterexample probes.
constexpr int kGapMaxWG = 1024;
constexpr size_t kGapWsBytes = size_t(1) << 30;
constexpr int kGapLdsFull = 48 << 10;
// few keys (at most this many workgroups): occupancy does not matter, so a
// whole-key decision may hold a large matching in LDS (gfx950: 160 KB per CU)
constexpr int kGapLdsFew = 128 << 10;
constexpr int64_t kGapFewKeys = 512;
constexpr int64_t kGapSkelLdsMax = 78 << 10;  // two such workgroups per CU (160 KB)
// (two 256-thread workgroups per CU either way: the kernel's 240 VGPRs)
constexpr int kGapLdsProbe = 72 << 10;
constexpr int kGapMaxRounds = 64;
constexpr int kGapProbeMinLen = 1024;
constexpr int kGapWaveMaxLen = 256;  // keys up to this long: one-wave gap-tier workgroups
constexpr int64_t kGapWaveMinKeys = 1024;             // ... when there are more of them than this
constexpr int64_t kGapWideMaxKeys = 64;    // at most this many keys for the gap tier ...
constexpr int kGapWideMinLen = 2048;        // ... the longest of them this long: 512-thread workgroups

}  // namespace

void lcrt::set_err(lc_ctx *c, const std::string &s) {
  std::lock_guard<std::mutex> g(c->err_mu);
  c->err = s;
}

int lcrt::check_offsets(lc_ctx *c, const char *who, const int64_t *key_off, int64_t n_keys) {
  if (key_off[0] < 0) {
    set_err(c, std::string(who) + ": key_off[0] < 0");
    return -EINVAL;
  }
  for (int64_t k = 0; k < n_keys; k++)
    if (key_off[k + 1] < key_off[k]) {
      set_err(c, std::string(who) + ": key_off not monotone at key " + std::to_string(k));
      return -EINVAL;
    }
  return 0;
}

// NAME=0 in the environment: a path's switch, read where the path is chosen
bool lcrt::env_is_off(const char *name) {
  const char *e = getenv(name);
  return e && e[0] == '0';
}

int lcrt::opts_to_params(lc_ctx *c, const lc_opts *o, lcdev::KParams *p) {
  lc_opts d;
  lc_default_opts(&d);
  if (!o) o = &d;
  if (o->init_version < 0 || o->init_version > 0x7FFFFFFE ||
      o->init_value < -1 || o->init_value > 0x7FFFFFFE) {
    set_err(c, "lc_opts: init_version/init_value out of int32 range");
    return -EINVAL;
  }
  p->init_ver = (int32_t)o->init_version;
  p->init_val = (int32_t)o->init_value;
  p->budget = o->max_configs_per_key > 0 ? o->max_configs_per_key : kDefaultBudget;
  p->time_ticks = 0;
  if (o->time_budget_ms > 0) {
    // device wall clock (s_memrealtime) rate, kHz = ticks per ms
    int dev = 0, khz = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
      khz = 100000;
    p->time_ticks = (uint64_t)o->time_budget_ms * (uint64_t)khz;
  }
  return 0;
}

// Is [p, p + n) inside a buffer registered with lc_host_register?
bool lcrt::is_pinned(lc_ctx *c, const void *p, size_t n) {
  std::lock_guard<std::mutex> g(c->pin_mu);
  const char *q = static_cast<const char *>(p);
  for (const auto &pr : c->pinned)
    if (q >= pr.first && q + n <= pr.first + pr.second) return true;
  return false;
}

// The device's staging buffer (kStageMax bytes, allocated on first use), or
// null with the context's error set.
char *lcrt::stage_buf(lc_ctx *c, Dev &d) {
  if (!d.h_stage) {
    if (hipHostMalloc(reinterpret_cast<void **>(&d.h_stage), kStageMax, 0) != hipSuccess) {
      d.h_stage = nullptr;
      set_err(c, "hipHostMalloc (staging) failed");
      return nullptr;
    }
  }
  return d.h_stage;
}

namespace {

// A gap-tier full-decision launch: its sizes and job (run_device).
struct GapPlan {
  int64_t gap_cap = 0;     // workspace entries per array per workgroup
  size_t gap_per_wg = 0;
  int wg_cap = 0, full_wg = 0;
  bool wide_wg = false, no_lds = false;
  size_t nk = 0;           // counterexample slots (the cex arrays' stride)
  lcdev::GapJob job{};
};

}  // namespace

// Infeasibility certificates for the invalid keys of a run_device call
// (cert.hip), after every tier has decided.
int lcrt::run_certificates(lc_ctx *c, Dev &d, const lc_op *d_ops, const int64_t *d_off, int64_t n_keys,
                     const lcdev::KParams &p, const lc_key_result *d_out, hipStream_t st,
                     const AuxOut &wo) {
  if (!wo.cert || !wo.cset || n_keys <= 0) return 0;
  if (!d.maybe_invalid) {
    // every key was decided by the version-order tier, which decides valid
    // keys only: no certificate to find, every key LC_CERT_NONE
    HIP_TRY(c, lcdev::launch_cert_none(wo.cert, n_keys, st));
    return 0;
  }
  if (int rc = ensure(c, d.d_cws, lcdev::cert_ws_bytes(wo.n_records, n_keys))) return rc;
  HIP_TRY(c, lcdev::launch_certificates(d_ops, d_off, n_keys, wo.n_records, p, d_out, d.d_cws.p,
                                        wo.cert, wo.cset, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return 0;
}

// A fused call's lazily copied status (Dev::st_pending): choose the next
// call's pass from it and return the keys the crash-light decision took (the
// call's n_gap), or -1 when nothing was pending.
int64_t lcrt::settle_status(Dev &d) {
  if (!d.st_pending) return -1;
  d.st_pending = false;
  if (hipEventSynchronize(d.es) != hipSuccess) return 0;
  const int32_t n_light = __atomic_load_n(d.h_handoff + 1, __ATOMIC_ACQUIRE);  // (status_settle_kernel)
  d.use_fused = 4 * (int64_t)n_light > d.st_keys;
  return n_light;
}

// A call that returned on the completion signal: its pass's HIP-event time,
// read once the kernel has retired (now, if it has not yet), into the
// device's statistics and the context's totals.  Before the events are
// recorded again, and by lc_last_stats / lc_last_totals.
void lcrt::settle_timing(lc_ctx *c, Dev &d) {
  if (!d.timing_pending) return;
  d.timing_pending = false;
  float ms = 0;
  if (hipEventSynchronize(d.ef) == hipSuccess && hipEventElapsedTime(&ms, d.e0, d.ef) == hipSuccess) {
    d.fast_ms = ms;
    d.kernel_ms = ms;
    d.tot.timed_calls++;
    d.tot.fast_kernel_ms += ms;
    d.tot.kernel_ms += ms;
  }
}

// d_status copied into h_status, and waited for.
int lcrt::read_status(lc_ctx *c, Dev &d, hipStream_t st) {
  HIP_TRY(c, hipMemcpyAsync(d.h_status, d.d_status, sizeof(lcdev::KStatus), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  return 0;
}

namespace {

// Wait for the pass's follower signal (seq in *h_done): spin, checking the
// stream every 1,024 rounds; past 2 ms (or once the stream is idle, which
// cannot happen before the word) synchronise the stream instead.  Returns 0,
// or -EIO on a stream error.
int wait_done(lc_ctx *c, Dev &d, uint32_t seq, hipStream_t st) {
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t i = 1;; i++) {
    if (__atomic_load_n(d.h_done, __ATOMIC_ACQUIRE) == seq) return 0;
    if ((i & 1023) == 0) {
      const hipError_t q = hipStreamQuery(st);
      if (q == hipSuccess) return 0;
      if (q != hipErrorNotReady) {
        set_err(c, std::string("fast tier: ") + hipGetErrorString(q));
        return -EIO;
      }
      if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) {
        HIP_TRY(c, hipStreamSynchronize(st));
        return 0;
      }
    }
  }
}

// ---- Resident version-order grid (kernels.h, launch_fast_resident) ----
// lc_check_device on a batch of at most one key per resident workgroup
// (C3's 1,250-key shard) is served by a grid that stays on the GPU between
// calls: the call writes the request and rings, the grid decides it and
// signals, and back-to-back calls pay neither a launch nor the follower
// kernel.  The grid leaves after LC_RESIDENT_IDLE_US (default 50) without a
// request, before any other work of this library runs on the device, and at
// lc_close.  LC_RESIDENT=0 turns it off (every call launches).

// Write request number d.res_seq + 1 (every word tagged with it).
void res_ring(Dev &d, const uint64_t (&v)[lcdev::kResWords]) {
  const uint32_t seq = ++d.res_seq;
  for (int i = 0; i < lcdev::kResWords; i++)
    __atomic_store_n(&d.res_h->req[i], lcdev::res_word(v[i], seq), __ATOMIC_RELEASE);
}

}  // namespace

// Stop the grid (if one is live) and wait for it to leave.
int lcrt::res_stop(lc_ctx *c, Dev &d) {
  if (!d.res_grid) return 0;
  uint64_t v[lcdev::kResWords] = {};
  v[2] = (uint64_t)lcdev::kResExitKeys;
  res_ring(d, v);
  d.res_grid = 0;
  HIP_TRY(c, hipStreamSynchronize(d.rst));
  return 0;
}

int lcrt::side_begin(lc_ctx *c, hipStream_t *st) {
  Dev &d = c->devs[0];
  HIP_TRY(c, hipSetDevice(d.id));
  (void)settle_status(d);
  if (int e = res_stop(c, d)) return e;  // the resident grid leaves before other work runs
  *st = d.stream;
  return 0;
}

int lcrt::side_begin(lc_ctx *c, SideState &s, int n_events, size_t pinned_bytes, hipStream_t *st) {
  if (int e = side_begin(c, st)) return e;
  for (int i = 0; i < n_events; i++)
    if (!s.ev[i]) HIP_TRY(c, hipEventCreate(&s.ev[i]));
  if (pinned_bytes && !s.pinned) HIP_TRY(c, hipHostMalloc(&s.pinned, pinned_bytes, 0));
  return 0;
}

void lcrt::release(SideState &s) {
  if (s.arena.p) (void)hipFree(s.arena.p);
  if (s.pinned) (void)hipHostFree(s.pinned);
  for (hipEvent_t e : s.ev)
    if (e) (void)hipEventDestroy(e);
  s = SideState{};
}

namespace {

// One request: returns 0 with every key decided or flagged for the later
// tiers (d.h_handoff as after fast_tier_kernel), its device time in
// *dev_ms; 1 when the grid could not serve it (the caller launches
// instead); or a negative error.
int res_request(lc_ctx *c, Dev &d, const lc_op *d_ops, const int64_t *d_off, int64_t n_keys,
                const lcdev::KParams &p, lc_key_result *d_out, hipStream_t st, double *dev_ms) {
  if (!d.res_h) {
    if (hipHostMalloc(reinterpret_cast<void **>(&d.res_h), sizeof(lcdev::ResHost),
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&d.res_h_dev), d.res_h, 0) != hipSuccess ||
        hipMalloc(reinterpret_cast<void **>(&d.res_d), sizeof(lcdev::ResDev)) != hipSuccess ||
        hipStreamCreateWithFlags(&d.rst, hipStreamNonBlocking) != hipSuccess ||
        hipDeviceGetAttribute(&d.res_khz, hipDeviceAttributeWallClockRate, d.id) != hipSuccess ||
        d.res_khz <= 0) {
      d.res_broken = true;
      return 1;
    }
    std::memset(static_cast<void *>(d.res_h), 0, sizeof(lcdev::ResHost));
  }
  // the inputs (and this call's memsets) are ready once the caller's stream is
  if (hipStreamQuery(st) != hipSuccess) HIP_TRY(c, hipStreamSynchronize(st));
  lcdev::ResHost *h = d.res_h;
  const uint64_t v[lcdev::kResWords] = {
      (uint64_t)d_ops, (uint64_t)d_off, (uint64_t)n_keys, (uint64_t)d_out, (uint64_t)d.d_flags.p,
      (uint64_t)d.d_status, (uint64_t)d.h_handoff_dev, (uint64_t)(uint32_t)p.init_ver,
      (uint64_t)(uint32_t)p.init_val};
  for (int attempt = 0; attempt < 3; attempt++) {
    // a grid that left on its idle bound has finished (its stream drained)
    // before a new one starts; a grid too small for this batch is stopped
    if (d.res_grid && (__atomic_load_n(&h->exited, __ATOMIC_ACQUIRE) || d.res_grid < n_keys))
      if (int e = res_stop(c, d)) return e;
    if (!d.res_grid) {
      // a new grid: numbering from 0 (no word tagged 1 yet), counters zero
      for (int i = 0; i < 16; i++) __atomic_store_n(&h->req[i], 0, __ATOMIC_RELAXED);
      __atomic_store_n(&h->exited, 0u, __ATOMIC_RELAXED);
      __atomic_store_n(&h->done, 0, __ATOMIC_RELEASE);
      d.res_seq = 0;
      const char *ie = getenv("LC_RESIDENT_IDLE_US");  // (read at each launch)
      d.res_idle_us = ie ? std::max<int64_t>(1, atoll(ie)) : 50;
      HIP_TRY(c, hipMemsetAsync(d.res_d, 0, sizeof(lcdev::ResDev), d.rst));
      HIP_TRY(c, lcdev::launch_fast_resident(d.res_h_dev, d.res_d, n_keys,
                                             (uint64_t)d.res_idle_us * (uint64_t)d.res_khz / 1000u,
                                             d.rst));
      d.res_grid = n_keys;
    }
    res_ring(d, v);
    const uint32_t seq = d.res_seq;
    // wait for the completion; every 1,024 rounds check that the grid has
    // not left (idle bound before the request: serve it from a new grid)
    // and bound the wait (a request is at most ~0.1 ms of device work)
    const auto t0 = std::chrono::steady_clock::now();
    bool left = false;
    for (uint32_t i = 1;; i++) {
      const uint64_t dn = __atomic_load_n(&h->done, __ATOMIC_ACQUIRE);
      if ((uint32_t)(dn >> 32) == seq) {
        const uint32_t a = (uint32_t)__atomic_load_n(&h->t0, __ATOMIC_RELAXED);
        *dev_ms = (double)(uint32_t)((uint32_t)dn - a) / (double)d.res_khz;
        return 0;
      }
      if ((i & 1023) == 0) {
        if (__atomic_load_n(&h->exited, __ATOMIC_ACQUIRE)) {
          left = true;
          break;
        }
        const hipError_t q = hipStreamQuery(d.rst);
        if (q != hipSuccess && q != hipErrorNotReady) {
          set_err(c, std::string("resident grid: ") + hipGetErrorString(q));
          d.res_grid = 0;
          d.res_broken = true;
          return -EIO;
        }
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(500)) break;
      }
    }
    if (int e = res_stop(c, d)) return e;
    if (!left) break;  // not served in 500 ms: launches from now on
    // (the grid left before it saw the request: the host was away longer
    // than the idle bound) — again, from a new grid
  }
  d.res_broken = true;
  return 1;
}

// One run_device call: its arguments, what follows from them, and what one
// stage leaves for the next.  The stages below read and write this and Dev.
struct Run {
  lc_ctx *c;
  Dev &d;
  const lc_op *d_ops;  // (a native 24-byte pass: named by Source::widen at the handoff)
  const int64_t *d_off;
  int64_t n_keys;
  const lcdev::KParams &p;
  lc_key_result *d_out;
  hipStream_t st;
  int64_t flags;
  const AuxOut &ao;
  const Source &src;
  bool fast_on = false;
  // With the gap tier on, the fast tier sends keys it can only pass on (no
  // version on an :ok mutation, a read [nil x], malformed) straight to the
  // JIT list d_jit2, which the gap tier then appends to.
  bool gap_on = false;
  bool want_wit = false;
  // A call with one pass launch (no chunks) returns on the pass's follower
  // signal (kernels.h launch_done_signal) instead of an event wait; with
  // LC_FLAG_NO_TIMING it records no events around the pass either.
  bool signal = false, timing = true;
  bool fused = false;  // the version-order and crash-light decisions run as one pass
  bool light = false;  // the crash-light pass ran (its time is in gap_ms)
  int64_t n_jit = 0;   // keys still to decide, listed in jit_list (null: every key)
  const int32_t *jit_list = nullptr;
  int64_t n_direct = 0;  // keys the fast tier sent straight to d_jit2
  int32_t n_ovf = 0;     // keys the search tier leaves to the HBM tiers (d_ovf)
  hipEvent_t before_jit = nullptr;
  // witness_stage: the keys it left at n_window (listed in d_ovf2), and the
  // longest key of its own list, for counted_witness_stage
  int32_t n_wlist = 0;
  int64_t wit_max_len = 0;
  GapPlan early;  // the gap tier launched early (handoff), if it was
  bool early_launched = false;
};

// The gap tier's full-decision launch for keys up to max_len records long,
// nj of them at most (buffers ensured).
int gap_plan(Run &r, int64_t max_len, int64_t nj, GapPlan &g) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  g.gap_cap = (max_len + 2 + 3) & ~int64_t(3);  // 16-B records
  g.gap_per_wg = lcdev::gap_tier_ws_bytes(1, g.gap_cap);
  if (g.gap_per_wg > kGapWsBytes) return 0;  // (the caller checks)
  g.wg_cap = (int)std::min<int64_t>(
      (int64_t)kGapMaxWG, std::max<int64_t>(1, (int64_t)(kGapWsBytes / g.gap_per_wg)));
  // many short keys: one-wave workgroups, four times as many decisions in
  // flight (10k 200-op keys: 0.78 -> 0.45 ms); few keys are latency-bound
  // and decide faster with 256 threads each (94 keys: 0.19 vs 0.145 ms)
  const bool wave_wg = max_len <= kGapWaveMaxLen && nj > kGapWaveMinKeys;
  g.full_wg = (int)std::min<int64_t>(nj, wave_wg ? 4 * (int64_t)g.wg_cap : g.wg_cap);
  int rc = ensure(c, d.d_gws, lcdev::gap_tier_ws_bytes(g.full_wg, g.gap_cap));
  // counterexample intervals: key, lo, hi, gaps, state (int32), nodes
  // (int64) per invalid key, and one int32 per probe workgroup
  g.nk = (size_t)nj;
  if (!rc) rc = ensure(c, d.d_cex, g.nk * (5 * 4 + 8) + 4 * (size_t)g.wg_cap + 64);
  if (rc) return rc;
  lcdev::GapJob &job = g.job;
  job = lcdev::GapJob{};
  // LC_GAP_PREF_BUDGET (tests): a tiny budget sends every branching decision
  // through the plain-order rerun
  const char *pb_env = getenv("LC_GAP_PREF_BUDGET");
  job.pref_budget = pb_env ? std::max(1, atoi(pb_env)) : lcdev::kGapPrefBudget;
  const size_t nk = g.nk;
  job.cex_nodes = reinterpret_cast<int64_t *>(d.d_cex.p);
  job.cex_key = reinterpret_cast<int32_t *>(d.d_cex.p + 8 * nk);
  job.cex_lo = reinterpret_cast<uint32_t *>(job.cex_key + nk);
  job.cex_hi = job.cex_lo + nk;
  job.cex_gaps = reinterpret_cast<int32_t *>(job.cex_hi + nk);
  job.cex_state = job.cex_gaps + nk;
  job.probe = job.cex_state + nk;
  job.mode = lcdev::kGapFull;
  job.n_tasks = (int32_t)nj;
  job.wit = r.want_wit ? r.ao.wit : nullptr;
  job.wkind = r.want_wit ? r.ao.kind : nullptr;
  // short keys: one-wave workgroups (barriers nearly free, 4x the decisions
  // in flight); longer keys: 256 threads share each decision's setup; a
  // few long keys (C4): 512, whose extra waves halve the setup's record
  // passes (the matching is one wave either way)
  g.wide_wg = nj <= kGapWideMaxKeys && max_len >= kGapWideMinLen;
  job.threads = wave_wg ? 64 : g.wide_wg ? 512 : 256;
  // Bisect counterexamples in place unless the keys are long and few
  // enough for multisection rounds to pay (each round costs two launches
  // and a sync; a probe of a short key costs less than that).
  job.bisect = max_len < kGapProbeMinLen || 2 * nj > g.wg_cap;
  // LDS per workgroup: the longest key's skeleton (68 B per record) plus
  // 8 KB for its matching when that stays within kGapSkelLdsMax (two
  // workgroups per CU); else room for the matching alone (80 B per record
  // plus its class table at worst), up to kGapLdsFull, or kGapLdsFew when
  // there are few keys
  const int64_t skel = 68 * g.gap_cap + (8 << 10);
  const int64_t match_cap = nj <= kGapFewKeys ? kGapLdsFew : kGapLdsFull;
  job.lds_bytes = (int)(skel <= kGapSkelLdsMax ? skel
                                               : std::min<int64_t>(match_cap, 80 * g.gap_cap + 1040));
  // LC_GAP_LDS=0 (tests): keep every matching in the HBM workspace
  g.no_lds = env_is_off("LC_GAP_LDS");
  if (g.no_lds) job.lds_bytes = 0;
  return 0;
}

// Settle what the last call left pending, make room for the per-key lists,
// and bring the handoff flags and d_status to zero.
// Invariant: d_status and the flags are zero between calls that completed
// (status_dirty / flags_dirty false); both are set again here until this
// call ends cleanly, so after an error return the next call re-zeroes.
int begin_call(Run &r) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  (void)settle_status(d);  // before use_fused or h_status is read
  settle_timing(c, d);     // before e0 / ef are recorded again
  d.tot.calls++;
  d.kernel_ms = d.hbm_ms = d.fast_ms = d.jit_ms = d.gap_ms = 0;
  d.n_hbm = d.n_jit = d.n_gap = 0;
  d.malformed = 0;
  d.counted = lc_counted_stats{};
  d.wit = lc_witness_stats{};
  d.cwit = lc_counted_witness_stats{};
  if (r.n_keys <= 0) return 0;
  if (r.n_keys > INT32_MAX) {
    set_err(c, "lc_check: more than 2^31-1 keys in one call");
    return -EINVAL;
  }
  const size_t list_bytes = sizeof(int32_t) * (size_t)r.n_keys;
  int rc = ensure(c, d.d_ovf, list_bytes);
  if (!rc) rc = ensure(c, d.d_ovf2, list_bytes);
  if (!rc) rc = ensure(c, d.d_jit, list_bytes);
  if (!rc) rc = ensure(c, d.d_jit2, list_bytes);
  if (!rc) rc = ensure(c, d.d_gap2, list_bytes);
  const bool flags_new = d.d_flags.cap < list_bytes || !d.d_flags.p;
  if (!rc) rc = ensure(c, d.d_flags, list_bytes);
  if (rc) return rc;
  if (flags_new || d.flags_dirty)  // the flags are all-zero between calls that completed
    HIP_TRY(c, hipMemsetAsync(d.d_flags.p, 0, d.d_flags.cap, st));
  d.flags_dirty = false;
  // d_status is zero on entry (the fast tier re-zeroes it; later tiers are
  // followed by a memset).  Until this call ends cleanly, assume it is not.
  if (d.status_dirty)
    HIP_TRY(c, hipMemsetAsync(d.d_status, 0, sizeof(lcdev::KStatus), st));
  d.status_dirty = true;
  return 0;
}

// Keys [k0, k0 + nk), records from r0 (relative to d_ops): the witness
// initialisation (the version order is the witness of every key the fast
// tier decides) and tier 0, the version-order decision (or the fused
// pass); the keys it cannot decide are flagged for the later tiers.
int launch_pass(Run &r, int64_t k0, int64_t nk, int64_t r0, int64_t nrec) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  const lcdev::KParams &p = r.p;
  const int64_t *off = r.d_off + k0;
  lc_key_result *out = r.d_out + k0;
  int32_t *flg = d.d_flags.p + k0;
  if (r.src.ops32) {  // the native 24-byte pass (no lc_aux outputs)
    const int64_t *base = r.src.base32 ? r.src.base32 + k0 : nullptr;
    if (r.fused)
      HIP_TRY(c, lcdev::launch_fused_tier32(r.src.ops32 + r0, off, base, nk, p, out, flg, d.d_status,
                                            d.h_handoff_dev, st));
    else
      HIP_TRY(c, lcdev::launch_fast_tier32(r.src.ops32 + r0, off, base, nk, p, out, flg, d.d_status,
                                           d.h_handoff_dev, st));
    return 0;
  }
  const lc_op *o = r.d_ops + r0;
  int32_t *wit = r.want_wit ? r.ao.wit + r0 : nullptr;
  int32_t *kind = r.want_wit ? r.ao.kind + k0 : nullptr;
  if (r.want_wit)
    HIP_TRY(c, lcdev::launch_witness_init(o, off, nk, nrec, p, r.fast_on, wit, kind, st));
  if (!r.fast_on) return 0;
  if (r.fused)
    HIP_TRY(c, lcdev::launch_fused_tier(o, off, nk, p, out, flg, d.d_status, d.h_handoff_dev, wit, kind,
                                        st));
  else
    HIP_TRY(c, lcdev::launch_fast_tier(o, off, nk, p, out, flg, d.d_status, d.h_handoff_dev, st));
  return 0;
}

// lc_check's pipeline: chunk i's copy is issued, the compute stream waits
// for it, widens it (24-byte records) and decides its keys while the copy
// engine moves chunk i + 1.
int launch_chunks(Run &r, const Chunks &ch) {
  lc_ctx *c = r.c;
  hipStream_t st = r.st;
  for (int i = 0; i < ch.n; i++) {
    if (int e = ch.issue(i)) return e;
    HIP_TRY(c, hipStreamWaitEvent(st, ch.ready[i], 0));
    const int64_t k0 = ch.k[i], nk = ch.k[i + 1] - k0;
    const int64_t r0 = ch.r[i], nrec = ch.r[i + 1] - r0;
    if (nk <= 0) continue;
    const int64_t *base = ch.d_base ? ch.d_base + k0 : nullptr;
    lc_op *wide = const_cast<lc_op *>(r.d_ops) + r0;
    if (ch.d_ops32 && !r.src.ops32)
      HIP_TRY(c, lcdev::launch_widen32(ch.d_ops32 + r0, r.d_off + k0, base, nk, ch.max_len, wide, st));
    if (ch.d_ops16)
      HIP_TRY(c, lcdev::launch_widen16(ch.d_ops16 + r0, r.d_off + k0, base, nk, ch.max_len, wide, st));
    if (int e = launch_pass(r, k0, nk, r0, nrec)) return e;
  }
  return 0;
}

// The first pass over every key, served by the resident grid, by one launch
// or by lc_check's chunk pipeline, and waited for; d.fast_ms is its time
// (or timing_pending).  *handed: some key goes on to the later tiers.
//
// Hot paths (same HIP calls, same order, same streams as ever; add none):
//  * lc_check_device, signal path, every key decided: [event e0] pass
//    [event ef] done-signal, all on st, then spinning on h_done;
//  * the resident request: a query of st, then host-mapped words only;
//  * native lc_check_device32: as the first with the 24-byte pass.
// A live resident grid is stopped before any other work of the library runs
// on its device: here when this call does not use it, and in the grid's arm
// before the later tiers' first launch.
int first_pass(Run &r, bool *handed) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  *handed = false;
  d.maybe_invalid = true;
  if (r.fast_on) {
    // Crash-heavy batches (most keys carry crashed writes/CAS: every key goes
    // on to the crash-light decision) take the fused pass, which reads each
    // key's records once for both decisions; others the version-order tier,
    // whose smaller register budget keeps 7 workgroups per CU.  Chosen from
    // the previous call on this device (LC_FUSED=0/1 forces it).
    const char *fenv = getenv("LC_FUSED");
    r.fused = r.gap_on && (fenv ? fenv[0] == '1' : d.use_fused);
    // Only when some workgroup raised h_handoff is the count copied back.
    __atomic_store_n(d.h_handoff, 0, __ATOMIC_RELEASE);
    d.flags_dirty = true;  // until the handoff (if any) is compacted
  }
  // the resident grid serves lc_check_device's plain version-order pass on
  // a batch of at most one key per resident workgroup (res_request); any
  // other call on this device first stops a live grid
  if (d.res_cap < 0) d.res_cap = lcdev::fast_resident_capacity();
  const bool resident = r.signal && !r.fused && !r.want_wit && !r.src.ops32 && !d.res_broken &&
                        r.n_keys <= d.res_cap && !env_is_off("LC_RESIDENT");
  bool served = false;  // the grid decided the pass
  if (resident) {
    double res_ms = 0;
    const int rc = res_request(c, d, r.d_ops, r.d_off, r.n_keys, r.p, r.d_out, st, &res_ms);
    if (rc < 0) return rc;
    served = rc == 0;
    if (served) {
      r.timing = true;  // (the grid's device clock: free)
      d.fast_ms = res_ms;
    } else {
      // not served (the grid may have decided part of it): launch instead,
      // from the state the pass starts from — zeroed status and flags
      HIP_TRY(c, hipMemsetAsync(d.d_status, 0, sizeof(lcdev::KStatus), st));
      HIP_TRY(c, hipMemsetAsync(d.d_flags.p, 0, d.d_flags.cap, st));
      __atomic_store_n(d.h_handoff, 0, __ATOMIC_RELEASE);
    }
  } else if (d.res_grid) {
    if (int e = res_stop(c, d)) return e;
  }
  if (served) {
    *handed = __atomic_load_n(d.h_handoff, __ATOMIC_ACQUIRE) != 0;
    if (*handed) {
      // the grid's exit publishes the flags and the status words to the
      // later tiers (and frees its CUs); their times are measured from here
      if (int e = res_stop(c, d)) return e;
      HIP_TRY(c, hipEventRecord(d.e0, st));
      HIP_TRY(c, hipEventRecord(d.ef, st));
    }
  } else {
    if (r.timing) HIP_TRY(c, hipEventRecord(d.e0, st));
    if (r.src.chunks) {
      if (int e = launch_chunks(r, *r.src.chunks)) return e;
    } else if (int e = launch_pass(r, 0, r.n_keys, 0, r.ao.n_records)) {
      return e;
    }
    if (!r.fast_on) {  // (witness initialisation only: every key goes to the search tiers)
      HIP_TRY(c, hipEventRecord(d.ef, st));
      return 0;
    }
    if (r.timing) HIP_TRY(c, hipEventRecord(d.ef, st));
    if (r.signal) {
      HIP_TRY(c, lcdev::launch_done_signal(d.h_done_dev, ++d.seq, st));
      if (int e = wait_done(c, d, d.seq, st)) return e;
    } else {
      HIP_TRY(c, hipEventSynchronize(d.ef));
    }
    *handed = __atomic_load_n(d.h_handoff, __ATOMIC_ACQUIRE) != 0;
    if (r.signal && !*handed) {
      // every key decided: the pass's event time (if any) is read later
      d.timing_pending = r.timing;
    } else {
      if (!r.timing) {
        // the later tiers' times are measured from here (the pass untimed)
        HIP_TRY(c, hipEventRecord(d.e0, st));
        HIP_TRY(c, hipEventRecord(d.ef, st));
      }
      float ms = 0;
      HIP_TRY(c, hipEventSynchronize(d.ef));
      HIP_TRY(c, hipEventElapsedTime(&ms, d.e0, d.ef));
      d.fast_ms = ms;
    }
  }
  r.n_jit = 0;
  r.jit_list = d.d_jit.p;
  if (*handed) return 0;
  d.flags_dirty = false;  // no key raised its flag
  // the version-order tier and the fused pass decide valid keys only
  // (they hand invalid ones on for their counterexamples)
  d.maybe_invalid = false;
  if (r.fused) {
    // every key decided in the one pass: were most of them crash-light?
    // (the answer picks the next call's pass; copied now, read later)
    // (one launch: the count to mapped host memory, d_status zeroed behind
    // it now — while the host returns — not at the start of the next call)
    HIP_TRY(c, lcdev::launch_status_settle(d.d_status, d.h_handoff_dev + 1, st));
    HIP_TRY(c, hipEventRecord(d.es, st));
    d.st_pending = true;
    d.st_keys = r.n_keys;
    d.status_dirty = false;
  }
  return 0;
}

// Some key was handed over: the 48-byte records (a native 24-byte pass), the
// compaction of the flags into lists, the crash-light pass over the gap
// tier's list, the gap tier itself when it can be sized already, and the
// status read that tells what is left (n_jit / jit_list / n_direct).
// (h_status is free until that read: lc_check_device32's widen uses it as
// scratch for the record count.)
int handoff(Run &r) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  const int64_t n_keys = r.n_keys;
  int32_t *wit = r.want_wit ? r.ao.wit : nullptr, *kind = r.want_wit ? r.ao.kind : nullptr;
  // the native 24-byte pass: the later tiers read 48-byte records
  if (r.src.widen)
    if (int e = r.src.widen(&r.d_ops)) return e;
  HIP_TRY(c, lcdev::launch_handoff_compact(d.d_flags.p, r.d_off, n_keys, r.gap_on ? 1 : 0, d.d_jit.p,
                                           d.d_jit2.p, d.d_status, kind, st));
  d.flags_dirty = false;  // the compaction clears every flag it reads
  // the crash-light pass reads the list and its length from the device:
  // no host round trip between the compaction and it.  After the fused
  // pass too: the keys it hands over are invalid or beyond the in-place
  // decision, and the light pass names an invalid version-pinned key's
  // first failure (check_kernel.hip, first_failure), so every path gives
  // the same results
  if (r.gap_on) {
    HIP_TRY(c, lcdev::launch_gap_light(r.d_ops, r.d_off, d.d_jit.p, n_keys, r.p, r.d_out, d.d_gap2.p,
                                       d.d_status, wit, kind, st));
    HIP_TRY(c, hipEventRecord(d.el, st));
    // Launched early: a few keys, one longer than the light pass holds
    // (kFastMaxRecords: it goes on to the gap tier proper) and the
    // shard's offsets in host memory — the full decisions start right
    // behind the light pass, sized from those offsets, their count read
    // on the device (GapJob::n_tasks_dev), instead of after a host round
    // trip for the status.  Same decisions, same results.
    if (r.src.h_off && n_keys <= kGapWideMaxKeys) {
      int64_t ml = 0;
      for (int64_t k = 0; k < n_keys; k++)
        ml = std::max<int64_t>(ml, r.src.h_off[k + 1] - r.src.h_off[k]);
      // LC_GAP_EARLY=0 (A/B): wait for the status
      if (ml > lcdev::kFastMaxRecords && !env_is_off("LC_GAP_EARLY")) {
        GapPlan &early = r.early;
        if (int e = gap_plan(r, ml, n_keys, early)) return e;
        if (early.gap_per_wg <= kGapWsBytes) {
          early.job.n_tasks_dev = &d.d_status->n_gap2;
          HIP_TRY(c, lcdev::launch_gap_tier(r.d_ops, r.d_off, d.d_gap2.p, r.p, r.d_out, d.d_gws.p,
                                            early.full_wg, early.gap_cap, d.d_jit2.p, d.d_status,
                                            early.job, st));
          HIP_TRY(c, hipEventRecord(d.eg, st));
          r.early_launched = true;
        }
      }
    }
  }
  if (int e = read_status(c, d, st)) return e;
  r.n_direct = d.h_status->n_jit2;
  if (r.fused) lcdev::light_count(*d.h_status);
  if (!r.gap_on) {
    r.n_jit = d.h_status->n_jit;
    return 0;
  }
  // fused: were most keys crash-light?  Else: most keys handed to the
  // gap tier: the next call fuses the passes
  d.use_fused = r.fused ? 4 * (int64_t)d.h_status->n_light > n_keys
                        : 2 * (int64_t)d.h_status->n_jit > n_keys;
  r.light = true;
  float ms = 0;
  HIP_TRY(c, hipEventElapsedTime(&ms, d.ef, d.el));
  d.gap_ms = ms;
  d.n_gap = r.fused ? d.h_status->n_light : d.h_status->n_jit;
  r.n_jit = d.h_status->n_gap2;  // what the gap tier proper still has to decide
  r.jit_list = d.d_gap2.p;
  return 0;
}

// Counterexamples of long keys (n_cex open intervals after the full
// decisions): P probes per interval per round, over the whole GPU, then the
// witness pass.
int gap_counterexamples(Run &r, GapPlan &g, int32_t n_cex, int64_t gap_cap) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  lcdev::GapJob &job = g.job;
  job.mode = lcdev::kGapProbe;
  // the probes of a few long keys: 512-thread workgroups as for their full
  // decisions (half as many probes per round; C4's interval still closes in
  // two rounds)
  job.threads = g.wide_wg ? 512 : 256;
  job.lds_bytes = g.no_lds ? 0 : kGapLdsProbe;
  // as many probes as run at once: a round's time is its slowest batch
  // of resident workgroups, and a second batch doubles it for a few
  // more cuts (C4 invalid: 1,024 probes = two batches of 512 resident)
  const int resident = lcdev::gap_tier_resident(job.lds_bytes, job.threads);
  job.P = (resident / n_cex >= 2 ? std::min(resident, g.wg_cap) : g.wg_cap) / n_cex;
  job.n_tasks = n_cex * job.P;
  if (int rc = ensure(c, d.d_gws, lcdev::gap_tier_ws_bytes(job.n_tasks, gap_cap))) return rc;
  for (int round = 0;; round++) {
    if (round == kGapMaxRounds) {
      // cannot happen (each round cuts an interval by P + 1 >= 3); the
      // JIT tier decides whatever is still open rather than the call fail
      job.give_up = 1;
      HIP_TRY(c, lcdev::launch_gap_narrow(r.d_ops, r.d_off, n_cex, r.d_out, d.d_jit2.p, d.d_status, job,
                                          st));
      break;
    }
    HIP_TRY(c, hipMemsetAsync(&d.d_status->n_open, 0, sizeof(int32_t), st));
    HIP_TRY(c, lcdev::launch_gap_tier(r.d_ops, r.d_off, nullptr, r.p, r.d_out, d.d_gws.p, job.n_tasks,
                                      gap_cap, d.d_jit2.p, d.d_status, job, st));
    HIP_TRY(c, lcdev::launch_gap_narrow(r.d_ops, r.d_off, n_cex, r.d_out, d.d_jit2.p, d.d_status, job,
                                        st));
    if (int e = read_status(c, d, st)) return e;
    if (d.h_status->n_open == 0) break;
  }
  if (r.want_wit) {
    // the witness of each closed counterexample's last linearizable prefix
    job.mode = lcdev::kGapWitness;
    job.P = 1;
    job.n_tasks = n_cex;
    HIP_TRY(c, lcdev::launch_gap_tier(r.d_ops, r.d_off, nullptr, r.p, r.d_out, d.d_gws.p,
                                      std::min<int>(n_cex, g.wg_cap), gap_cap, d.d_jit2.p, d.d_status,
                                      job, st));
  }
  return 0;
}

// Tier 1: gap matching for version-pinned keys (crashed writes/CAS, long
// keys, invalid keys); what it cannot decide goes on to the JIT search, whose
// list (n_jit / jit_list) and start event (before_jit) this leaves.
int gap_tier(Run &r) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  r.before_jit = r.light ? d.el : d.ef;
  if (!r.gap_on) return 0;
  const int64_t gap_cap = ((int64_t)d.h_status->max_len + 2 + 3) & ~int64_t(3);  // 16-B records
  if (r.n_jit == 0 || lcdev::gap_tier_ws_bytes(1, gap_cap) > kGapWsBytes) {
    // no gap-tier pass: its queue (if any) joins the direct keys for the JIT
    if (r.n_jit > 0)
      HIP_TRY(c, hipMemcpyAsync(d.d_jit2.p + r.n_direct, r.jit_list, sizeof(int32_t) * (size_t)r.n_jit,
                                hipMemcpyDeviceToDevice, st));
    r.n_jit += r.n_direct;
    r.jit_list = d.d_jit2.p;
    return 0;
  }
  GapPlan g;
  if (r.early_launched) {
    g = r.early;  // launched behind the light pass; the status read since includes it
  } else {
    if (int e = gap_plan(r, d.h_status->max_len, r.n_jit, g)) return e;
    HIP_TRY(c, lcdev::launch_gap_tier(r.d_ops, r.d_off, r.jit_list, r.p, r.d_out, d.d_gws.p, g.full_wg,
                                      g.gap_cap, d.d_jit2.p, d.d_status, g.job, st));
    if (int e = read_status(c, d, st)) return e;
  }
  g.job.n_tasks_dev = nullptr;
  const int32_t n_cex = d.h_status->n_cex;
  if (n_cex > 0)
    if (int e = gap_counterexamples(r, g, n_cex, gap_cap)) return e;
  if (!r.early_launched || n_cex > 0) {  // (launched early and done: the status is current)
    HIP_TRY(c, hipEventRecord(d.eg, st));
    if (int e = read_status(c, d, st)) return e;
  }
  float ms = 0;
  HIP_TRY(c, hipEventElapsedTime(&ms, d.ef, d.eg));
  d.gap_ms = ms;
  if (!r.light && !r.fused) d.n_gap = r.n_jit;
  r.n_jit = d.h_status->n_jit2;
  r.jit_list = d.d_jit2.p;
  r.before_jit = d.eg;
  return 0;
}

// Tier 2, the frontier search of the keys still listed: straight to the
// cooperative HBM tier (n_ovf of them in d_ovf) or through the LDS tier,
// which leaves the keys that outgrow it there.
int search_tier(Run &r) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  const int64_t n_jit = r.n_jit;
  float ms = 0;
  d.n_jit = n_jit;
  // Few keys for the frontier search (at most kJitDirectMaxKeys: one 4-wave
  // workgroup per key, all resident at once) go straight to the cooperative
  // tier, whose LDS tables serve small frontiers and whose hash tables keep
  // large ones; the LDS tier's one-wave-per-key pass would be redone for
  // every key that outgrows it.  Measured (tools/jit_direct_ab.py, version-
  // less batches): 1,000 x 1,000 at concurrency 20 19.4 -> 15.0 ms,
  // 1,000 x 200 2.4 -> 1.8 ms, 64 x 1,000 10.1 -> 6.5 ms; but 4,000 x 100
  // 1.0 -> 3.0 ms, where the LDS tier's four keys per workgroup win.
  // LC_JIT_DIRECT=0 (A/B) keeps the LDS tier first.
  // (not with LC_FLAG_NO_FAST_PATH, whose JIT list is implicit: every key)
  const bool direct = !env_is_off("LC_JIT_DIRECT") && n_jit > 0 && r.jit_list &&
                      n_jit <= kJitDirectMaxKeys && !(r.flags & LC_FLAG_NO_HBM_RETRY);
  if (direct)
    HIP_TRY(c, hipMemcpyAsync(d.d_ovf.p, r.jit_list, sizeof(int32_t) * (size_t)n_jit,
                              hipMemcpyDeviceToDevice, st));
  if (direct || n_jit == 0) {
    HIP_TRY(c, hipEventElapsedTime(&ms, d.e0, r.before_jit));
    d.kernel_ms = ms;
  } else {
    // JIT search with the frontier in SGPRs / LDS
    HIP_TRY(c, lcdev::launch_lds_tier(r.d_ops, r.d_off, r.jit_list, n_jit, r.p, r.d_out, d.d_ovf.p,
                                      d.d_status, st));
    HIP_TRY(c, hipEventRecord(d.e1, st));
    if (int e = read_status(c, d, st)) return e;
    HIP_TRY(c, hipEventElapsedTime(&ms, r.before_jit, d.e1));
    d.jit_ms = ms;
    HIP_TRY(c, hipEventElapsedTime(&ms, d.e0, d.e1));
    d.kernel_ms = ms;
  }
  d.malformed = d.h_status->malformed;
  r.n_ovf = direct ? (int32_t)n_jit : d.h_status->n_overflow;
  d.n_hbm = r.n_ovf;
  return 0;
}

// HBM-tier re-runs of the keys in d_ovf, each tier passing what outgrows it
// to the next.
int hbm_tiers(Run &r) {
  if (r.n_ovf <= 0 || (r.flags & LC_FLAG_NO_HBM_RETRY)) return 0;
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  int32_t n_list = r.n_ovf;
  int32_t *list = d.d_ovf.p, *next = d.d_ovf2.p;
  HIP_TRY(c, hipEventRecord(d.e1, st));
  // LC_HBM_COOP (test/A-B knob): 0 one wavefront per key throughout,
  // 4 / 16 a workgroup of that many wavefronts per key throughout; default:
  // 8 for at most 512 keys (two workgroups per CU), else 4.  (Round 1 used
  // one wavefront per key beyond 4,096 keys; with the LDS tables the
  // 4-wave workgroups win there too: version-less 10,000 x 1,000 at
  // concurrency 20, HBM tier 128 -> 98 ms, tools/hbm_width_large.py.)
  const char *coop_env = getenv("LC_HBM_COOP");
  const int coop_mode = coop_env ? atoi(coop_env) : 1;
  for (int tier = 0; tier < kHbmTiers && n_list > 0; tier++) {
    int wpk = coop_mode == 1 ? (n_list <= kHbmCoop8MaxKeys ? 8 : 4) : coop_mode;
    const bool coop = wpk == 4 || wpk == 8 || wpk == 16;
    // workgroups: at most the resident ones (keys are claimed dynamically)
    const int resident = wpk == 16 ? kHbmCoop16Resident : wpk == 8 ? 512
                         : wpk == 4 ? kHbmCoop4Resident : kHbmWaves[tier];
    const int waves = std::min<int>(std::min(kHbmWaves[tier], resident), n_list);
    if (int rc = ensure(c, d.d_ws, lcdev::hbm_tier_ws_bytes(waves, kHbmCap[tier]))) return rc;
    HIP_TRY(c, hipMemsetAsync(&d.d_status->n_overflow2, 0, sizeof(int32_t), st));
    HIP_TRY(c, hipMemsetAsync(&d.d_status->hbm_next, 0, sizeof(int32_t), st));
    const int last = tier == kHbmTiers - 1;
    if (coop)
      HIP_TRY(c, lcdev::launch_hbm_coop(r.d_ops, r.d_off, list, n_list, r.p, r.d_out, d.d_ws.p, waves,
                                        kHbmCap[tier], next, &d.d_status->n_overflow2,
                                        &d.d_status->malformed, &d.d_status->hbm_next, last, wpk, st));
    else
      HIP_TRY(c, lcdev::launch_hbm_tier(r.d_ops, r.d_off, list, n_list, r.p, r.d_out, d.d_ws.p, waves,
                                        kHbmCap[tier], next, &d.d_status->n_overflow2,
                                        &d.d_status->malformed, &d.d_status->hbm_next, last, st));
    if (int e = read_status(c, d, st)) return e;
    n_list = tier < kHbmTiers - 1 ? d.h_status->n_overflow2 : 0;
    std::swap(list, next);
  }
  float ms = 0;
  HIP_TRY(c, hipEventRecord(d.e2, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipEventElapsedTime(&ms, d.e1, d.e2));
  d.hbm_ms = ms;
  d.malformed = d.h_status->malformed;  // (keys sent straight here report it)
  return 0;
}

// LC_FLAG_COUNTED_CLASSES: the keys the tiers left :unknown with
// LC_REASON_WINDOW_OVERFLOW (listed on the device from d_out) are searched
// again with their crashed writes/CAS counted per class (kernels.h
// launch_counted_tier), over the HBM tiers' ladder of set capacities.  Runs
// after every tier's event time has been read (e1 / e2 are free again); the
// counters it uses are zero on entry as all of d_status is.
int counted_tier(Run &r) {
  if (!(r.flags & LC_FLAG_COUNTED_CLASSES)) return 0;
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  int32_t *list = d.d_ovf.p, *next = d.d_ovf2.p;
  HIP_TRY(c, hipEventRecord(d.e1, st));
  HIP_TRY(c, lcdev::launch_counted_compact(r.d_out, r.n_keys, list, &d.d_status->n_counted, st));
  if (int e = read_status(c, d, st)) return e;
  int32_t n_list = d.h_status->n_counted;
  d.counted.n_keys = n_list;
  if (n_list <= 0) return 0;
  const int by_value = !env_is_off("LC_COUNTED_BY_VALUE");
  for (int tier = 0; tier < kHbmTiers && n_list > 0; tier++) {
    const int waves = std::min<int>(kHbmWaves[tier], n_list);
    if (int rc = ensure(c, d.d_ws, lcdev::hbm_tier_ws_bytes(waves, kHbmCap[tier]))) return rc;
    HIP_TRY(c, hipMemsetAsync(&d.d_status->n_overflow2, 0, sizeof(int32_t), st));
    HIP_TRY(c, hipMemsetAsync(&d.d_status->hbm_next, 0, sizeof(int32_t), st));
    HIP_TRY(c, lcdev::launch_counted_tier(r.d_ops, r.d_off, list, n_list, r.p, r.d_out, d.d_ws.p, waves,
                                          kHbmCap[tier], next, &d.d_status->n_overflow2, d.d_status,
                                          tier == kHbmTiers - 1, by_value, st));
    if (int e = read_status(c, d, st)) return e;
    n_list = tier < kHbmTiers - 1 ? d.h_status->n_overflow2 : 0;
    std::swap(list, next);
  }
  float ms = 0;
  HIP_TRY(c, hipEventRecord(d.e2, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  HIP_TRY(c, hipEventElapsedTime(&ms, d.e1, d.e2));
  d.counted.kernel_ms = ms;
  d.counted.n_decided = d.h_status->n_counted_decided;
  d.counted.n_unfit = d.h_status->n_counted_unfit;
  d.malformed = d.h_status->malformed;
  return 0;
}

// LC_FLAG_SEARCH_WITNESS: the keys that are decided but still have witness
// kind NONE (a search tier decided them) are listed on the device from d_out
// and the kind array and searched depth first for a linearization (kernels.h
// launch_witness_search), which becomes their witness; nothing else of the
// call's outputs changes.  Runs last, with its own status words (d_wst: the
// d_status invariant is not its concern) and, while it runs, the HBM tiers'
// workspace; e1 / e2 are free again.
int witness_stage(Run &r) {
  if (!(r.flags & LC_FLAG_SEARCH_WITNESS) || !r.want_wit) return 0;
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  if (int rc = ensure(c, d.d_wst, sizeof(lcdev::WitnessStatus))) return rc;
  lcdev::WitnessStatus ws{};
  auto read_ws = [&]() -> int {
    HIP_TRY(c, hipMemcpyAsync(&ws, d.d_wst.p, sizeof(ws), hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipStreamSynchronize(st));
    return 0;
  };
  int32_t *list = d.d_ovf.p;
  HIP_TRY(c, hipMemsetAsync(d.d_wst.p, 0, sizeof(lcdev::WitnessStatus), st));
  HIP_TRY(c, hipEventRecord(d.e1, st));
  HIP_TRY(c, lcdev::launch_witness_compact(r.d_out, r.ao.kind, r.d_off, r.n_keys, list, d.d_wst.p, st));
  if (int e = read_ws()) return e;
  const int32_t n_list = ws.n_list;
  d.wit.n_keys = n_list;
  if (n_list <= 0) return 0;
  // one wave per SIMD at most, and as many as kWitnessWsBytes of workspace
  // hold; a key longer than that much workspace for one wave is not searched
  int64_t max_n = std::max<int64_t>(ws.max_len, 1);
  while (lcdev::witness_wave_bytes(max_n) > kWitnessWsBytes) max_n /= 2;
  const int waves = (int)std::min<int64_t>(
      std::min<int64_t>(n_list, lcdev::kWitnessWaves),
      std::max<int64_t>(1, (int64_t)(kWitnessWsBytes / lcdev::witness_wave_bytes(max_n))));
  if (int rc = ensure(c, d.d_ws, lcdev::witness_ws_bytes(waves, max_n))) return rc;
  lcdev::KParams p = r.p;
  p.budget = std::min<int64_t>(p.budget, lcdev::kWitnessNodeCap);
  HIP_TRY(c, lcdev::launch_witness_search(r.d_ops, r.d_off, list, n_list, p, r.d_out, r.ao.wit, r.ao.kind,
                                          d.d_ws.p, waves, max_n, d.d_wst.p, d.d_ovf2.p, st));
  HIP_TRY(c, hipEventRecord(d.e2, st));
  if (int e = read_ws()) return e;
  r.n_wlist = ws.n_wlist;
  r.wit_max_len = ws.max_len;
  float ms = 0;
  HIP_TRY(c, hipEventElapsedTime(&ms, d.e1, d.e2));
  d.wit.kernel_ms = ms;
  d.wit.n_found = ws.n_found;
  d.wit.n_budget = ws.n_budget;
  d.wit.n_window = ws.n_window;
  d.wit.nodes = (int64_t)ws.nodes;
  d.wit.cache_hits = (int64_t)ws.cache_hits;
  d.tot.kernel_ms += ms;
  return 0;
}

// LC_FLAG_COUNTED_WITNESS (with LC_FLAG_SEARCH_WITNESS): the keys
// witness_stage left at n_window (it listed them in d_ovf2) are searched
// again with their crashed writes/CAS counted per class (kernels.h
// launch_witness_counted).  Runs right behind witness_stage: its status words
// (the stage's own are zero since witness_stage's memset), its workspace and
// e1 / e2, which are free again.
int counted_witness_stage(Run &r) {
  if (!(r.flags & LC_FLAG_COUNTED_WITNESS) || !(r.flags & LC_FLAG_SEARCH_WITNESS) || !r.want_wit) return 0;
  lc_ctx *c = r.c;
  Dev &d = r.d;
  hipStream_t st = r.st;
  const int32_t n_list = r.n_wlist;
  d.cwit.n_keys = n_list;
  if (n_list <= 0) return 0;
  int64_t max_n = std::max<int64_t>(r.wit_max_len, 1);
  while (lcdev::witness_counted_wave_bytes(max_n) > kWitnessWsBytes) max_n /= 2;
  const int waves = (int)std::min<int64_t>(
      std::min<int64_t>(n_list, lcdev::kWitnessWaves),
      std::max<int64_t>(1, (int64_t)(kWitnessWsBytes / lcdev::witness_counted_wave_bytes(max_n))));
  if (int rc = ensure(c, d.d_ws, lcdev::witness_counted_ws_bytes(waves, max_n))) return rc;
  lcdev::KParams p = r.p;
  p.budget = std::min<int64_t>(p.budget, lcdev::kWitnessNodeCap);
  HIP_TRY(c, hipEventRecord(d.e1, st));
  HIP_TRY(c, lcdev::launch_witness_counted(r.d_ops, r.d_off, d.d_ovf2.p, n_list, p, r.d_out, r.ao.wit,
                                           r.ao.kind, d.d_ws.p, waves, max_n, d.d_wst.p, st));
  HIP_TRY(c, hipEventRecord(d.e2, st));
  lcdev::WitnessStatus ws{};
  HIP_TRY(c, hipMemcpyAsync(&ws, d.d_wst.p, sizeof(ws), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  float ms = 0;
  HIP_TRY(c, hipEventElapsedTime(&ms, d.e1, d.e2));
  d.cwit.kernel_ms = ms;
  d.cwit.n_found = ws.cw_found;
  d.cwit.n_budget = ws.cw_budget;
  d.cwit.n_unfit = ws.cw_unfit;
  d.cwit.nodes = (int64_t)ws.cw_nodes;
  d.cwit.cache_hits = (int64_t)ws.cw_hits;
  d.tot.kernel_ms += ms;
  return 0;
}

// The later tiers ran: d_status back to zero (the invariant between calls),
// the call's totals.
int end_call(Run &r) {
  lc_ctx *c = r.c;
  Dev &d = r.d;
  HIP_TRY(c, hipMemsetAsync(d.d_status, 0, sizeof(lcdev::KStatus), r.st));
  HIP_TRY(c, hipStreamSynchronize(r.st));
  d.status_dirty = false;
  if (r.timing) {
    d.tot.timed_calls++;
    d.tot.fast_kernel_ms += d.fast_ms;
  }
  d.tot.kernel_ms += d.kernel_ms + d.hbm_ms + d.counted.kernel_ms;
  return 0;
}

}  // namespace

// Run the tiers for n_keys keys whose device arrays are in place.
int lcrt::run_device(lc_ctx *c, Dev &d, const lc_op *d_ops, const int64_t *d_off, int64_t n_keys,
                     const lcdev::KParams &p, lc_key_result *d_out, hipStream_t st, int64_t flags,
                     const AuxOut &ao, const Source &src) {
  Run r{c, d, d_ops, d_off, n_keys, p, d_out, st, flags, ao, src};
  r.fast_on = !(flags & LC_FLAG_NO_FAST_PATH);
  r.gap_on = !(flags & (LC_FLAG_NO_FAST_PATH | LC_FLAG_NO_GAP_TIER));
  r.want_wit = ao.wit && ao.kind;
  r.signal = !src.chunks && r.fast_on && n_keys > 0;
  r.timing = !r.signal || !(flags & LC_FLAG_NO_TIMING);
  r.n_jit = n_keys;
  if (int e = begin_call(r)) return e;
  if (n_keys <= 0) return 0;
  bool handed = false;
  if (int e = first_pass(r, &handed)) return e;
  if (handed)
    if (int e = handoff(r)) return e;
  if (r.n_jit == 0 && r.n_direct == 0) {  // every key decided (none left for the counted tier)
    d.kernel_ms = d.fast_ms + d.gap_ms;
    if (!d.timing_pending && r.timing) {
      d.tot.timed_calls++;
      d.tot.fast_kernel_ms += d.fast_ms;
      d.tot.kernel_ms += d.kernel_ms;
    }
    // after a handoff d_status is not zero: cleared behind this call's work
    // (the host has read it), not in front of the next call's
    if (r.light) HIP_TRY(c, hipMemsetAsync(d.d_status, 0, sizeof(lcdev::KStatus), st));
    d.status_dirty = false;
    if (int e = witness_stage(r)) return e;  // (a gap-tier decision may have come without a witness)
    return counted_witness_stage(r);
  }
  if (int e = gap_tier(r)) return e;
  if (int e = search_tier(r)) return e;
  if (int e = hbm_tiers(r)) return e;
  if (int e = counted_tier(r)) return e;
  if (int e = end_call(r)) return e;
  if (int e = witness_stage(r)) return e;
  return counted_witness_stage(r);
}

// One device's counters of the call added to the context's (zeroed when the
// call began).
void lcrt::fill_stats(lc_stats &s, const Dev &d) {
  s.kernel_ms += d.kernel_ms;
  s.fast_kernel_ms += d.fast_ms;
  s.jit_kernel_ms += d.jit_ms;
  s.n_jit_keys += d.n_jit;
  s.gap_kernel_ms += d.gap_ms;
  s.n_gap_keys += d.n_gap;
  s.hbm_kernel_ms += d.hbm_ms;
  s.n_hbm_keys += d.n_hbm;
  s.n_malformed += d.malformed;
}

namespace {

// key_off[n_keys] - key_off[0] of key offsets that live in device memory,
// read through d.h_status (pinned).  Only before any status copy of the
// same call: ahead of run_device, or from Source::widen at the handoff,
// which precedes the handoff's status read.
int device_record_count(lc_ctx *c, Dev &d, const int64_t *d_key_off, int64_t n_keys, hipStream_t st,
                        int64_t *nrec) {
  int64_t *ends = reinterpret_cast<int64_t *>(d.h_status);
  HIP_TRY(c, hipMemcpyAsync(&ends[0], d_key_off, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipMemcpyAsync(&ends[1], d_key_off + n_keys, sizeof(int64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  *nrec = ends[1] - ends[0];
  return 0;
}

// lc_check_device32: the 24-byte records in device memory widened into
// d.d_ops, *nrec of them.
int widen_device32(lc_ctx *c, Dev &d, const lc_op32 *d_ops32, const int64_t *d_key_off,
                   const int64_t *d_key_base, int64_t n_keys, hipStream_t st, int64_t *nrec) {
  if (int e = device_record_count(c, d, d_key_off, n_keys, st, nrec)) return e;
  if (*nrec < 0) {
    set_err(c, "lc_check_device32: key_off[n_keys] < key_off[0]");
    return -EINVAL;
  }
  if (int e = ensure(c, d.d_ops, sizeof(lc_op) * (size_t)*nrec)) return e;
  // the grid's second dimension for long keys: sized from the mean length
  // (any size is correct: each workgroup strides its key)
  HIP_TRY(c, lcdev::launch_widen32(d_ops32, d_key_off, d_key_base, n_keys, 4 * (*nrec / n_keys + 1),
                                   d.d_ops.p, st));
  return 0;
}

}  // namespace

// lc_check_device_ex (48-byte records) and lc_check_device32 (rec32: 24-byte
// records and key bases), on the context's first device.  `who` names the
// entry point in its errors.
// Hot paths: a call without lc_aux outputs or LC_FLAG_WHOLE_GPU issues
// hipSetDevice and then run_device's calls, nothing else; 24-byte records
// are decided as they are (Source::ops32) and widened only at a handoff.
int lcrt::check_device(lc_ctx *c, const char *who, const void *ops, bool rec32, const int64_t *d_key_off,
                       const int64_t *d_key_base, int64_t n_keys, const lc_opts *opts, lc_key_result *d_out,
                       void *stream, const lc_aux *aux) {
  const auto t0 = std::chrono::steady_clock::now();
  c->stats = lc_stats{};
  for (Dev &d : c->devs) {
    d.counted = lc_counted_stats{};
    d.wit = lc_witness_stats{};
    d.cwit = lc_counted_witness_stats{};
  }
  if (n_keys < 0 || (n_keys > 0 && (!ops || !d_key_off || !d_out))) {
    set_err(c, std::string(who) + ": null buffer or negative n_keys");
    return -EINVAL;
  }
  const unsigned align = rec32 ? 8 : 16;
  if (reinterpret_cast<uintptr_t>(ops) % align) {
    set_err(c, std::string(who) + ": ops must be " + std::to_string(align) + "-byte aligned");
    return -EINVAL;
  }
  lcdev::KParams p;
  int rc = opts_to_params(c, opts, &p);
  if (rc) return rc;
  Dev &d = c->devs[0];
  HIP_TRY(c, hipSetDevice(d.id));
  hipStream_t st = stream ? static_cast<hipStream_t>(stream) : d.stream;
  const int64_t flags = opts ? opts->flags : 0;
  const bool want_wit = aux && aux->witness && aux->witness_kind;
  const bool want_cert = aux && aux->certificate;
  const lc_op32 *d_ops32 = rec32 ? static_cast<const lc_op32 *>(ops) : nullptr;
  // d_ops points at the record of index d_key_off[0]; the kernels read that
  // base themselves, so a key_off slice of a larger array may be passed.
  const lc_op *d_ops = rec32 ? nullptr : static_cast<const lc_op *>(ops);
  AuxOut ao;
  Source src;
  if (rec32 && n_keys > 0 && !(aux && (aux->witness || aux->certificate)) &&
      !(flags & (LC_FLAG_NO_FAST_PATH | LC_FLAG_WHOLE_GPU))) {
    // decided from the 24-byte records as they are; the 48-byte form (and
    // the record count it needs, read from device memory) only if a key is
    // handed over to the later tiers
    src.ops32 = d_ops32;
    src.base32 = d_key_base;
    src.widen = [&](const lc_op **out) -> int {
      int64_t nrec = 0;
      if (int e = widen_device32(c, d, d_ops32, d_key_off, d_key_base, n_keys, st, &nrec)) return e;
      *out = d.d_ops.p;
      return 0;
    };
  } else if (n_keys > 0) {
    // the record count lives in device memory
    if (rec32) {
      if (int e = widen_device32(c, d, d_ops32, d_key_off, d_key_base, n_keys, st, &ao.n_records))
        return e;
      d_ops = d.d_ops.p;
    } else if (want_wit || want_cert) {
      if (int e = device_record_count(c, d, d_key_off, n_keys, st, &ao.n_records)) return e;
    }
    if (want_wit) {
      ao.wit = aux->witness;
      ao.kind = aux->witness_kind;
    }
    if (want_cert) {
      ao.cert = aux->certificate;
      ao.cset = aux->certificate_set;
      if (!ao.cset) {  // the position sets still need a home on the device
        if (int e = ensure(c, d.d_cset, sizeof(int32_t) * (size_t)ao.n_records)) return e;
        ao.cset = d.d_cset.p;
      }
    }
  }
  rc = run_device(c, d, d_ops, d_key_off, n_keys, p, d_out, st, flags, ao, src);
  if (!rc) rc = run_certificates(c, d, d_ops, d_key_off, n_keys, p, d_out, st, ao);
  if (!rc && (flags & LC_FLAG_WHOLE_GPU) && n_keys > 0)
    rc = whole_gpu_device(c, d_ops, d_key_off, n_keys, opts, d_out, want_cert ? aux->certificate : nullptr,
                          st);
  fill_stats(c->stats, d);
  c->stats.n_keys = n_keys;
  c->stats.n_ops = -1;  // not read back from device memory
  c->stats.n_devices = 1;
  c->stats.total_ms = std::chrono::duration<double, std::milli>(
                          std::chrono::steady_clock::now() - t0).count();
  return rc;
}

extern "C" {

int lc_abi_version(void) { return LC_ABI_VERSION; }

void lc_default_opts(lc_opts *o) {
  if (!o) return;
  o->init_version = 0;
  o->init_value = LC_NIL;
  o->max_configs_per_key = 0;
  o->time_budget_ms = 0;
  o->flags = 0;
}

// The id is also findable in the file without loading it ("LC_BUILD_ID:"
// marker): tests/conftest.py checks it before anything loads a HIP runtime.
__attribute__((used)) static const char kBuildTag[] = "LC_BUILD_ID:" LC_BUILD_ID;
const char *lc_build_id(void) { return kBuildTag + 12; }

int lc_open(uint32_t device_mask, lc_ctx **out) {
  if (!out) return -EINVAL;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return -ENODEV;
  // LC_VIRTUAL_DEVICES=k: k device contexts on the first selected GPU (tests
  // of the multi-device fan-out on a one-GPU box)
  const char *venv = getenv("LC_VIRTUAL_DEVICES");
  const int virt = venv ? std::max(0, std::min(32, atoi(venv))) : 0;
  lc_ctx *c = new lc_ctx();
  for (int i = 0; i < n && i < 32; i++) {
    if (device_mask && !(device_mask & (1u << i))) continue;
    for (int v = 0; v < (virt >= 2 ? virt : 1); v++) {
      Dev d;
      d.id = i;
      bool ok = hipSetDevice(i) == hipSuccess;
      for (hipStream_t *s : {&d.stream, &d.cst, &d.cst2})
        ok = ok && hipStreamCreateWithFlags(s, hipStreamNonBlocking) == hipSuccess;
      for (hipEvent_t *e : {&d.e0, &d.e1, &d.e2, &d.ef, &d.eg, &d.el, &d.eh0, &d.eh1, &d.es})
        ok = ok && hipEventCreateWithFlags(e, kEventFlags) == hipSuccess;
      if (!ok ||
          hipMalloc(reinterpret_cast<void **>(&d.d_status), sizeof(lcdev::KStatus)) != hipSuccess ||
          hipHostMalloc(reinterpret_cast<void **>(&d.h_status), sizeof(lcdev::KStatus), 0) != hipSuccess ||
          hipHostMalloc(reinterpret_cast<void **>(&d.h_handoff), 2 * sizeof(int32_t),
                        hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
          hipHostGetDevicePointer(reinterpret_cast<void **>(&d.h_handoff_dev), d.h_handoff, 0) != hipSuccess ||
          hipHostMalloc(reinterpret_cast<void **>(&d.h_done), 64,
                        hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
          hipHostGetDevicePointer(reinterpret_cast<void **>(&d.h_done_dev), d.h_done, 0) != hipSuccess) {
        c->devs.push_back(d);  // lc_close frees what was created
        lc_close(c);
        return -ENODEV;
      }
      // pinned memory may be reused from a closed context: the completion
      // word must not already hold this context's first sequence number
      __atomic_store_n(d.h_done, 0u, __ATOMIC_RELEASE);
      __atomic_store_n(d.h_handoff, 0, __ATOMIC_RELEASE);
      __atomic_store_n(d.h_handoff + 1, 0, __ATOMIC_RELEASE);
      c->devs.push_back(d);
    }
    if (virt >= 2) break;
  }
  if (c->devs.empty()) {
    delete c;
    return -ENODEV;
  }
  *out = c;
  return 0;
}

void lc_close(lc_ctx *c) {
  if (!c) return;
  if (!c->devs.empty()) {
    // the side checkers' states live on the first device
    (void)hipSetDevice(c->devs[0].id);
    if (c->devs[0].stream) (void)hipStreamSynchronize(c->devs[0].stream);
    release(c->evs);
    release(c->sfs);
    release(c->aps);
    release(c->wrs);
    release(c->wts);
    release(c->pfs);
    release(c->scs);
    release(c->cys);
  }
  for (auto &f : c->fxs) lc_fx_close(f.first);
  if (c->fx_all) lc_fx_close(c->fx_all);
  for (auto &pr : c->pinned) (void)hipHostUnregister(const_cast<char *>(pr.first));
  for (Dev &d : c->devs) {
    (void)hipSetDevice(d.id);
    (void)res_stop(c, d);
    if (d.rst) (void)hipStreamDestroy(d.rst);
    if (d.res_d) (void)hipFree(d.res_d);
    if (d.res_h) (void)hipHostFree(d.res_h);
    if (d.stream) (void)hipStreamSynchronize(d.stream);
    // every Buf of Dev
    for (void *b : std::initializer_list<void *>{
             d.d_ops.p, d.d_off.p, d.d_out.p, d.d_ovf.p, d.d_ovf2.p, d.d_jit.p, d.d_flags.p, d.d_jit2.p,
             d.d_gap2.p, d.d_gws.p, d.d_cex.p, d.d_ws.p, d.d_wit.p, d.d_kind.p, d.d_cert.p, d.d_cset.p,
             d.d_cws.p, d.d_ops32.p, d.d_base.p, d.d_wst.p})
      if (b) (void)hipFree(b);
    if (d.d_status) (void)hipFree(d.d_status);
    if (d.h_status) (void)hipHostFree(d.h_status);
    if (d.h_handoff) (void)hipHostFree(d.h_handoff);
    if (d.h_done) (void)hipHostFree(d.h_done);
    if (d.h_stage) (void)hipHostFree(d.h_stage);
    for (hipEvent_t e : {d.e0, d.e1, d.e2, d.ef, d.eg, d.el, d.eh0, d.eh1, d.es})
      if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : d.cev) (void)hipEventDestroy(e);
    for (hipStream_t cs : {d.cst, d.cst2})
      if (cs) {
        (void)hipStreamSynchronize(cs);
        (void)hipStreamDestroy(cs);
      }
    if (d.stream) (void)hipStreamDestroy(d.stream);
  }
  delete c;
}

const char *lc_last_error(lc_ctx *c) { return c ? c->err.c_str() : "null context"; }

int lc_last_stats(lc_ctx *c, lc_stats *out) {
  if (!c || !out) return -EINVAL;
  // a call that returned on the completion signal: its pass's event time
  // (single-device calls only take that path)
  if (c->devs[0].timing_pending) {
    settle_timing(c, c->devs[0]);
    c->stats.fast_kernel_ms = c->devs[0].fast_ms;
    c->stats.kernel_ms = c->devs[0].kernel_ms;
  }
  // the keys the crash-light decision took in a fused call, copied lazily
  for (Dev &d : c->devs) {
    const int64_t n = settle_status(d);
    if (n > 0) c->stats.n_gap_keys += n;
  }
  *out = c->stats;
  return 0;
}

int lc_quiesce(lc_ctx *c) {
  if (!c) return -EINVAL;
  for (Dev &d : c->devs) {
    if (!d.res_grid) continue;
    (void)hipSetDevice(d.id);
    if (int e = res_stop(c, d)) return e;
  }
  return 0;
}

int lc_last_counted_stats(lc_ctx *c, lc_counted_stats *out) {
  if (!c || !out) return -EINVAL;
  lc_counted_stats s{};
  for (const Dev &d : c->devs) {
    s.n_keys += d.counted.n_keys;
    s.n_decided += d.counted.n_decided;
    s.n_unfit += d.counted.n_unfit;
    s.kernel_ms += d.counted.kernel_ms;
  }
  *out = s;
  return 0;
}

int lc_last_witness_stats(lc_ctx *c, lc_witness_stats *out) {
  if (!c || !out) return -EINVAL;
  lc_witness_stats s{};
  for (const Dev &d : c->devs) {
    s.n_keys += d.wit.n_keys;
    s.n_found += d.wit.n_found;
    s.n_budget += d.wit.n_budget;
    s.n_window += d.wit.n_window;
    s.nodes += d.wit.nodes;
    s.cache_hits += d.wit.cache_hits;
    s.kernel_ms += d.wit.kernel_ms;
  }
  *out = s;
  return 0;
}

int lc_last_counted_witness_stats(lc_ctx *c, lc_counted_witness_stats *out) {
  if (!c || !out) return -EINVAL;
  lc_counted_witness_stats s{};
  for (const Dev &d : c->devs) {
    s.n_keys += d.cwit.n_keys;
    s.n_found += d.cwit.n_found;
    s.n_budget += d.cwit.n_budget;
    s.n_unfit += d.cwit.n_unfit;
    s.nodes += d.cwit.nodes;
    s.cache_hits += d.cwit.cache_hits;
    s.kernel_ms += d.cwit.kernel_ms;
  }
  *out = s;
  return 0;
}

int lc_last_totals(lc_ctx *c, lc_totals *out, int32_t reset) {
  if (!c || !out) return -EINVAL;
  lc_totals t{};
  for (Dev &d : c->devs) {
    settle_timing(c, d);
    t.calls += d.tot.calls;
    t.timed_calls += d.tot.timed_calls;
    t.fast_kernel_ms += d.tot.fast_kernel_ms;
    t.kernel_ms += d.tot.kernel_ms;
    if (reset) d.tot = lc_totals{};
  }
  *out = t;
  return 0;
}

int lc_last_device_stats(lc_ctx *c, int32_t i, lc_device_stats *out) {
  if (!c || !out || i < 0 || i >= (int32_t)c->devs.size()) return -EINVAL;
  *out = c->devs[(size_t)i].last;
  return 0;
}

int lc_host_register(lc_ctx *c, const void *ptr, uint64_t bytes) {
  if (!c || !ptr || !bytes) return -EINVAL;
  std::lock_guard<std::mutex> g(c->pin_mu);
  // portable: page-locked for every device of the process (the fan-out's
  // threads copy from it to each GPU of the context)
  const hipError_t e = hipHostRegister(const_cast<void *>(ptr), (size_t)bytes,
                                       hipHostRegisterPortable);
  if (e != hipSuccess) {
    set_err(c, std::string("hipHostRegister: ") + hipGetErrorString(e));
    return -EIO;
  }
  c->pinned.emplace_back(static_cast<const char *>(ptr), bytes);
  return 0;
}

int lc_host_unregister(lc_ctx *c, const void *ptr) {
  if (!c || !ptr) return -EINVAL;
  std::lock_guard<std::mutex> g(c->pin_mu);
  for (size_t i = 0; i < c->pinned.size(); i++)
    if (c->pinned[i].first == ptr) {
      const hipError_t e = hipHostUnregister(const_cast<void *>(ptr));
      c->pinned.erase(c->pinned.begin() + (long)i);
      if (e != hipSuccess) {
        set_err(c, std::string("hipHostUnregister: ") + hipGetErrorString(e));
        return -EIO;
      }
      return 0;
    }
  set_err(c, "lc_host_unregister: pointer not registered with this context");
  return -EINVAL;
}

int lc_last_call_profile(lc_ctx *c, lc_call_profile *out) {
  if (!c || !out) return -EINVAL;
  *out = c->prof;
  return 0;
}

int lc_check_device_ex(lc_ctx *c, const lc_op *d_ops, const int64_t *d_key_off,
                       int64_t n_keys, const lc_opts *opts, lc_key_result *d_out,
                       void *stream, const lc_aux *aux) {
  if (!c) return -EINVAL;
  return check_device(c, "lc_check_device", d_ops, false, d_key_off, nullptr, n_keys, opts, d_out,
                      stream, aux);
}

int lc_check_device(lc_ctx *c, const lc_op *d_ops, const int64_t *d_key_off,
                    int64_t n_keys, const lc_opts *opts, lc_key_result *d_out,
                    void *stream) {
  return lc_check_device_ex(c, d_ops, d_key_off, n_keys, opts, d_out, stream, nullptr);
}

int lc_check_device32(lc_ctx *c, const lc_op32 *d_ops, const int64_t *d_key_off,
                      const int64_t *d_key_base, int64_t n_keys, const lc_opts *opts,
                      lc_key_result *d_out, void *stream, const lc_aux *aux) {
  if (!c) return -EINVAL;
  return check_device(c, "lc_check_device32", d_ops, true, d_key_off, d_key_base, n_keys, opts, d_out,
                      stream, aux);
}

}  // extern "C"
