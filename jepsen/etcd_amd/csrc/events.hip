// events.hip — jepsen.independent's per-key split and knossos's history
// completion on the device (include/lincheck_events.h has the rules), and the
// same rules on the host (lc_events_pack_host).
//
// Kernels, in launch order:
//   count    validates every event and counts the client events of each key
//            (lanes of a wave with the same key issue one atomic add)
//   scan     exclusive scan of the counts: the keys' segments
//   scatter  writes each client event's position into its key's segment, by
//            an atomic ticket per key (unordered)
//   pair     one workgroup per key: sorts the segment's positions (in LDS, or
//            in global memory for a key above kLdsEvents), which is both the
//            subhistory order and the records' call order; then wave 0 walks
//            it in 64-event chunks and gives every invoke its completion
//   scan     exclusive scan of the keys' record counts: key_off
//   emit     one workgroup per key: ordered compaction of the surviving
//            invokes into lc_op32 records, completion[] and key_base
// With one key there is no split: the subhistory is the event array itself
// (skipped events included, which the walk passes over), so count only
// validates, and scan / scatter / the sort do not run.
// Every loop is bounded by an event, key or table count; no kernel waits on
// memory another workgroup writes.
#include <errno.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <unordered_map>
#include <vector>

#include "../../../include/lincheck.h"
#include "events.h"
#include "wave.h"

namespace lcev {
namespace {

constexpr uint32_t kTypeMask = 0xFF;

// Rules 3 and 4: the record of invoke `iv` (at position ipos) with its
// completion `cp` (at cpos; has_cp false: none).  Never called for a FAIL
// pair.  (Field by field, no pointer to either event: they stay in registers.)
__host__ __device__ inline void make_record(const lc_event &iv, int64_t ipos, bool has_cp, const lc_event &cp,
                                            int64_t cpos, int64_t base, lc_op32 *o, int32_t *completion) {
  const bool ok = has_cp && (cp.tf & kTypeMask) == LC_EV_OK;
  const uint32_t src_tf = ok ? cp.tf : iv.tf;
  const uint32_t fkw = (iv.tf >> 8) & 0xFF;
  const bool mismatch = ok && ((cp.tf >> 8) & 0xFF) != fkw;
  const bool unknown = fkw >= LC_EV_F_UNKNOWN || ((src_tf >> 16) & 1) || mismatch;
  o->f = unknown ? LC_EV_F_UNKNOWN : (int32_t)fkw;
  o->value = unknown ? -1 : ok ? cp.value : iv.value;
  o->expected = unknown ? -1 : ok ? cp.expected : iv.expected;
  o->version = unknown ? -1 : ok ? cp.version : iv.version;
  o->call = (uint32_t)(ipos - base);
  o->ret = ok ? (uint32_t)(cpos - base) : LC_INF32;
  *completion = has_cp ? (int32_t)cpos : -1;
}

// Rule 7 for one event: 0 fine, 1 bad key, 2 bad type.
__host__ __device__ inline int event_error(int32_t key, uint32_t tf, int64_t n_keys) {
  if (key < -1 || key >= n_keys) return 1;
  return (tf & kTypeMask) > LC_EV_INFO ? 2 : 0;
}

__device__ __forceinline__ uint64_t lanes_lt(int lane) { return (1ull << lane) - 1; }

// ---- count / scatter --------------------------------------------------------
// At most this many rounds of "the first remaining lane's key": a wave whose
// lanes hold more distinct keys than that sends the rest one add per lane
// (distinct keys are distinct addresses: nothing queues there).
constexpr int kKeyRounds = 8;

__global__ __launch_bounds__(kThreads) void ev_count_kernel(const lc_event *ev, int64_t n, int64_t n_keys,
                                                            int32_t *cnt, Status *status) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  int n_client = 0, n_invoke = 0;
  // (every lane of a wave runs the same number of rounds: ballots inside)
  for (int64_t b = (int64_t)blockIdx.x * kThreads + (threadIdx.x & ~63); b < n; b += stride) {
    const int64_t i = b + lane;
    int32_t key = -1;
    uint32_t tf = 0;
    if (i < n) {
      key = ev[i].key;
      tf = ev[i].tf;
      const int e = event_error(key, tf, n_keys);
      if (e) {
        atomicMax(&status->err, e);
        atomicMax(&status->err_pos, (int32_t)i);
        key = -1;
      }
    }
    const bool client = key >= 0;
    n_client += client;
    n_invoke += client && (tf & kTypeMask) == LC_EV_INVOKE;
    if (!cnt) continue;
    uint64_t todo = __ballot(client);
    for (int r = 0; r < kKeyRounds && todo; r++) {
      const int l = lcdev::first_lane(todo);
      const int32_t k = __shfl(key, l);
      const uint64_t m = __ballot(client && key == k);
      if (lane == l) atomicAdd(&cnt[k], __popcll(m));
      todo &= ~m;
    }
    if (client && ((todo >> lane) & 1)) atomicAdd(&cnt[key], 1);
  }
  // one add per workgroup (the grid is capped: a few thousand in all)
  __shared__ int s_client, s_invoke;
  if (threadIdx.x == 0) s_client = s_invoke = 0;
  __syncthreads();
  n_client = lcdev::wave_prefix_sum(n_client, lane);
  n_invoke = lcdev::wave_prefix_sum(n_invoke, lane);
  if (lane == 63) {
    atomicAdd(&s_client, n_client);
    atomicAdd(&s_invoke, n_invoke);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    if (s_client) atomicAdd((unsigned long long *)&status->n_client, (unsigned long long)s_client);
    if (s_invoke) atomicAdd((unsigned long long *)&status->n_invoke, (unsigned long long)s_invoke);
  }
}

__global__ __launch_bounds__(kThreads) void ev_scatter_kernel(const lc_event *ev, int64_t n, int64_t n_keys,
                                                              const int64_t *seg_off, int32_t *cursor,
                                                              uint32_t *seg) {
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * kThreads;
  for (int64_t b = (int64_t)blockIdx.x * kThreads + (threadIdx.x & ~63); b < n; b += stride) {
    const int64_t i = b + lane;
    int32_t key = -1;
    if (i < n) {
      key = ev[i].key;
      if (event_error(key, ev[i].tf, n_keys)) key = -1;  // as count saw it
    }
    const bool client = key >= 0;
    int32_t slot = 0;
    uint64_t todo = __ballot(client);
    for (int r = 0; r < kKeyRounds && todo; r++) {
      const int l = lcdev::first_lane(todo);
      const int32_t k = __shfl(key, l);
      const uint64_t m = __ballot(client && key == k);
      int32_t first = 0;
      if (lane == l) first = atomicAdd(&cursor[k], __popcll(m));
      first = __shfl(first, l);
      if (client && key == k) slot = first + __popcll(m & lanes_lt(lane));
      todo &= ~m;
    }
    if (client && ((todo >> lane) & 1)) slot = atomicAdd(&cursor[key], 1);
    // slot < cnt[key]: count added one per client event of the key
    if (client) seg[seg_off[key] + slot] = (uint32_t)i;
  }
}

// ---- scan -------------------------------------------------------------------
// out[0 .. n] = exclusive scan of in[0 .. n) (out[n]: the total), by one
// workgroup; optionally the sums of a / b into *sum_a / *sum_b and the total
// into *total.  Sums stay below 2^31 (they count events).
constexpr int kScanThreads = 1024;
__global__ __launch_bounds__(kScanThreads) void ev_scan_kernel(const int32_t *in, int64_t n, int64_t *out,
                                                               const int32_t *a, const int32_t *b,
                                                               int64_t *total, int64_t *sum_a,
                                                               int64_t *sum_b) {
  __shared__ int s_w[kScanThreads / 64];
  __shared__ unsigned long long s_a, s_b;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x == 0) s_a = s_b = 0;
  int64_t running = 0;
  unsigned long long my_a = 0, my_b = 0;
  for (int64_t t0 = 0; t0 < n; t0 += kScanThreads) {
    const int64_t i = t0 + threadIdx.x;
    const int v = i < n ? in[i] : 0;
    if (i < n && a) my_a += (unsigned)a[i];
    if (i < n && b) my_b += (unsigned)b[i];
    const int incl = lcdev::wave_prefix_sum(v, lane);
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kScanThreads / 64; w++) {
      const int x = s_w[w];
      before += w < wave ? x : 0;
      all += x;
    }
    if (i < n) out[i] = running + before + incl - v;
    running += all;
    __syncthreads();
  }
  if (my_a) atomicAdd(&s_a, my_a);
  if (my_b) atomicAdd(&s_b, my_b);
  __syncthreads();
  if (threadIdx.x == 0) {
    out[n] = running;
    if (total) *total = running;
    if (sum_a) *sum_a = (int64_t)s_a;
    if (sum_b) *sum_b = (int64_t)s_b;
  }
}

// ---- sort -------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld(const uint32_t *p, bool global) {
  // global memory: past the L1, which other waves of the workgroup write through
  return global ? __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : *p;
}
__device__ __forceinline__ void st(uint32_t *p, uint32_t v, bool global) {
  if (global)
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  else
    *p = v;
}
__device__ __forceinline__ void cswap(uint32_t *a, uint32_t i, uint32_t j, bool global) {
  const uint32_t x = ld(a + i, global), y = ld(a + j, global);
  if (x > y) {
    st(a + i, y, global);
    st(a + j, x, global);
  }
}
// Ascending bitonic sort of a[0 .. n) by the whole workgroup.  Every
// comparison puts the smaller value at the lower index (each merge starts
// with a mirrored step), so the elements n .. 2^k-1 a power-of-two network
// needs stand for +infinity, never move, and are never touched.  (Unsigned:
// n < 2^31, so the network's size is at most 2^31.)
__device__ __forceinline__ void bitonic_sort(uint32_t *a, uint32_t n, bool global) {
  uint32_t p2 = 1;
  while (p2 < n) p2 <<= 1;
  const uint32_t half = p2 >> 1;
  for (uint32_t k = 2; k <= p2 && k; k <<= 1) {
    const uint32_t hk = k >> 1, sh = __builtin_ctz(hk);
    for (uint32_t t = threadIdx.x; t < half; t += kThreads) {
      const uint32_t blk = (t >> sh) * k, o = t & (hk - 1);
      const uint32_t i = blk + o, j = blk + k - 1 - o;
      if (j < n) cswap(a, i, j, global);
    }
    __syncthreads();
    for (uint32_t s = k >> 2; s >= 1; s >>= 1) {
      for (uint32_t t = threadIdx.x; t < half; t += kThreads) {
        const uint32_t i = ((t & ~(s - 1)) << 1) | (t & (s - 1)), j = i + s;
        if (j < n) cswap(a, i, j, global);
      }
      __syncthreads();
    }
  }
}

// ---- the process table ------------------------------------------------------
// process -> the last event of that process seen so far, as slot words
// (uint32) process << 32 | val with val = (index in the segment + 1) << 1 |
// is-invoke, so a slot in use is never 0.  Open addressing, linear probing,
// no deletions.  The first kLdsProcs distinct processes of a key live in LDS
// (kLdsSlots slots), the further ones in the key's part of `gtab` (twice its
// event count in slots, zeroed by the wave when first needed).
constexpr int kLdsSlots = 2 * kLdsProcs;
constexpr int kLdsShift = 21;  // 32 - log2(kLdsSlots)
static_assert((1 << (32 - kLdsShift)) == kLdsSlots, "kLdsShift");
constexpr uint32_t kHashMul = 2654435761u;

__device__ __forceinline__ uint64_t gl_load(const unsigned long long *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- pair -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ev_pair_kernel(Ws w) {
  __shared__ uint32_t s_pos[kLdsEvents];
  __shared__ unsigned long long s_tab[kLdsSlots];
  const bool identity = w.k == 1;
  const int64_t key = blockIdx.x;
  const int64_t off = identity ? 0 : w.seg_off[key];
  const int cnt = (int)(identity ? w.n : w.seg_off[key + 1] - off);
  const int lane = threadIdx.x & 63;
  int32_t *match = w.match + off;
  uint32_t *seg = identity ? nullptr : w.seg + off;

  // (64-bit loop counters: cnt may be within a stride of 2^31)
  for (int64_t i = threadIdx.x; i < cnt; i += kThreads) match[i] = -1;
  for (int i = threadIdx.x; i < kLdsSlots; i += kThreads) s_tab[i] = 0;
  bool big = false;
  if (!identity && cnt > 1) {
    if (cnt <= kLdsEvents) {
      for (int i = threadIdx.x; i < cnt; i += kThreads) s_pos[i] = seg[i];  // cnt <= kLdsEvents
      __syncthreads();
      bitonic_sort(s_pos, cnt, false);
      for (int i = threadIdx.x; i < cnt; i += kThreads) seg[i] = s_pos[i];
    } else {
      big = true;
      __syncthreads();
      bitonic_sort(seg, cnt, true);
    }
  }
  __syncthreads();
  if (threadIdx.x >= 64) return;

  // wave 0: the walk.  Uniform state: the distinct processes seen, whether
  // the global table has been zeroed.
  unsigned long long *gtab = w.gtab + 2 * off;
  const uint64_t gslots = 2 * (uint64_t)cnt;
  int n_procs = 0;
  bool gl_ready = false;
  int n_inv = 0, n_fail = 0, n_ign = 0;
  for (int64_t c0 = 0; c0 < cnt; c0 += 64) {
    const int i = (int)c0 + lane;  // used only when < cnt
    bool act = i < cnt;
    int32_t proc = 0;
    uint32_t type = 0;
    if (act) {
      const uint32_t pos = identity ? (uint32_t)i : ld(seg + i, big);
      const lc_event *e = w.ev + pos;
      proc = e->process;
      type = e->tf & kTypeMask;
      if (identity) act = e->key >= 0 && !event_error(e->key, e->tf, w.k);
    }
    const bool inv = act && type == LC_EV_INVOKE;
    // the lanes of my process
    uint64_t todo = __ballot(act), mine = 0;
    while (todo) {
      const int l = lcdev::first_lane(todo);
      const int32_t p = __shfl(proc, l);
      const uint64_t m = __ballot(act && proc == p);
      if (act && proc == p) mine = m;
      todo &= ~m;
    }
    const uint64_t lower = mine & lanes_lt(lane);
    const int pl = lower ? 63 - __builtin_clzll(lower) : lane;
    const int pl_inv = __shfl((int)inv, pl);
    const int last = act ? 63 - __builtin_clzll(mine) : lane;
    const int last_inv = __shfl((int)inv, last);
    bool has_pred = act && lower != 0, pred_inv = pl_inv != 0;
    int pred_idx = (int)c0 + pl;

    // the first lane of each process: its predecessor from the table, and
    // the process's last event of this chunk into the table
    const bool first = act && lower == 0;
    const uint64_t word = (uint64_t)(uint32_t)proc << 32 | ((uint32_t)(c0 + last + 1) << 1) |
                          (uint32_t)last_inv;
    bool found = false;
    if (first) {
      uint32_t h = ((uint32_t)proc * kHashMul) >> kLdsShift;
      for (int probe = 0; probe < kLdsSlots; probe++) {
        const uint64_t e = s_tab[h];
        if (e == 0) break;
        if ((uint32_t)(e >> 32) == (uint32_t)proc) {
          found = true;
          has_pred = true;
          pred_inv = e & 1;
          pred_idx = (int)((uint32_t)e >> 1) - 1;
          s_tab[h] = word;
          break;
        }
        h = (h + 1) & (kLdsSlots - 1);
      }
      if (!found && gl_ready) {
        uint64_t g = ((uint64_t)((uint32_t)proc * kHashMul) * gslots) >> 32;
        for (uint64_t probe = 0; probe < gslots; probe++) {
          const uint64_t e = gl_load(gtab + g);
          if (e == 0) break;
          if ((uint32_t)(e >> 32) == (uint32_t)proc) {
            found = true;
            has_pred = true;
            pred_inv = e & 1;
            pred_idx = (int)((uint32_t)e >> 1) - 1;
            __hip_atomic_store(gtab + g, (unsigned long long)word, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            break;
          }
          g = g + 1 == gslots ? 0 : g + 1;
        }
      }
    }
    // processes new to the tables, ranked: LDS up to its capacity, then global
    const uint64_t fresh = __ballot(first && !found);
    if (fresh) {
      const int n_fresh = __popcll(fresh);
      if (n_procs + n_fresh > kLdsProcs && !gl_ready) {
        for (uint64_t g = lane; g < gslots; g += 64)
          __hip_atomic_store(gtab + g, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        lcdev::wave_fence();
        gl_ready = true;
      }
      if (first && !found) {
        const int rank = n_procs + __popcll(fresh & lanes_lt(lane));
        if (rank < kLdsProcs) {
          uint32_t h = ((uint32_t)proc * kHashMul) >> kLdsShift;
          for (int probe = 0; probe < kLdsSlots; probe++) {
            if (atomicCAS(&s_tab[h], 0ull, (unsigned long long)word) == 0) break;
            h = (h + 1) & (kLdsSlots - 1);
          }
        } else {
          uint64_t g = ((uint64_t)((uint32_t)proc * kHashMul) * gslots) >> 32;
          for (uint64_t probe = 0; probe < gslots; probe++) {
            if (atomicCAS(gtab + g, 0ull, (unsigned long long)word) == 0) break;
            g = g + 1 == gslots ? 0 : g + 1;
          }
        }
      }
      n_procs += n_fresh;
    }
    lcdev::wave_fence();

    const bool comp = act && type != LC_EV_INVOKE;
    const bool paired = comp && has_pred && pred_inv;
    if (paired) match[pred_idx] = type == LC_EV_FAIL ? -2 : i;
    n_inv += __popcll(__ballot(inv));
    n_fail += __popcll(__ballot(paired && type == LC_EV_FAIL));
    n_ign += __popcll(__ballot(comp && !paired));
  }
  if (lane == 0) {
    w.nops[key] = n_inv - n_fail;
    w.nfail[key] = n_fail;
    w.nign[key] = n_ign;
    if (big) atomicAdd((unsigned long long *)&w.status->n_big, 1ull);
  }
}

// ---- emit -------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void ev_emit_kernel(Ws w) {
  __shared__ int s_w[kThreads / 64];
  __shared__ long long s_base;
  const bool identity = w.k == 1;
  const int64_t key = blockIdx.x;
  const int64_t o0 = w.key_off[key], o1 = w.key_off[key + 1];
  if (o1 == o0) {
    if (threadIdx.x == 0) w.key_base[key] = 0;
    return;
  }
  const int64_t off = identity ? 0 : w.seg_off[key];
  const int cnt = (int)(identity ? w.n : w.seg_off[key + 1] - off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t *match = w.match + off;
  const uint32_t *seg = identity ? nullptr : w.seg + off;
  int64_t running = 0;
  for (int64_t t0 = 0; t0 < cnt; t0 += kThreads) {
    const int64_t i = t0 + threadIdx.x;
    bool surv = false;
    int64_t pos = 0;
    int32_t m = -1;
    lc_event iv{};
    if (i < cnt) {
      pos = identity ? i : seg[i];
      iv = w.ev[pos];
      const bool client = !identity || (iv.key >= 0 && !event_error(iv.key, iv.tf, w.k));
      if (client && (iv.tf & kTypeMask) == LC_EV_INVOKE) {
        m = match[i];
        surv = m != -2;
      }
    }
    const uint64_t b = __ballot(surv);
    if (lane == 0) s_w[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int x = 0; x < kThreads / 64; x++) {
      before += x < wave ? s_w[x] : 0;
      all += s_w[x];
    }
    const int64_t idx = running + before + lcdev::lanes_below(b);
    if (surv && idx == 0) s_base = pos;  // the key's first call: once per key
    __syncthreads();
    if (surv && o0 + idx < o1) {
      const int64_t base = s_base;
      lc_event cp{};
      int64_t cpos = -1;
      if (m >= 0) {
        cpos = identity ? m : seg[m];
        cp = w.ev[cpos];
      }
      lc_op32 o;
      int32_t c;
      make_record(iv, pos, m >= 0, cp, cpos, base, &o, &c);
      w.ops32[o0 + idx] = o;
      w.completion[o0 + idx] = c;
    }
    running += all;
  }
  if (threadIdx.x == 0) w.key_base[key] = s_base;
}

}  // namespace

hipError_t launch_events(const Ws &w, hipStream_t st) {
  if (w.k == 0 || w.n == 0) {
    // nothing to split; events with no key to belong to are still validated
    if (w.n > 0) {
      const int grid = (int)std::min<int64_t>((w.n + kThreads - 1) / kThreads, 2048);
      hipLaunchKernelGGL(ev_count_kernel, dim3(grid), dim3(kThreads), 0, st, w.ev, w.n, w.k, nullptr,
                         w.status);
    }
    if (hipError_t e = hipMemsetAsync(w.key_off, 0, sizeof(int64_t) * (size_t)(w.k + 1), st)) return e;
    if (w.k > 0)
      if (hipError_t e = hipMemsetAsync(w.key_base, 0, sizeof(int64_t) * (size_t)w.k, st)) return e;
    return hipGetLastError();
  }
  const bool identity = w.k == 1;
  const int grid = (int)std::min<int64_t>((w.n + kThreads - 1) / kThreads, 2048);
  hipLaunchKernelGGL(ev_count_kernel, dim3(grid), dim3(kThreads), 0, st, w.ev, w.n, w.k,
                     identity ? nullptr : w.cnt, w.status);
  if (!identity) {
    hipLaunchKernelGGL(ev_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, w.cnt, w.k, w.seg_off,
                       nullptr, nullptr, nullptr, nullptr, nullptr);
    hipLaunchKernelGGL(ev_scatter_kernel, dim3(grid), dim3(kThreads), 0, st, w.ev, w.n, w.k, w.seg_off,
                       w.cursor, w.seg);
  }
  hipLaunchKernelGGL(ev_pair_kernel, dim3((unsigned)w.k), dim3(kThreads), 0, st, w);
  hipLaunchKernelGGL(ev_scan_kernel, dim3(1), dim3(kScanThreads), 0, st, w.nops, w.k, w.key_off, w.nfail,
                     w.nign, &w.status->n_ops, &w.status->n_fail, &w.status->n_ignored);
  hipLaunchKernelGGL(ev_emit_kernel, dim3((unsigned)w.k), dim3(kThreads), 0, st, w);
  return hipGetLastError();
}

}  // namespace lcev

extern "C" {

int lc_events_limits(lc_events_limit_info *out) {
  if (!out) return -EINVAL;
  out->max_lds_events = lcev::kLdsEvents;
  out->lds_process_capacity = lcev::kLdsProcs;
  return 0;
}

int lc_events_pack_host(const lc_event *ev, int64_t n_events, int64_t n_keys, lc_events_out *out) {
  if (n_events < 0 || n_keys < 0 || n_events >= (int64_t(1) << 31) || n_keys >= (int64_t(1) << 31) ||
      (n_events > 0 && !ev) || !out || !out->key_off || (n_keys > 0 && !out->key_base))
    return -EINVAL;
  int64_t n_invoke = 0;
  try {
    // the keys' subhistories: a stable counting sort of the client positions
    std::vector<int64_t> off((size_t)n_keys + 1, 0);
    for (int64_t i = 0; i < n_events; i++) {
      if (lcev::event_error(ev[i].key, ev[i].tf, n_keys)) return -EINVAL;
      if (ev[i].key < 0) continue;
      off[(size_t)ev[i].key + 1]++;
      n_invoke += (ev[i].tf & lcev::kTypeMask) == LC_EV_INVOKE;
    }
    if (out->cap < n_invoke || (n_invoke > 0 && (!out->ops32 || !out->completion))) return -EINVAL;
    for (int64_t k = 0; k < n_keys; k++) off[(size_t)k + 1] += off[(size_t)k];
    std::vector<int32_t> sub((size_t)off[(size_t)n_keys]);
    {
      std::vector<int64_t> at(off.begin(), off.end() - 1);
      for (int64_t i = 0; i < n_events; i++)
        if (ev[i].key >= 0) sub[(size_t)at[(size_t)ev[i].key]++] = (int32_t)i;
    }
    struct Open {
      int32_t invoke, completion;  // positions; completion -1: none, -2: FAIL
    };
    std::vector<Open> recs;
    std::unordered_map<int32_t, size_t> pending;  // process -> its open invoke in recs
    int64_t n_ops = 0;
    out->key_off[0] = 0;
    for (int64_t k = 0; k < n_keys; k++) {
      recs.clear();
      pending.clear();
      for (int64_t s = off[(size_t)k]; s < off[(size_t)k + 1]; s++) {
        const int32_t pos = sub[(size_t)s];
        const lc_event &e = ev[pos];
        const uint32_t type = e.tf & lcev::kTypeMask;
        if (type == LC_EV_INVOKE) {
          pending[e.process] = recs.size();
          recs.push_back({pos, -1});
        } else {
          auto it = pending.find(e.process);
          if (it == pending.end()) continue;  // no invoke before it: ignored
          recs[it->second].completion = type == LC_EV_FAIL ? -2 : pos;
          pending.erase(it);
        }
      }
      int64_t base = 0;
      bool have = false;
      for (const Open &r : recs) {
        if (r.completion == -2) continue;
        if (!have) {
          base = r.invoke;
          have = true;
        }
        lcev::make_record(ev[r.invoke], r.invoke, r.completion >= 0,
                          ev[r.completion >= 0 ? r.completion : r.invoke], r.completion, base,
                          &out->ops32[n_ops], &out->completion[n_ops]);
        n_ops++;
      }
      out->key_base[k] = base;
      out->key_off[k + 1] = n_ops;
    }
    out->n_ops = n_ops;
  } catch (const std::bad_alloc &) {
    return -ENOMEM;
  }
  return 0;
}

}  // extern "C"
