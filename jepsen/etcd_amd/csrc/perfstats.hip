// perfstats.hip — lc_perf_stats' kernels (include/lincheck_perf.h).
//
//  scan    one coalesced pass over the 16-byte records: rule 8's tests, t_max
//          and n_client (a workgroup's reduction, then one atomic each), the
//          process sort's keys and positions, the point arrays' "none".
//  sort    rocPRIM's radix sort (stable) of the positions by process; a record
//          that is no client's has the key 0xFFFFFFFF and sorts last, so the
//          client events are slots [0, n_client).
//  pairs   a workgroup takes kChunk slots at a time, kBlock per round.  A
//          round's records are gathered through the sorted positions into an
//          LDS tile with one halo slot on either side, so that the invoke in
//          a round's last slot sees its successor and the completion in its
//          first slot its predecessor, whatever wave, workgroup or chunk they
//          fall into; a slot beyond the client events, and the halo at either
//          end of them, reads as process -1, which is nobody's.  Rules 5 and 6
//          count into one table: a uint32 histogram in the LDS, flushed with
//          64-bit atomics at the workgroup's end, or global atomics directly
//          above the LDS bound.  Every slot writes (group, latency); a slot
//          that is no pair's invoke writes the group n_groups, which sorts
//          last.
//  groups  two stable radix sorts, by latency and then by group: the groups
//          in ascending order, each ascending by latency.
//  select  the slot where a group starts reads the group's count from the
//          table the pair pass counted and picks the n_q entries of rule 6.
#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>

#include "perfstats.h"

namespace lcps {

namespace {

constexpr uint32_t kNoClient = 0xFFFFFFFFu;

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
  for (int o = kWave / 2; o > 0; o >>= 1) v += __shfl_down(v, o, kWave);
  return v;
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_down(v, o, kWave);
    v = x > v ? x : v;
  }
  return v;
}

__global__ __launch_bounds__(kBlock) void ps_scan_kernel(Ws w) {
  __shared__ unsigned long long s_max[kBlock / kWave], s_cnt[kBlock / kWave];
  __shared__ int s_bad;
  if (threadIdx.x == 0) s_bad = 0;
  __syncthreads();
  unsigned long long t_max = 0, n_client = 0;
  int bad = 0;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < w.n_events; i += stride) {
    const lc_ps_event e = w.ev[i];
    bad |= bad_event(e, w.n_f);
    const bool client = e.process >= 0;
    if (client && e.time >= 0) {
      n_client++;
      t_max = (unsigned long long)e.time > t_max ? (unsigned long long)e.time : t_max;
    }
    w.pkey_in[i] = client ? (uint32_t)e.process : kNoClient;
    w.ppos_in[i] = (int32_t)i;
    if (w.comp_pos) {
      w.comp_pos[i] = -1;
      w.latency[i] = LC_PS_NONE;
    }
  }
  t_max = wave_max(t_max);
  n_client = wave_sum(n_client);
  if (bad) atomicOr(&s_bad, bad);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_max[threadIdx.x / kWave] = t_max;
    s_cnt[threadIdx.x / kWave] = n_client;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < kBlock / kWave; k++) {
      t_max = s_max[k] > t_max ? s_max[k] : t_max;
      n_client += s_cnt[k];
    }
    if (t_max) atomicMax(&w.status->t_max, t_max);
    if (n_client) atomicAdd(&w.status->n_client, n_client);
    if (s_bad) atomicOr(&w.status->bad, s_bad);
  }
}

__global__ __launch_bounds__(kBlock) void ps_fill_kernel(int64_t *p, int64_t n, int64_t v) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) p[i] = v;
}

// the record at a slot, or nobody's
__device__ __forceinline__ lc_ps_event slot_event(const Ws &w, int64_t slot) {
  if (slot >= 0 && slot < w.n_client) return w.ev[w.ppos[slot]];
  lc_ps_event e;
  e.time = 0;
  e.process = -1;
  e.f = 0;
  e.type = LC_EV_INVOKE;
  e.pad = 0;
  return e;
}

template <bool kLds>
__global__ __launch_bounds__(kBlock) void ps_pair_kernel(Ws w) {
  extern __shared__ uint32_t s_hist[];  // kLds: hist_entries
  __shared__ lc_ps_event tile[kBlock + 2];
  __shared__ unsigned long long s_part[kBlock / kWave][4];
  const int tid = threadIdx.x;
  if (kLds) {
    for (int64_t i = tid; i < w.hist_entries; i += kBlock) s_hist[i] = 0;
  }
  const int64_t n_rate_entries = (int64_t)w.n_f * 3 * w.n_rate;
  const uint32_t no_group = (uint32_t)((int64_t)w.n_f * w.n_quant);
  auto count = [&](int64_t entry) {
    if (kLds)
      atomicAdd(&s_hist[entry], 1u);
    else
      atomicAdd(&w.hist[entry], 1ull);
  };
  unsigned long long n_pairs = 0, n_pending = 0, n_ignored = 0, n_mismatched = 0;
  const int64_t n_chunks = (w.n_client + kChunk - 1) / kChunk;
  for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
    for (int round = 0; round < kChunk / kBlock; round++) {
      const int64_t base = chunk * kChunk + (int64_t)round * kBlock;
      if (base >= w.n_client) break;  // (uniform over the workgroup)
      const int64_t slot = base + tid;
      __syncthreads();  // the last round's tile is read; the histogram is zero
      tile[tid + 1] = slot_event(w, slot);
      if (tid == 0) tile[0] = slot_event(w, base - 1);
      if (tid == kWave) tile[kBlock + 1] = slot_event(w, base + kBlock);
      __syncthreads();
      if (slot >= w.n_client) continue;
      const lc_ps_event e = tile[tid + 1];
      uint32_t group = no_group;
      int64_t lat = LC_PS_NONE;
      if (e.type == LC_EV_INVOKE) {
        const lc_ps_event nx = tile[tid + 2];
        if (nx.process == e.process && nx.type != LC_EV_INVOKE) {
          n_pairs++;
          if (nx.f != e.f) n_mismatched++;
          lat = nx.time - e.time;
          const int64_t g = (int64_t)e.f * w.n_quant + e.time / w.quant_dt;
          group = (uint32_t)g;
          count(n_rate_entries + g);
          if (w.comp_pos) {
            const int32_t pos = w.ppos[slot];
            w.comp_pos[pos] = w.ppos[slot + 1];
            w.latency[pos] = lat;
          }
        } else {
          n_pending++;
        }
      } else {
        const lc_ps_event pv = tile[tid];
        if (!(pv.process == e.process && pv.type == LC_EV_INVOKE)) n_ignored++;
        count(((int64_t)e.f * 3 + (e.type - 1)) * w.n_rate + e.time / w.rate_dt);
      }
      w.gkey[slot] = group;
      w.glat[slot] = lat;
    }
  }
  n_pairs = wave_sum(n_pairs);
  n_pending = wave_sum(n_pending);
  n_ignored = wave_sum(n_ignored);
  n_mismatched = wave_sum(n_mismatched);
  if ((tid & (kWave - 1)) == 0) {
    unsigned long long *p = s_part[tid / kWave];
    p[0] = n_pairs, p[1] = n_pending, p[2] = n_ignored, p[3] = n_mismatched;
  }
  __syncthreads();
  if (tid < 4) {
    unsigned long long v = 0;
    for (int k = 0; k < kBlock / kWave; k++) v += s_part[k][tid];
    unsigned long long *dst = tid == 0   ? &w.status->n_pairs
                              : tid == 1 ? &w.status->n_pending
                              : tid == 2 ? &w.status->n_ignored
                                         : &w.status->n_mismatched;
    if (v) atomicAdd(dst, v);
  }
  if (kLds) {
    for (int64_t i = tid; i < w.hist_entries; i += kBlock) {
      const uint32_t v = s_hist[i];
      if (v) atomicAdd(&w.hist[i], (unsigned long long)v);
    }
  }
}

__global__ __launch_bounds__(kBlock) void ps_select_kernel(Ws w) {
  const int64_t n_groups = (int64_t)w.n_f * w.n_quant;
  const int64_t n_rate_entries = (int64_t)w.n_f * 3 * w.n_rate;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < w.n_client; i += stride) {
    const int64_t g = w.gkey[i];
    if (g >= n_groups) continue;
    if (i > 0 && w.gkey[i - 1] == g) continue;  // (the group's start is elsewhere)
    const int64_t n = (int64_t)w.hist[n_rate_entries + g];
    if (n < 1 || i + n > w.n_client) continue;  // (never: the count is the pair pass's own)
    for (int k = 0; k < w.n_q; k++) w.quant[g * w.n_q + k] = w.glat[i + quantile_index(w.q[k], n)];
  }
}

int blocks_for(int64_t n) { return (int)std::min<int64_t>(kMaxGrid, std::max<int64_t>(1, (n + kBlock - 1) / kBlock)); }

}  // namespace

size_t sort_temp_bytes(int64_t n, int group_bits) {
  size_t a = 0, b = 0, c = 0;
  uint32_t *k = nullptr;
  int32_t *v = nullptr;
  int64_t *l = nullptr;
  (void)rocprim::radix_sort_pairs(nullptr, a, k, k, v, v, (size_t)n, 0, 32);
  (void)rocprim::radix_sort_pairs(nullptr, b, l, l, k, k, (size_t)n, 0, 64);
  (void)rocprim::radix_sort_pairs(nullptr, c, k, k, l, l, (size_t)n, 0, (unsigned)group_bits);
  return std::max(a, std::max(b, c));
}

hipError_t launch_scan(const Ws &w, hipStream_t st) {
  hipLaunchKernelGGL(ps_scan_kernel, dim3(blocks_for(w.n_events)), dim3(kBlock), 0, st, w);
  return hipGetLastError();
}

hipError_t launch_process_sort(const Ws &w, hipStream_t st) {
  size_t bytes = w.temp_bytes;
  return rocprim::radix_sort_pairs(w.temp, bytes, w.pkey_in, w.pkey, w.ppos_in, w.ppos, (size_t)w.n_events, 0, 32, st);
}

hipError_t launch_pairs(const Ws &w, hipStream_t st) {
  const int64_t n_quant_entries = (int64_t)w.n_f * w.n_quant * w.n_q;
  if (n_quant_entries > 0) {
    hipLaunchKernelGGL(ps_fill_kernel, dim3(blocks_for(n_quant_entries)), dim3(kBlock), 0, st, w.quant, n_quant_entries,
                       (int64_t)LC_PS_NONE);
    if (hipError_t e = hipGetLastError()) return e;
  }
  const int grid = (int)std::min<int64_t>(kMaxGrid, (w.n_client + kChunk - 1) / kChunk);
  if (w.hist_entries <= w.lds_entries)
    hipLaunchKernelGGL(ps_pair_kernel<true>, dim3(grid), dim3(kBlock), sizeof(uint32_t) * (size_t)w.hist_entries, st,
                       w);
  else
    hipLaunchKernelGGL(ps_pair_kernel<false>, dim3(grid), dim3(kBlock), 0, st, w);
  return hipGetLastError();
}

hipError_t launch_group_sort(const Ws &w, int group_bits, hipStream_t st) {
  size_t bytes = w.temp_bytes;
  if (hipError_t e = rocprim::radix_sort_pairs(w.temp, bytes, w.glat, w.glat2, w.gkey, w.gkey2, (size_t)w.n_client, 0,
                                               64, st))
    return e;
  bytes = w.temp_bytes;
  return rocprim::radix_sort_pairs(w.temp, bytes, w.gkey2, w.gkey, w.glat2, w.glat, (size_t)w.n_client, 0,
                                   (unsigned)group_bits, st);
}

hipError_t launch_select(const Ws &w, hipStream_t st) {
  hipLaunchKernelGGL(ps_select_kernel, dim3(blocks_for(w.n_client)), dim3(kBlock), 0, st, w);
  return hipGetLastError();
}

}  // namespace lcps
