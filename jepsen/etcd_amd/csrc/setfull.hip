// setfull.hip — the kernels of lc_set_full (include/lincheck_setfull.h): what
// scales with the payload or with reads x elements runs here.
//
//  sf_fill_kernel / sf_prep_kernel / sf_table_kernel (once per call): the
//    table's keys set to empty; the reads' positions as two int32 arrays
//    (the element kernel reads them lane by lane); the E element values into
//    an open-addressed table of >= 2 E slots, a 64-bit compare-and-swap on
//    the key, (element, inv_pos) stored beside it.  A second insertion of one
//    value raises status[0].
//  sf_mark_kernel (per tile): one work item per (read, payload entry); the
//    item finds its read in the prefix sums of the reads' lengths, probes the
//    table, tests rule 3 and sets bit (element, read) of the element-major
//    bitmap.  An atomicOr that finds its bit set marks the element in
//    dup_seen: it occurs twice in that read.  Phantoms: one add per workgroup
//    onto counters 128 B apart.
//  sf_element_kernel (per tile): one wavefront per element.  The reads that
//    concern it are a suffix of its row (columns are in ok_pos order): a
//    binary search finds it.  first_seen is the lowest set bit.
//    last_present / last_absent are the largest inv_pos over the set / clear
//    bits: the wave walks the row from the top, 64 columns at a time, and
//    stops once ok_pos of the next column down is at or below both bests — a
//    lower column's invoke precedes its own completion, so it cannot win.
//    Then rules 4 to 6 (setfull.h, decide) and one 40-byte record.
//
// Every loop is bounded by an element, read, payload or table count; no
// workgroup waits for another; results leave through vector stores.
#include "setfull.h"

namespace lcsf {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kChunk = 4096;      // work items of one workgroup iteration
constexpr int kMaxGrid = 256 * 8; // grid-stride kernels: at most this many workgroups

__global__ __launch_bounds__(kThreads) void sf_fill_kernel(int64_t *key, uint64_t cap) {
  for (uint64_t i = blockIdx.x * (uint64_t)kThreads + threadIdx.x; i < cap; i += (uint64_t)gridDim.x * kThreads)
    key[i] = kEmpty;
}

__global__ __launch_bounds__(kThreads) void sf_prep_kernel(const lc_sf_read *__restrict__ reads, int64_t n_reads,
                                                           int32_t *__restrict__ r_inv,
                                                           int32_t *__restrict__ r_ok) {
  for (int64_t r = blockIdx.x * (int64_t)kThreads + threadIdx.x; r < n_reads; r += (int64_t)gridDim.x * kThreads) {
    r_inv[r] = reads[r].inv_pos;
    r_ok[r] = reads[r].ok_pos;
  }
}

__global__ __launch_bounds__(kThreads) void sf_table_kernel(const lc_sf_add *__restrict__ adds, int64_t n_adds,
                                                            int64_t *tab_key, Ent *tab_ent, uint64_t cap,
                                                            int32_t *status) {
  unsigned long long *key = reinterpret_cast<unsigned long long *>(tab_key);
  for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < n_adds; e += (int64_t)gridDim.x * kThreads) {
    const int64_t v = adds[e].value;
    uint64_t s = slot_of(v, cap);
    for (uint64_t i = 0; i < cap; i++) {
      const unsigned long long old = atomicCAS(&key[s], (unsigned long long)kEmpty, (unsigned long long)v);
      if (old == (unsigned long long)kEmpty) {
        tab_ent[s] = Ent{(int32_t)e, adds[e].inv_pos};
        break;
      }
      if (old == (unsigned long long)v) {  // two adds of one value
        status[1] = (int32_t)e;
        status[0] = 1;
        break;
      }
      s = (s + 1) & (cap - 1);
    }
  }
}

// The largest r in [lo, hi] with work_off[r] <= w (work_off[lo] <= w holds).
__device__ __forceinline__ int64_t read_of(const int64_t *__restrict__ work_off, int64_t lo, int64_t hi, int64_t w) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (work_off[mid] <= w) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void sf_mark_kernel(Ws w, int64_t e0, int64_t e1) {
  __shared__ long long s_ph[kWaves];
  const Ent *__restrict__ ent = w.tab_ent;
  const int64_t *__restrict__ key = w.tab_key;
  const int64_t n_chunks = (w.n_work + kChunk - 1) / kChunk;
  long long ph = 0;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t w0 = c * kChunk;
    const int64_t w1 = w0 + kChunk < w.n_work ? w0 + kChunk : w.n_work;
    // the chunk's reads: every item's search stays inside [r_lo, r_hi]
    const int64_t r_lo = read_of(w.work_off, 0, w.n_reads - 1, w0);
    const int64_t r_hi = read_of(w.work_off, r_lo, w.n_reads - 1, w1 - 1);
    for (int64_t i = w0 + threadIdx.x; i < w1; i += kThreads) {
      const int64_t r = read_of(w.work_off, r_lo, r_hi, i);
      const int64_t v = w.values[w.reads[r].off + (i - w.work_off[r])];
      const int32_t ok_pos = w.reads[r].ok_pos;
      Ent hit{-1, 0};
      if (v != kEmpty) {
        uint64_t s = slot_of(v, w.cap);
        for (uint64_t p = 0; p < w.cap; p++) {
          const int64_t k = key[s];
          if (k == v) {
            hit = ent[s];
            break;
          }
          if (k == kEmpty) break;
          s = (s + 1) & (w.cap - 1);
        }
      }
      if (hit.id < 0 || ok_pos <= hit.inv_pos) {
        ph++;  // names no element, or one the read does not concern
      } else if (hit.id >= e0 && hit.id < e1) {
        const uint32_t bit = 1u << (r & 31);
        const uint32_t old = atomicOr(&w.bitmap[(hit.id - e0) * w.wpr + (r >> 5)], bit);
        if (old & bit) {
          w.dup_seen[hit.id] = 1;
          w.status[2] = 1;
        }
      }
    }
  }
  if (e0 != 0) return;  // a later tile: the phantoms are counted already
  for (int o = 32; o; o >>= 1) ph += __shfl_xor(ph, o);
  if ((threadIdx.x & 63) == 0) s_ph[threadIdx.x >> 6] = ph;
  __syncthreads();
  if (threadIdx.x == 0) {
    long long t = 0;
    for (int i = 0; i < kWaves; i++) t += s_ph[i];
    if (t)
      atomicAdd(reinterpret_cast<unsigned long long *>(&w.counters[(blockIdx.x % kCounterShards) * kCounterStride]),
                (unsigned long long)t);
  }
}

__device__ __forceinline__ long long wave_max_i64(long long v) {
  for (int o = 32; o; o >>= 1) {
    const long long u = __shfl_xor(v, o);
    v = u > v ? u : v;
  }
  return v;
}

__global__ __launch_bounds__(kThreads) void sf_element_kernel(Ws w, int64_t e0, int64_t e1) {
  const int32_t *__restrict__ r_inv = w.r_inv;
  const int32_t *__restrict__ r_ok = w.r_ok;
  const int lane = threadIdx.x & 63;
  const int64_t R = w.n_reads;
  for (int64_t e = e0 + blockIdx.x * (int64_t)kWaves + (threadIdx.x >> 6); e < e1;
       e += (int64_t)gridDim.x * kWaves) {
    const lc_sf_add a = w.adds[e];
    const uint32_t *__restrict__ row = w.bitmap + (e - e0) * w.wpr;
    // c0: the first column whose read concerns e (ok_pos > inv_pos)
    int64_t c0 = 0;
    {
      int64_t hi = R;
      while (c0 < hi) {
        const int64_t mid = (c0 + hi) >> 1;
        if (r_ok[mid] > a.inv_pos) hi = mid;
        else c0 = mid + 1;
      }
    }
    // first_seen: the lowest set bit (the mark pass sets none below c0)
    int64_t fs = -1;
    for (int64_t wb = c0 >> 5; wb < w.wpr && fs < 0; wb += 64) {
      const int64_t wi = wb + lane;
      uint32_t word = wi < w.wpr ? row[wi] : 0u;
      if (wi == (c0 >> 5)) word &= ~0u << (c0 & 31);
      const uint64_t any = __ballot(word != 0);
      if (any) {
        const int l = (int)__builtin_ctzll(any);
        const uint32_t wl = (uint32_t)__shfl((int)word, l);
        fs = (wb + l) * 32 + __builtin_ctz(wl);
      }
    }
    // last_present / last_absent: (inv_pos, column) maxima over the set /
    // clear bits, from the top; among equal inv_pos the highest column wins
    long long best_p = -1, best_a = -1;
    if (c0 < R) {
      for (int64_t base = ((R - 1) >> 6) << 6; base + 63 >= c0; base -= 64) {
        const int64_t col = base + lane;
        long long kp = -1, ka = -1;
        if (col >= c0 && col < R) {
          const long long k = ((long long)r_inv[col] << 32) | (long long)col;
          if ((row[col >> 5] >> (col & 31)) & 1u) kp = k;
          else ka = k;
        }
        kp = wave_max_i64(kp);
        ka = wave_max_i64(ka);
        best_p = kp > best_p ? kp : best_p;
        best_a = ka > best_a ? ka : best_a;
        if (base - 1 < c0) break;
        const long long thr = r_ok[base - 1];
        if ((best_p >> 32) >= thr && (best_a >> 32) >= thr) break;  // no lower column can win
      }
    }
    if (lane == 0) {
      int32_t fs_pos = -1, lp_pos = -1, la_pos = -1;
      int64_t fs_time = 0, lp_time = 0, la_time = 0;
      if (fs >= 0) {
        fs_pos = w.reads[fs].ok_pos;
        fs_time = w.reads[fs].ok_time;
      }
      if (best_p >= 0) {
        lp_pos = (int32_t)(best_p >> 32);
        lp_time = w.reads[best_p & 0xFFFFFFFFll].inv_time;
      }
      if (best_a >= 0) {
        la_pos = (int32_t)(best_a >> 32);
        la_time = w.reads[best_a & 0xFFFFFFFFll].inv_time;
      }
      w.out[e] = decide(a, fs_pos, fs_time, lp_pos, lp_time, la_pos, la_time);
    }
  }
}

int grid_for(int64_t items, int64_t per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)(g < kMaxGrid ? g : kMaxGrid);
}

}  // namespace

hipError_t launch_table(const Ws &w, hipStream_t st) {
  sf_fill_kernel<<<grid_for((int64_t)w.cap, kThreads), kThreads, 0, st>>>(w.tab_key, w.cap);
  sf_prep_kernel<<<grid_for(w.n_reads, kThreads), kThreads, 0, st>>>(w.reads, w.n_reads, w.r_inv, w.r_ok);
  sf_table_kernel<<<grid_for(w.n_adds, kThreads), kThreads, 0, st>>>(
      w.adds, w.n_adds, w.tab_key, w.tab_ent, w.cap, w.status);
  return hipGetLastError();
}

hipError_t launch_tile(const Ws &w, int64_t e0, int64_t e1, hipStream_t st) {
  hipError_t e = hipMemsetAsync(w.bitmap, 0, sizeof(uint32_t) * (size_t)((e1 - e0) * w.wpr), st);
  if (e != hipSuccess) return e;
  if (w.n_work > 0) sf_mark_kernel<<<grid_for(w.n_work, kChunk), kThreads, 0, st>>>(w, e0, e1);
  sf_element_kernel<<<grid_for(e1 - e0, kWaves), kThreads, 0, st>>>(w, e0, e1);
  return hipGetLastError();
}

}  // namespace lcsf
