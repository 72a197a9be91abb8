// watch.hip — the kernels of lc_watch_check (include/lincheck_watch.h): the
// log hashes that propose rule 2's classes, the exact compare that makes them
// exact and gives rule 4's prefix and suffix, rule 5's forward pass and its
// backtrack.  gfx950, wave64.
//
//  wt_hash_kernel (a workgroup per thread's log): lane j takes the elements j,
//    j + 256, .. by Horner's rule in B^256 and scales its share by the power of
//    B that its last element lacks; the shares are summed through the LDS.
//    (watch.h: the hash is a sum, so the order of the lanes does not matter.)
//  wt_compare_kernel (a workgroup per pair of logs): the first index at which
//    they differ, then, on what is left, the first index from the end.
//  wt_forward_kernel (a workgroup per differing thread): Myers' rounds with
//    the diagonals across the lanes and V in the LDS, updated in place (round d
//    writes the diagonals of d's parity and reads the others).  A lane follows
//    its snake for kLone steps; a snake that goes on is put on a list, and the
//    workgroup finishes the list one snake at a time with the compare's search.
//    Every round's row goes to the trace.
//  wt_backtrack_kernel (a wave per finished thread): the walk from D down to
//    1 over the trace; every lane computes the same, lane 0 stores the edits.
//
// wg_first_mismatch is the search the compare and the snakes share: each wave
// strides over tiles of kTile elements, kTileU independent loads per lane and
// array, and leaves at its first tile with a mismatch; the minimum is an LDS
// word, which the waves also read before each tile to leave once a mismatch
// below their tile is known.  That read is one address for the whole wave, and
// the result goes through readfirstlane: the exit is wave-uniform.  No barrier
// sits inside the loop, so a snake of L elements costs L / kStride round trips.
//
// Every loop is bounded by a length, a tile count, a round count (dcap) or a
// list length, all fixed at launch or by an earlier barrier; no workgroup waits
// for another; results leave through vector stores.
#include <limits.h>

#include "watch.h"

namespace lcwt {

namespace {

constexpr int kVOff = LC_WT_MAX_D_LIMIT + 1;      // V[k] lives at V[kVOff + k], k in [-dcap - 1, dcap + 1]
constexpr int kVLen = 2 * LC_WT_MAX_D_LIMIT + 3;
constexpr int kHashUnroll = 8;

constexpr uint64_t cpow(uint64_t b, uint64_t e) { return e == 0 ? 1 : (e & 1 ? b : 1) * cpow(b * b, e >> 1); }
constexpr uint64_t kBase1W = cpow(kBase1, kBlock), kBase2W = cpow(kBase2, kBlock);

__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int w = __shfl_xor(v, o, 64);
    v = w < v ? w : v;
  }
  return v;
}

// The least i in [0, L) with pa[i * step] != pb[i * step], or L.  Every lane
// of the workgroup calls it with the same arguments; s_first is an LDS word.
__device__ int wg_first_mismatch(const int64_t *__restrict__ pa, const int64_t *__restrict__ pb, int L, int step,
                                 int *s_first) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();  // (nobody still reads the word's earlier value)
  if (threadIdx.x == 0) *s_first = L;
  __syncthreads();
  const int n_tiles = (L + kTile - 1) / kTile;
  for (int tile = wave; tile < n_tiles; tile += kWaves) {
    const int base = tile * kTile;
    if (__builtin_amdgcn_readfirstlane(*(volatile int *)s_first) < base) break;
    int64_t va[kTileU], vb[kTileU];
#pragma unroll
    for (int u = 0; u < kTileU; u++) {
      const int i = base + u * 64 + lane;
      const bool in = i < L;
      va[u] = in ? pa[(int64_t)i * step] : 0;
      vb[u] = in ? pb[(int64_t)i * step] : 0;
    }
    int first = INT_MAX;
#pragma unroll
    for (int u = kTileU - 1; u >= 0; u--)
      if (va[u] != vb[u]) first = base + u * 64 + lane;
    if (__ballot(first != INT_MAX)) {
      const int w = wave_min(first);
      if (lane == 0) atomicMin(s_first, w);
      break;
    }
  }
  __syncthreads();
  return *(volatile int *)s_first;
}

__global__ __launch_bounds__(kBlock) void wt_hash_kernel(const int64_t *__restrict__ values,
                                                         const int64_t *__restrict__ off,
                                                         const int32_t *__restrict__ len, Hash *__restrict__ out) {
  __shared__ uint64_t s1[kBlock], s2[kBlock];
  const int64_t *v = values + off[blockIdx.x];
  const int n = len[blockIdx.x], j = threadIdx.x;
  uint64_t p1 = 0, p2 = 0;
  int i = j, last = -1;
  // full groups of kHashUnroll independent loads, then the rest one by one
  for (; (int64_t)i + (kHashUnroll - 1) * kBlock < n; i += kHashUnroll * kBlock) {
    int64_t x[kHashUnroll];
#pragma unroll
    for (int u = 0; u < kHashUnroll; u++) x[u] = v[i + u * kBlock];
#pragma unroll
    for (int u = 0; u < kHashUnroll; u++) {
      p1 = p1 * kBase1W + mix1(x[u]);
      p2 = p2 * kBase2W + mix2(x[u]);
    }
    last = i + (kHashUnroll - 1) * kBlock;
  }
  for (; i < n; i += kBlock) {
    const int64_t x = v[i];
    p1 = p1 * kBase1W + mix1(x);
    p2 = p2 * kBase2W + mix2(x);
    last = i;
  }
  const uint64_t e = last < 0 ? 0 : (uint64_t)(n - 1 - last);  // below kBlock
  s1[j] = p1 * pow64(kBase1, e);
  s2[j] = p2 * pow64(kBase2, e);
  __syncthreads();
  for (int w = kBlock / 2; w > 0; w >>= 1) {
    if (j < w) {
      s1[j] += s1[j + w];
      s2[j] += s2[j + w];
    }
    __syncthreads();
  }
  if (j == 0) out[blockIdx.x] = Hash{s1[0], s2[0]};
}

__global__ __launch_bounds__(kBlock) void wt_compare_kernel(const int64_t *__restrict__ values,
                                                            const Pair *__restrict__ pairs,
                                                            PairRes *__restrict__ res) {
  __shared__ int s_first;
  const Pair pr = pairs[blockIdx.x];
  const int64_t *A = values + pr.a_off, *B = values + pr.b_off;
  const int lim = pr.a_len < pr.b_len ? pr.a_len : pr.b_len;
  const int p = wg_first_mismatch(A, B, lim, 1, &s_first);
  // the suffix of what the prefix leaves: never past it (with lim - p == 0 nothing is read)
  const int s = wg_first_mismatch(A + pr.a_len - 1, B + pr.b_len - 1, lim - p, -1, &s_first);
  if (threadIdx.x == 0) res[blockIdx.x] = PairRes{p, s};
}

__global__ __launch_bounds__(kBlock) void wt_forward_kernel(const int64_t *__restrict__ values,
                                                            const Item *__restrict__ items,
                                                            int32_t *__restrict__ trace, int32_t *__restrict__ dist) {
  __shared__ int V[kVLen];
  __shared__ int list[LC_WT_MAX_D_LIMIT + 1];
  __shared__ int s_first, s_cnt;
  const Item it = items[blockIdx.x];
  const int64_t *a = values + it.a_off, *b = values + it.b_off;
  const int n = it.n, m = it.m, dcap = it.dcap, tid = threadIdx.x;
  const int kend = n - m, kabs = kend < 0 ? -kend : kend;
  int32_t *tr = trace + it.trace_off;
  if (tid == 0) V[kVOff + 1] = 0;
  int D = -1;
  for (int d = 0; d <= dcap; d++) {
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    for (int i = tid; i <= d; i += kBlock) {
      const int k = -d + 2 * i;
      const int vm = V[kVOff + k - 1], vp = V[kVOff + k + 1];
      int x = comes_down(k, d, vm, vp) ? vp : vm + 1;
      int y = x - k;
      bool more = true;
      for (int t = 0; t < kLone; t++) {
        if (!(x < n && y < m && a[x] == b[y])) {
          more = false;
          break;
        }
        x++, y++;
      }
      if (more && x < n && y < m) list[atomicAdd(&s_cnt, 1)] = i;  // the snake may go on
      V[kVOff + k] = x;
    }
    __syncthreads();
    const int cnt = s_cnt;  // at most d + 1; the same for every lane
    for (int e = 0; e < cnt; e++) {
      const int k = -d + 2 * list[e];
      const int x = V[kVOff + k], y = x - k;
      const int L = n - x < m - y ? n - x : m - y;
      const int f = wg_first_mismatch(a + x, b + y, L, 1, &s_first);
      if (tid == 0) V[kVOff + k] = x + f;
    }
    __syncthreads();
    const int64_t row = trace_row(d);
    for (int i = tid; i <= d; i += kBlock) tr[row + i] = V[kVOff - d + 2 * i];
    // the same LDS word for every lane: the exit is uniform over the workgroup
    if (d >= kabs && ((d - kend) & 1) == 0 && V[kVOff + kend] >= n) {
      D = d;
      break;
    }
  }
  if (tid == 0) dist[blockIdx.x] = D;
}

__global__ __launch_bounds__(64) void wt_backtrack_kernel(const int64_t *__restrict__ values,
                                                          const Item *__restrict__ items,
                                                          const int32_t *__restrict__ trace,
                                                          const int32_t *__restrict__ dist,
                                                          lc_wt_edit *__restrict__ edits) {
  const Item it = items[blockIdx.x];
  const int D = dist[blockIdx.x];
  if (D < 0) return;  // (one item per workgroup: uniform)
  const int64_t *a = values + it.a_off, *b = values + it.b_off;
  const int32_t *tr = trace + it.trace_off;
  lc_wt_edit *out = edits + it.edit_off;
  int k = it.n - it.m;
  for (int d = D; d >= 1; d--) {
    const int32_t *row = tr + trace_row(d - 1);
    // row d - 1 holds the diagonals -(d - 1) + 2 i; the neighbour the rule does not read may lie outside
    const int im = k - 1 + (d - 1), ip = k + 1 + (d - 1);
    const int vm = (im < 0 || im > 2 * (d - 1)) ? 0 : row[im >> 1];
    const int vp = (ip < 0 || ip > 2 * (d - 1)) ? 0 : row[ip >> 1];
    lc_wt_edit e;
    // (the path lies inside the grid; an index that did not would be a fault of the trace's, and is not followed)
    if (comes_down(k, d, vm, vp)) {
      const int y = vp - (k + 1);
      e = lc_wt_edit{it.base + vp, y >= 0 && y < it.m ? b[y] : 0, LC_WT_INSERT, 0};
      k = k + 1;
    } else {
      e = lc_wt_edit{it.base + vm, vm >= 0 && vm < it.n ? a[vm] : 0, LC_WT_DELETE, 0};
      k = k - 1;
    }
    if (threadIdx.x == 0) out[d - 1] = e;
  }
}

}  // namespace

hipError_t launch_hashes(const int64_t *values, const int64_t *off, const int32_t *len, int n_threads, Hash *out,
                         hipStream_t st) {
  if (n_threads <= 0) return hipSuccess;
  hipLaunchKernelGGL(wt_hash_kernel, dim3(n_threads), dim3(kBlock), 0, st, values, off, len, out);
  return hipGetLastError();
}

hipError_t launch_compare(const int64_t *values, const Pair *pairs, int n_pairs, PairRes *res, hipStream_t st) {
  if (n_pairs <= 0) return hipSuccess;
  hipLaunchKernelGGL(wt_compare_kernel, dim3(n_pairs), dim3(kBlock), 0, st, values, pairs, res);
  return hipGetLastError();
}

hipError_t launch_forward(const int64_t *values, const Item *items, int n_items, int32_t *trace, int32_t *dist,
                          hipStream_t st) {
  if (n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(wt_forward_kernel, dim3(n_items), dim3(kBlock), 0, st, values, items, trace, dist);
  return hipGetLastError();
}

hipError_t launch_backtrack(const int64_t *values, const Item *items, int n_items, const int32_t *trace,
                            const int32_t *dist, lc_wt_edit *edits, hipStream_t st) {
  if (n_items <= 0) return hipSuccess;
  hipLaunchKernelGGL(wt_backtrack_kernel, dim3(n_items), dim3(64), 0, st, values, items, trace, dist, edits);
  return hipGetLastError();
}

}  // namespace lcwt
