// txngraph.hip — the launchers both Elle checkers call (txngraph.h): none
// reads a checker's workspace.
//
//  Key slots: rocprim select lists a key table's occupied slots, in slot order.
//  Edges: rocprim select, merge_sort by (from, to, type, key), unique — the
//    result does not depend on which slot an edge came from.
//  Real time (rule 6 of include/lincheck_append.h): rocprim select / radix
//    sort / prefix max, then two binary searches per txn (ap_rt_kernel).
//
// Every loop is bounded by a txn count; no workgroup waits for another;
// results leave through vector stores.
#include <rocprim/device/device_merge_sort.hpp>
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include <algorithm>

#include "txngraph_dev.h"

namespace lctg {

namespace {

struct KeySet {
  const int64_t *ktab;
  __host__ __device__ bool operator()(int32_t s) const { return ktab[s] != -1; }
};
struct EdgeSet {
  __host__ __device__ bool operator()(const lc_ap_edge &e) const { return e.from >= 0; }
};
struct EdgeLess {
  __host__ __device__ bool operator()(const lc_ap_edge &a, const lc_ap_edge &b) const { return edge_less(a, b); }
};
struct EdgeSame {
  __host__ __device__ bool operator()(const lc_ap_edge &a, const lc_ap_edge &b) const { return edge_same(a, b); }
};
struct IsOk {
  const lc_ap_txn *txns;
  __host__ __device__ bool operator()(int32_t t) const { return txns[t].type == LC_AP_OK; }
};
struct MaxOp {
  __host__ __device__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; }
};

// kind 0: out[i] = comp_pos of txn idx[i]; kind 1: its inv_pos.
template <int kKind>
__global__ __launch_bounds__(kThreads) void ap_gather_kernel(const lc_ap_txn *__restrict__ txns,
                                                             const int32_t *__restrict__ idx, int64_t n,
                                                             int32_t *__restrict__ out) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads)
    out[i] = kKind ? txns[idx[i]].inv_pos : txns[idx[i]].comp_pos;
}

// The number of entries of comp[0, n) below x.
__device__ __forceinline__ int64_t count_below(const int32_t *__restrict__ comp, int64_t n, int32_t x) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (comp[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void ap_rt_kernel(const lc_ap_txn *__restrict__ txns, int64_t n_txns,
                                                         const int32_t *__restrict__ comp,
                                                         const int32_t *__restrict__ pm, int64_t n_ok,
                                                         int32_t *__restrict__ rt_lo, int32_t *__restrict__ rt_hi) {
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < n_txns; t += (int64_t)gridDim.x * kThreads) {
    int32_t lo = 0, hi = 0;
    if (txns[t].type != LC_AP_FAIL) {
      hi = (int32_t)count_below(comp, n_ok, txns[t].inv_pos);
      // positions are distinct: above m(B) is at or above m(B) + 1
      lo = hi ? (int32_t)count_below(comp, n_ok, pm[hi - 1] + 1) : 0;
    }
    rt_lo[t] = lo;
    rt_hi[t] = hi;
  }
}

}  // namespace

size_t key_temp_bytes(uint64_t kcap) {
  size_t a = 0;
  int32_t *p = nullptr;
  int64_t *cnt = nullptr;
  (void)rocprim::select(nullptr, a, rocprim::counting_iterator<int32_t>(0), p, cnt, (size_t)kcap, KeySet{nullptr});
  return a;
}

hipError_t launch_key_slots(const int64_t *ktab, uint64_t kcap, int32_t *kslots, int64_t *d_n_keys, void *temp,
                            size_t temp_bytes, hipStream_t st) {
  return rocprim::select(temp, temp_bytes, rocprim::counting_iterator<int32_t>(0), kslots, d_n_keys, (size_t)kcap,
                         KeySet{ktab}, st);
}

size_t edge_temp_bytes(int64_t n_slots) {
  size_t a = 0, b = 0, c = 0;
  lc_ap_edge *e = nullptr;
  int64_t *cnt = nullptr;
  const size_t n = (size_t)(n_slots > 0 ? n_slots : 1);
  (void)rocprim::select(nullptr, a, e, e, cnt, n, EdgeSet());
  (void)rocprim::merge_sort(nullptr, b, e, e, n, EdgeLess());
  (void)rocprim::unique(nullptr, c, e, e, cnt, n, EdgeSame());
  return std::max(a, std::max(b, c));
}

hipError_t launch_edge_select(const lc_ap_edge *slots, int64_t n_slots, lc_ap_edge *dst, int64_t *d_count, void *temp,
                              size_t temp_bytes, hipStream_t st) {
  return rocprim::select(temp, temp_bytes, slots, dst, d_count, (size_t)n_slots, EdgeSet(), st);
}

hipError_t launch_edge_sort(lc_ap_edge *src, lc_ap_edge *dst, int64_t n, int64_t *d_count, void *temp,
                            size_t temp_bytes, hipStream_t st) {
  size_t bytes = temp_bytes;
  hipError_t e = rocprim::merge_sort(temp, bytes, src, dst, (size_t)n, EdgeLess(), st);
  if (e != hipSuccess) return e;
  bytes = temp_bytes;
  return rocprim::unique(temp, bytes, dst, src, d_count, (size_t)n, EdgeSame(), st);
}

size_t rt_temp_bytes(int64_t n_txns) {
  size_t a = 0, b = 0, c = 0;
  int32_t *p = nullptr;
  int64_t *cnt = nullptr;
  const size_t n = (size_t)(n_txns > 0 ? n_txns : 1);
  (void)rocprim::select(nullptr, a, rocprim::counting_iterator<int32_t>(0), p, cnt, n, IsOk{nullptr});
  (void)rocprim::radix_sort_pairs(nullptr, b, p, p, p, p, n);
  (void)rocprim::inclusive_scan(nullptr, c, p, p, n, MaxOp());
  return std::max(a, std::max(b, c));
}

hipError_t launch_real_time(const lc_ap_txn *txns, int64_t n_txns, int64_t n_ok, const RtArrays &rt, int64_t *d_count,
                            void *temp, size_t temp_bytes, hipStream_t st) {
  if (n_ok > 0) {
    size_t bytes = temp_bytes;  // (the count select writes is the host's n_ok)
    hipError_t e = rocprim::select(temp, bytes, rocprim::counting_iterator<int32_t>(0), rt.ok_idx, d_count,
                                   (size_t)n_txns, IsOk{txns}, st);
    if (e != hipSuccess) return e;
    ap_gather_kernel<0><<<grid_for(n_ok, kThreads), kThreads, 0, st>>>(txns, rt.ok_idx, n_ok, rt.ok_comp);
    bytes = temp_bytes;
    e = rocprim::radix_sort_pairs(temp, bytes, rt.ok_comp, rt.comp_sorted, rt.ok_idx, rt.byc, (size_t)n_ok, 0, 32, st);
    if (e != hipSuccess) return e;
    ap_gather_kernel<1><<<grid_for(n_ok, kThreads), kThreads, 0, st>>>(txns, rt.byc, n_ok, rt.ok_comp);
    bytes = temp_bytes;
    e = rocprim::inclusive_scan(temp, bytes, rt.ok_comp, rt.pm, (size_t)n_ok, MaxOp(), st);
    if (e != hipSuccess) return e;
  }
  ap_rt_kernel<<<grid_for(n_txns, kThreads), kThreads, 0, st>>>(txns, n_txns, rt.comp_sorted, rt.pm, n_ok, rt.rt_lo,
                                                               rt.rt_hi);
  return hipGetLastError();
}

}  // namespace lctg
