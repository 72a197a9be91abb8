// screen.hip — lc_cycle_screen's kernels (screen.h; the method is
// include/lincheck_screen.h's).
//
//  scr_setup_kernel: the edges' ends into two int32 arrays (the rounds read 8
//    of an edge's 24 bytes), first(u) by binary search over the txns' inv_pos
//    (n_txns for a txn that is not OK: it then reads no suffix), round 0's
//    labels.  A FAIL txn has H = INT32_MAX and K = -1, the scans' identities,
//    and keeps them: it has no edge, no first(u), and rt_hi 0.
//  A label round: two rocprim scans over the last round's labels (the suffix
//    minimum of H as a prefix minimum over the reversed array, the prefix
//    maximum of K over byc), scr_label_node_kernel (a thread per txn: the
//    txn's own label, its suffix, its prefix), scr_label_edge_kernel (a
//    thread per edge: load and compare, then atomicMin / atomicMax only where
//    the label moves, so a converged round only reads), scr_round_end_kernel
//    (one thread: the round counted, the phase done where nothing changed).
//  scr_flag_kernel: H < K, counted on the sharded counters; round 0's
//    survivors.  scr_class_kernel: the edges whose ends are not both
//    survivors of one (H, K) leave (from = -1).
//  A trim round: scr_trim_edge_kernel marks has-in / has-out from the edges
//    in class between survivors, scr_trim_node_kernel takes alive & in & out
//    and clears the marks, scr_round_end_kernel.
//  scr_mark_kernel: bit 1 and its count.
//
// The kernels of a round written here return at once when their phase is done,
// so the driver launches rounds in batches and looks at the control words once
// per batch.  rocprim's scans do not look at those words: the rounds of a
// batch that follow the quiet one (3 at most) still run their two scans, over
// labels that no longer move; the results do not depend on it.
// Every loop is bounded by a txn, edge or round count; no workgroup waits for
// another; results leave through vector stores and 32-bit atomicMin /
// atomicMax.
#include <rocprim/device/device_scan.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include <algorithm>

#include "screen.h"
#include "txngraph_dev.h"

namespace lcscreen {

namespace {

struct MinOp {
  __host__ __device__ int32_t operator()(int32_t a, int32_t b) const { return a < b ? a : b; }
};
struct MaxOp {
  __host__ __device__ int32_t operator()(int32_t a, int32_t b) const { return a > b ? a : b; }
};
struct Reversed {  // i -> a[n - 1 - i]
  const int32_t *a;
  int32_t n;
  __host__ __device__ int32_t operator()(int32_t i) const { return a[n - 1 - i]; }
};
struct Through {  // i -> a[idx[i]]
  const int32_t *a, *idx;
  __host__ __device__ int32_t operator()(int32_t i) const { return a[idx[i]]; }
};

// One store per wave that saw a change.
__device__ __forceinline__ void note_change(int32_t *changed, bool mine) {
  if (__any(mine) && (threadIdx.x & 63) == 0) *changed = 1;
}

__global__ __launch_bounds__(kThreads) void scr_setup_kernel(Ws w) {
  const int64_t n = w.n_txns, items = n > w.n_edges ? n : w.n_edges;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < items; i += (int64_t)gridDim.x * kThreads) {
    if (i < w.n_edges) {
      w.e_from[i] = w.edges[i].from;
      w.e_to[i] = w.edges[i].to;
    }
    if (i < n) {
      const lc_ap_txn x = w.txns[i];
      int64_t lo = n;
      if (x.type == LC_AP_OK) {  // the least index whose inv_pos is above comp_pos
        int64_t hi = n;
        lo = 0;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (w.txns[mid].inv_pos > x.comp_pos) hi = mid;
          else lo = mid + 1;
        }
      }
      w.first[i] = (int32_t)lo;
      w.h[0][i] = x.type == LC_AP_OK ? x.comp_pos : kNoComp;
      w.k[0][i] = x.type == LC_AP_FAIL ? kNoInv : x.inv_pos;
    }
  }
}

__global__ __launch_bounds__(kThreads) void scr_label_node_kernel(Ws w, int r) {
  if (w.ctl->label.done) return;
  const int32_t *hc = w.h[(r - 1) & 1], *kc = w.k[(r - 1) & 1];
  int32_t *hn = w.h[r & 1], *kn = w.k[r & 1];
  const int64_t n = w.n_txns;
  bool moved = false;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < n; t += (int64_t)gridDim.x * kThreads) {
    const int32_t h0 = hc[t], k0 = kc[t], f = w.first[t], rh = w.rt_hi[t];
    int32_t h = h0, k = k0;
    if (f < n) h = min(h, w.s_rev[n - 1 - f]);
    if (rh > 0) k = max(k, w.p_inc[rh - 1]);
    hn[t] = h;
    kn[t] = k;
    moved |= h != h0 || k != k0;
  }
  note_change(&w.ctl->label.changed, moved);
}

__global__ __launch_bounds__(kThreads) void scr_label_edge_kernel(Ws w, int r) {
  if (w.ctl->label.done) return;
  const int32_t *hc = w.h[(r - 1) & 1], *kc = w.k[(r - 1) & 1];
  int32_t *hn = w.h[r & 1], *kn = w.k[r & 1];
  bool moved = false;
  for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < w.n_edges; e += (int64_t)gridDim.x * kThreads) {
    const int32_t u = w.e_from[e], v = w.e_to[e];
    // the new labels only fall (H) or rise (K) during the round: a value read
    // here that the old label of the other end does not beat needs no atomic
    const int32_t hv = hc[v], ku = kc[u];
    if (hv < hn[u]) {
      atomicMin(&hn[u], hv);
      moved = true;
    }
    if (ku > kn[v]) {
      atomicMax(&kn[v], ku);
      moved = true;
    }
  }
  note_change(&w.ctl->label.changed, moved);
}

__global__ void scr_round_end_kernel(Phase *p) {
  if (p->done) return;
  p->rounds++;
  if (!p->changed) p->done = 1;
  p->changed = 0;
}

__global__ __launch_bounds__(kThreads) void scr_flag_kernel(Ws w, int b) {
  long long cnt[kCounters] = {0, 0};
  const int32_t *h = w.h[b], *k = w.k[b];
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < w.n_txns; t += (int64_t)gridDim.x * kThreads) {
    const bool node = k[t] >= 0, rt = node && h[t] < k[t];  // (a FAIL txn's K is -1)
    w.mark[t] = rt ? LC_SCREEN_RT : 0;
    w.alive[0][t] = node && !rt;
    cnt[0] += rt;
  }
  flush_counters<kCounters>(cnt, w.counters);
}

__global__ __launch_bounds__(kThreads) void scr_class_kernel(Ws w, int b) {
  const int32_t *h = w.h[b], *k = w.k[b];
  const uint8_t *alive = w.alive[0];
  for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < w.n_edges; e += (int64_t)gridDim.x * kThreads) {
    const int32_t u = w.e_from[e], v = w.e_to[e];
    if (!(alive[u] && alive[v] && h[u] == h[v] && k[u] == k[v])) w.e_from[e] = -1;
  }
}

__global__ __launch_bounds__(kThreads) void scr_trim_edge_kernel(Ws w, int r) {
  if (w.ctl->trim.done) return;
  const uint8_t *alive = w.alive[(r - 1) & 1];
  for (int64_t e = blockIdx.x * (int64_t)kThreads + threadIdx.x; e < w.n_edges; e += (int64_t)gridDim.x * kThreads) {
    const int32_t u = w.e_from[e];
    if (u < 0) continue;
    const int32_t v = w.e_to[e];
    if (alive[u] && alive[v]) {
      w.has_out[u] = 1;
      w.has_in[v] = 1;
    }
  }
}

__global__ __launch_bounds__(kThreads) void scr_trim_node_kernel(Ws w, int r) {
  if (w.ctl->trim.done) return;
  const uint8_t *ac = w.alive[(r - 1) & 1];
  uint8_t *an = w.alive[r & 1];
  bool moved = false;
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < w.n_txns; t += (int64_t)gridDim.x * kThreads) {
    const uint8_t a0 = ac[t], a = a0 & w.has_in[t] & w.has_out[t];
    an[t] = a;
    w.has_in[t] = 0;
    w.has_out[t] = 0;
    moved |= a != a0;
  }
  note_change(&w.ctl->trim.changed, moved);
}

__global__ __launch_bounds__(kThreads) void scr_mark_kernel(Ws w, int b) {
  long long cnt[kCounters] = {0, 0};
  const uint8_t *alive = w.alive[b];
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < w.n_txns; t += (int64_t)gridDim.x * kThreads) {
    if (alive[t]) {
      w.mark[t] |= LC_SCREEN_TRIM;
      cnt[1]++;
    }
  }
  flush_counters<kCounters>(cnt, w.counters);
}

}  // namespace

size_t scan_temp_bytes(int64_t n_txns) {
  size_t a = 0, b = 0;
  int32_t *p = nullptr;
  const size_t n = (size_t)(n_txns > 0 ? n_txns : 1);
  const rocprim::counting_iterator<int32_t> idx(0);
  (void)rocprim::inclusive_scan(nullptr, a, rocprim::make_transform_iterator(idx, Reversed{nullptr, 0}), p, n, MinOp());
  (void)rocprim::inclusive_scan(nullptr, b, rocprim::make_transform_iterator(idx, Through{nullptr, nullptr}), p, n,
                                MaxOp());
  return std::max(a, b);
}

hipError_t launch_setup(const Ws &w, hipStream_t st) {
  scr_setup_kernel<<<grid_for(std::max(w.n_txns, w.n_edges), kThreads), kThreads, 0, st>>>(w);
  return hipGetLastError();
}

hipError_t launch_label_round(const Ws &w, int r, void *temp, size_t temp_bytes, hipStream_t st) {
  const int32_t *hc = w.h[(r - 1) & 1], *kc = w.k[(r - 1) & 1];
  const rocprim::counting_iterator<int32_t> idx(0);
  size_t bytes = temp_bytes;
  hipError_t e = rocprim::inclusive_scan(temp, bytes, rocprim::make_transform_iterator(idx, Reversed{hc, (int32_t)w.n_txns}),
                                         w.s_rev, (size_t)w.n_txns, MinOp(), st);
  if (e != hipSuccess) return e;
  if (w.n_ok > 0) {
    bytes = temp_bytes;
    e = rocprim::inclusive_scan(temp, bytes, rocprim::make_transform_iterator(idx, Through{kc, w.byc}), w.p_inc,
                                (size_t)w.n_ok, MaxOp(), st);
    if (e != hipSuccess) return e;
  }
  scr_label_node_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w, r);
  if (w.n_edges > 0) scr_label_edge_kernel<<<grid_for(w.n_edges, kThreads), kThreads, 0, st>>>(w, r);
  scr_round_end_kernel<<<1, 1, 0, st>>>(&w.ctl->label);
  return hipGetLastError();
}

hipError_t launch_flags(const Ws &w, int b, hipStream_t st) {
  scr_flag_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w, b);
  if (w.n_edges > 0) scr_class_kernel<<<grid_for(w.n_edges, kThreads), kThreads, 0, st>>>(w, b);
  return hipGetLastError();
}

hipError_t launch_trim_round(const Ws &w, int r, hipStream_t st) {
  if (w.n_edges > 0) scr_trim_edge_kernel<<<grid_for(w.n_edges, kThreads), kThreads, 0, st>>>(w, r);
  scr_trim_node_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w, r);
  scr_round_end_kernel<<<1, 1, 0, st>>>(&w.ctl->trim);
  return hipGetLastError();
}

hipError_t launch_marks(const Ws &w, int b, hipStream_t st) {
  scr_mark_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w, b);
  return hipGetLastError();
}

}  // namespace lcscreen
