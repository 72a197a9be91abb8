// cycles.hip — lc_cycle_reach's kernel (cycles.h; the question is
// include/lincheck_cycles.h's).
//
//  cyc_reach_kernel: a workgroup takes queries by ticket (an atomicAdd on one
//    word, so they are taken in ascending order) and searches one at a time,
//    breadth first along the predecessor lists.  A visited bit and a head bit
//    per node stand in LDS; the head bits are set from the query's head list
//    and cleared by the same list, the visited bits are cleared by the queue,
//    so a query costs what it visits, not n_nodes.  The frontier is a queue
//    (the workgroup's slab of w.queue: every node enters it once, so n_nodes
//    entries hold it and it never wraps), taken kThreads nodes a pass, a node
//    a lane.  A lane walks a short predecessor list itself; the nodes of the
//    pass with more than kLongList predecessors go to the LDS window, and the
//    whole workgroup then walks each of their lists kThreads entries a step.
//    A node that meets its head bit raises the query's hit word; the query's
//    thread 0 lowers the launch's result word by atomicMin.  Without
//    LC_REACH_ALL a workgroup reads that word before a query (a ticket above
//    it ends the workgroup: later tickets are higher still) and once a pass
//    (the query is dropped), and a search ends with its first head.  The
//    result is exact either way, because the word only falls and a query is
//    dropped only for a hit below it.
//
// Every loop is bounded by a node, edge or query count; no workgroup waits for
// another; results leave through vector stores, a 32-bit atomicMin and a
// 32-bit atomicAdd.  The host has checked every node id against n_nodes
// before the launch (lccyc::validate), and n_nodes against kMaxNodes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "cycles.h"

namespace lccyc {

namespace {

constexpr int kWords = (int)(kMaxNodes / 32);

struct Shared {
  uint32_t vis[kWords], head[kWords];
  int32_t window[kThreads];  // the pass's nodes with a long predecessor list
  int32_t tail, n_long, hit, query, stop;
};

__device__ __forceinline__ void visit(Shared &s, int32_t *queue, int32_t a) {
  const uint32_t bit = 1u << (a & 31);
  const uint32_t old = atomicOr(&s.vis[a >> 5], bit);
  if (old & bit) return;
  if (s.head[a >> 5] & bit) s.hit = 1;
  queue[atomicAdd(&s.tail, 1)] = a;  // below n_nodes: a node enters once
}

__global__ __launch_bounds__(kThreads) void cyc_reach_kernel(Ws w, uint32_t flags) {
  __shared__ Shared s;
  const int tid = threadIdx.x;
  const bool all = flags & LC_REACH_ALL;
  const int32_t n_nodes = (int32_t)w.n_nodes, n_queries = (int32_t)w.n_queries;
  const int32_t n_words = (n_nodes + 31) >> 5;
  for (int32_t i = tid; i < n_words; i += kThreads) s.vis[i] = s.head[i] = 0;
  int32_t *queue = w.queue + (int64_t)blockIdx.x * n_nodes;
  unsigned long long n_run = 0, n_visited = 0;  // thread 0's
  for (int32_t it = 0; it < n_queries; it++) {  // (a workgroup takes at most every query)
    __syncthreads();
    if (tid == 0) {
      // (unsigned: every workgroup takes one ticket past the last query, and n_queries may be near 2^31)
      const uint32_t q = atomicAdd(reinterpret_cast<uint32_t *>(&w.words[1]), 1u);
      const bool go = q < (uint32_t)n_queries &&
                      (all || (int32_t)q <= __hip_atomic_load(&w.words[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
      s.query = go ? (int32_t)q : -1;
      s.tail = 1;
      s.n_long = 0;
      s.hit = 0;
      s.stop = 0;
    }
    __syncthreads();
    const int32_t q = s.query;
    if (q < 0) break;
    const int32_t src = w.q_node[q];
    const int64_t h0 = w.q_head_off[q], h1 = w.q_head_off[q + 1];
    for (int64_t i = h0 + tid; i < h1; i += kThreads) {
      const int32_t h = w.q_heads[i];
      atomicOr(&s.head[h >> 5], 1u << (h & 31));
    }
    if (tid == 0) {
      s.vis[src >> 5] = 1u << (src & 31);
      queue[0] = src;
    }
    __syncthreads();
    int32_t done = 0, tail = 1, hit = 0;
    // a pass takes at least one node off the queue: n_nodes passes at most
    for (int32_t pass = 0; pass < n_nodes && done < tail; pass++) {
      const int32_t cnt = min(kThreads, tail - done);
      if (tid < cnt) {
        const int32_t b = queue[done + tid];
        const int64_t lo = w.pred_off[b], hi = w.pred_off[b + 1];
        if (hi - lo > kLongList)
          s.window[atomicAdd(&s.n_long, 1)] = b;
        else
          for (int64_t i = lo; i < hi; i++) visit(s, queue, w.pred[i]);
      }
      if (tid == 0 && !all)
        s.stop = q > __hip_atomic_load(&w.words[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __syncthreads();
      const int32_t n_long = s.n_long;  // at most cnt
      for (int32_t j = 0; j < n_long; j++) {
        const int32_t b = s.window[j];
        const int64_t lo = w.pred_off[b], hi = w.pred_off[b + 1];
        for (int64_t i = lo + tid; i < hi; i += kThreads) visit(s, queue, w.pred[i]);
      }
      __syncthreads();
      done += cnt;
      tail = s.tail;
      hit = s.hit;
      const int32_t stop = s.stop;
      if (tid == 0) s.n_long = 0;
      __syncthreads();
      if (!all && (hit || stop)) {
        hit = stop ? 0 : hit;  // (a dropped query reports nothing; a lower hit stands)
        break;
      }
    }
    // the bits this query set, cleared by what set them
    for (int32_t i = tid; i < tail; i += kThreads) s.vis[queue[i] >> 5] = 0;
    for (int64_t i = h0 + tid; i < h1; i += kThreads) s.head[w.q_heads[i] >> 5] = 0;
    if (tid == 0) {
      if (hit) atomicMin(&w.words[0], q);
      if (all) w.hit[q] = hit;
      n_run++;
      n_visited += (unsigned long long)tail;
    }
  }
  if (tid == 0) {
    w.counts[2 * blockIdx.x] = n_run;
    w.counts[2 * blockIdx.x + 1] = n_visited;
  }
}

}  // namespace

hipError_t launch_reach(const Ws &w, int n_wg, uint32_t flags, hipStream_t st) {
  hipLaunchKernelGGL(cyc_reach_kernel, dim3((unsigned)n_wg), dim3(kThreads), 0, st, w, flags);
  return hipGetLastError();
}

}  // namespace lccyc
