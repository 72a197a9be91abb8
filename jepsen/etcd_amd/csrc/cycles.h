// cycles.h — what lc_cycle_reach's host twin (cycles_host.cpp, g++), its
// driver (cycles_dev.cpp) and its kernel (cycles.hip) share.  The question is
// include/lincheck_cycles.h's.
#pragma once
#include <stdint.h>

#include "../../../include/lincheck_cycles.h"
#include "graph_host.h"

namespace lccyc {

// One workgroup's LDS: a visited bit and a head bit per node, then the window
// of the queue's chunk (the nodes of the chunk whose predecessor lists the
// whole workgroup shares out) and a few words.  Two workgroups per CU have
// 163,840 / 2 = 81,920 bytes each; 2 x 262,144 / 8 = 65,536 bytes of bitmaps
// plus kThreads x 4 = 1,024 bytes of window plus 20 bytes of words are 66,580.
constexpr int kThreads = 256;
constexpr int64_t kMaxNodes = 262144;
constexpr int kMaxWorkgroups = 512;  // 256 CUs x 2
// A predecessor list of more than kLongList entries is left to the whole
// workgroup, kThreads entries a step.
constexpr int kLongList = 64;
// The queues (one int32 per node and workgroup) take at most this many bytes.
constexpr int64_t kQueueBytes = int64_t(256) << 20;
// default_min_work: the least power of two above the measured crossover
// (tools/cycle_search_probe.py's sweep on one MI355X; DESIGN.md §9 has the
// rows).  A deep component costs the device its depth and the host its work,
// so the crossover moves with the candidate count; the largest work at which
// the host loop still won (a tie: 16,384 nodes, 64 candidates) was 3,145,152,
// and the device won every point above it.
constexpr int64_t kDefaultMinWork = int64_t(1) << 22;

// The contract of include/lincheck_cycles.h: 0, or -EINVAL with the text in *err.
int validate(int64_t n_nodes, const int64_t *pred_off, const int32_t *pred, int64_t n_pred, int64_t n_queries,
             const int32_t *q_node, const int64_t *q_head_off, const int32_t *q_heads, int64_t n_heads, uint32_t flags,
             const int32_t *hit, const char **err);

int64_t min_work();

// The workgroups a launch over these counts starts (>= 1).
int workgroups(int64_t n_nodes, int64_t n_queries);

#if defined(__HIPCC__)
// One call's device workspace.
struct Ws {
  int64_t n_nodes, n_queries;
  const int64_t *pred_off;
  const int32_t *pred;
  const int32_t *q_node;
  const int64_t *q_head_off;
  const int32_t *q_heads;
  int32_t *queue;   // workgroups x n_nodes
  int32_t *hit;     // n_queries (LC_REACH_ALL)
  // [0] the least hit so far (INT32_MAX: none), [1] the next query's ticket
  int32_t *words;
  unsigned long long *counts;  // [0] queries run, [1] nodes visited
};

hipError_t launch_reach(const Ws &w, int n_wg, uint32_t flags, hipStream_t st);

// cycles_dev.cpp, for the checkers' drivers: a ReachProblem whose arrays are
// host memory, answered on the context's first device.  0 with *first_hit,
// -E2BIG above kMaxNodes, -ENOMEM or -EIO.
int reach_problem(lc_ctx *c, const lcgraph::ReachProblem &p, int64_t *first_hit);
// The marked pass a restricted call hands to graph_and_summary: the marks, the
// limits of this call, reach_problem as the hook.
void device_pass(lc_ctx *c, const int32_t *mark, lcgraph::MarkedPass *mp);
// What the pass counted (restricted = 1), or all zero for a call that ran none.
lc_cycle_search_summary search_summary(const lcgraph::MarkedPass *mp);
#endif

}  // namespace lccyc
