// events.h — launchers of the event kernels (events.hip): the per-key split
// and history completion of lc_check_events (include/lincheck_events.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../../include/lincheck.h"

namespace lcev {

constexpr int kLdsEvents = 4096;  // a key's positions sorted in LDS up to this many events
constexpr int kLdsProcs = 1024;   // distinct processes of one key the LDS table holds
constexpr int kThreads = 256;

// Zero before every call; read back once after the last kernel.
struct Status {
  int32_t err;       // 1: a key outside [-1, n_keys); 2: a type above 3
  int32_t err_pos;   // the position of one such event
  int64_t n_client, n_invoke, n_ops, n_fail, n_ignored, n_big;
};

// The device workspace of one call over n events and k keys (k == 1: the
// subhistory is the whole array in place, and cnt / cursor / seg_off / seg
// are not used).
struct Ws {
  const lc_event *ev;
  int64_t n, k;
  int32_t *cnt, *cursor;       // per key: client events, scatter tickets (zeroed per call)
  int64_t *seg_off;            // k + 1: the keys' segments of seg / match
  uint32_t *seg;               // n: the positions of each key's events
  int32_t *match;              // n, indexed like seg: an invoke's completion (index in the
                               // segment), -1 none, -2 dropped with its FAIL completion
  unsigned long long *gtab;    // 2 n: the global-memory home of the process tables
  int32_t *nops, *nfail, *nign;  // per key
  int64_t *key_off, *key_base;
  lc_op32 *ops32;              // n
  int32_t *completion;         // n
  Status *status;
};

// Enqueues every kernel of the split / completion / packing on `st`.
hipError_t launch_events(const Ws &w, hipStream_t st);

}  // namespace lcev
