// screen.h — what lc_cycle_screen's host twin (screen_host.cpp, g++), its
// driver (screen_dev.cpp) and its kernels (screen.hip) share.  The method is
// include/lincheck_screen.h's.  The txn and edge records, the edges' order,
// the sharded counters' geometry and real time's launcher are txngraph.h's.
#pragma once
#include <stdint.h>

#include "../../../include/lincheck_screen.h"
#include "txngraph.h"

namespace lcscreen {

using namespace lctg;

// default_max_rounds: the least power of two that is at least twice the
// largest round count the two 10^6-txn valid probe histories needed
// (tools/screen_probe.py; DESIGN.md §9 has the figures): list-append took 6
// label and 4 trim rounds, rw-register 5 and 3, so 2 x 6 = 12 and 16.
constexpr int32_t kDefaultMaxRounds = 16;
constexpr int32_t kNoComp = INT32_MAX;  // H where no OK txn is reachable
constexpr int32_t kNoInv = -1;          // K's identity: positions are >= 0
constexpr int kCounters = 2;            // txns with LC_SCREEN_RT, txns with LC_SCREEN_TRIM
constexpr int kBatch = 4;               // rounds the driver launches between two looks at the control words

// The contract of include/lincheck_screen.h: 0, or -EINVAL with the text in
// *err.  *n_ok receives the number of OK txns.
int validate(const lc_ap_txn *txns, int64_t n_txns, const lc_ap_edge *edges, int64_t n_edges,
             const lc_screen_out *out, int64_t *n_ok, const char **err);

int32_t max_rounds();

// The summary of a call without txns: clean, no rounds.
inline lc_screen_summary empty_summary() {
  lc_screen_summary s{};
  s.clean = 1;
  s.max_rounds = max_rounds();
  return s;
}

#if defined(__HIPCC__)
// The control words of a phase (the labels, then the trim), on the device.
// A round's kernels return at once when `done` is set; the round's last
// kernel counts the round, and sets `done` where nothing raised `changed`.
struct Phase {
  int32_t done, rounds, changed, pad;
};
struct Control {
  Phase label, trim;
};

// One call's device workspace.
struct Ws {
  const lc_ap_txn *txns;
  const lc_ap_edge *edges;
  const int32_t *byc, *rt_hi;  // launch_real_time's
  int64_t n_txns, n_edges, n_ok;
  int32_t *e_from, *e_to;      // n_edges: the edges' ends; from is -1 once the edge is out of class
  int32_t *first;              // n_txns: first(u) of an OK txn
  int32_t *h[2], *k[2];        // n_txns: the labels, round r reading [~r & 1] and writing [r & 1] (r from 1)
  int32_t *s_rev;              // n_txns: s_rev[i] is the least H among the last i + 1 txns
  int32_t *p_inc;              // n_ok: p_inc[i] is the greatest K among byc[0 .. i]
  uint8_t *alive[2];           // n_txns: the trim's survivors, double-buffered as the labels are
  uint8_t *has_in, *has_out;   // n_txns: zero between rounds
  int32_t *mark;               // n_txns
  int64_t *counters;           // kCounters x kCounterShards x kCounterStride
  Control *ctl;
};

size_t scan_temp_bytes(int64_t n_txns);
// The edges' ends, first(u), round 0's labels.
hipError_t launch_setup(const Ws &w, hipStream_t st);
// Label round r (from 1).
hipError_t launch_label_round(const Ws &w, int r, void *temp, size_t temp_bytes, hipStream_t st);
// The labels final in buffer b: bit 0 and its count, round 0's survivors, the edges out of class.
hipError_t launch_flags(const Ws &w, int b, hipStream_t st);
// Trim round r (from 1).
hipError_t launch_trim_round(const Ws &w, int r, hipStream_t st);
// The survivors final in buffer b: bit 1 and its count.
hipError_t launch_marks(const Ws &w, int b, hipStream_t st);

// screen_dev.cpp, for the checkers' drivers: the screen over txns, unique
// edges, byc and rt_hi that stand on the device (stream st); *scr receives the
// summary (h2d_ms 0) and, where clean == 0 and h_mark is given, h_mark the
// marks (n_txns words of host memory).  n_txns > 0.  0, -ENOMEM or -EIO.
int screen_resident(lc_ctx *c, hipStream_t st, const lc_ap_txn *d_txns, int64_t n_txns, int64_t n_ok,
                    const lc_ap_edge *d_edges, int64_t n_edges, const int32_t *d_byc, const int32_t *d_rt_hi,
                    lc_screen_summary *scr, int32_t *h_mark = nullptr);
#endif

}  // namespace lcscreen
