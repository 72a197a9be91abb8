// runtime.h — what lincheck.cpp (the context and the tiers; it defines the
// functions declared here unless another file is named) shares with the rest
// of the register path (check_host.cpp, frontiers_dev.cpp, whole_gpu.cpp) and
// the side checkers' drivers (*_dev.cpp).  Internal: not installed with
// include/, and lcrt has hidden visibility.
#pragma once
#include <errno.h>
#include <hip/hip_runtime.h>

#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../../include/lincheck.h"
#include "../../../include/lincheck_fx.h"
#include "kernels.h"
#include "counted.h"
#include "events.h"
#include "plan_host.h"
#include "workspace.h"

namespace lcrt __attribute__((visibility("hidden"))) {

// A device buffer with its capacity in bytes (ensure(): at least 256 bytes,
// grow-only, freed at lc_close).  No destructor: lc_open copies a Dev into
// lc_ctx::devs, and lc_close frees every buffer once.
template <class T>
struct Buf {
  T *p = nullptr;
  size_t cap = 0;
};

struct Dev {
  int id = -1;
  hipStream_t stream = nullptr;

  // ---- device buffers (each is named once more, in lc_close's list) ----
  Buf<lc_op> d_ops;
  Buf<int64_t> d_off;
  Buf<lc_key_result> d_out;
  Buf<int32_t> d_ovf, d_ovf2;
  Buf<int32_t> d_jit;
  Buf<int32_t> d_flags;         // per key: handed over by the fast tier (zero between calls)
  Buf<int32_t> d_jit2;          // keys the gap tier passes on
  Buf<int32_t> d_gap2;          // keys the crash-light pass leaves to the gap tier
  Buf<int32_t> d_gws;           // gap-tier workspace
  Buf<char> d_cex;              // gap-tier counterexample intervals + probes
  Buf<void> d_ws;               // HBM tiers' workspace
  Buf<int32_t> d_wit, d_kind;   // lc_check_ex: device copies of the lc_aux outputs
  Buf<int32_t> d_cert, d_cset;  // lc_aux certificates (4 per key), their position sets
  Buf<int32_t> d_cws;           // certificate workspace
  Buf<char> d_ops32;            // copy pipeline: lc_check32 / lc_check16's staging records
  Buf<int64_t> d_base;          // ... and the keys' bases
  Buf<lcdev::WitnessStatus> d_wst;  // LC_FLAG_SEARCH_WITNESS: the stage's status words

  // ---- events ----
  hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
  hipEvent_t ef = nullptr;                  // after the first pass
  hipEvent_t el = nullptr;                  // after the crash-light pass
  hipEvent_t eg = nullptr;                  // after the gap tier
  hipEvent_t eh0 = nullptr, eh1 = nullptr;  // around lc_check's host-to-device copies

  // ---- status words, and what the next call has to know about them ----
  lcdev::KStatus *d_status = nullptr;   // all-zero between calls
  lcdev::KStatus *h_status = nullptr;   // pinned: D2H copies of d_status
  int32_t *h_handoff = nullptr;         // host-coherent: [0] fast tier handed keys over, [1] a fused
                                        // pass's crash-light key count (status_settle_kernel)
  int32_t *h_handoff_dev = nullptr;     // its device address
  bool status_dirty = true;             // d_status may be non-zero
  // the handoff flags may be non-zero (the fast tier raised some and no
  // compaction, which clears them, followed)
  bool flags_dirty = true;
  // A fused call that handed nothing over copies its status without waiting
  // for it (the counts only choose the next call's pass and fill this call's
  // n_gap_keys): the next call, or lc_last_stats, settles it (settle_status).
  hipEvent_t es = nullptr;
  bool st_pending = false;
  int64_t st_keys = 0;
  bool use_fused = false;  // the next call takes the fused version-order + crash-light pass
  // some key of the last run_device call may be LC_INVALID (a key was handed
  // over past the version-order tier, which decides valid keys only): the
  // certificate pass runs only then
  bool maybe_invalid = true;

  // ---- completion signal ----
  // The version-order / fused pass's follower signal (kernels.h
  // launch_done_signal): a host-mapped word the host spins on instead of
  // waiting for an event; the pass's HIP-event time is read later
  // (timing_pending)
  uint32_t *h_done = nullptr, *h_done_dev = nullptr;
  uint32_t seq = 0;
  bool timing_pending = false;

  // ---- resident grid ----
  // the resident version-order grid (kernels.h launch_fast_resident), on its
  // own stream; res_grid: workgroups of the live grid (0: none)
  lcdev::ResHost *res_h = nullptr, *res_h_dev = nullptr;
  lcdev::ResDev *res_d = nullptr;
  hipStream_t rst = nullptr;
  int64_t res_grid = 0;
  uint32_t res_seq = 0;
  int res_khz = 0;          // the device's wall-clock rate
  int64_t res_idle_us = 50; // LC_RESIDENT_IDLE_US (read at each grid launch)
  int64_t res_cap = -1;     // lcdev::fast_resident_capacity() (once)
  bool res_broken = false;  // a request the grid did not complete: launches only from then on

  // ---- copy pipeline ----
  // lc_check's host-to-device pipeline: the copy streams and one event per
  // chunk (its records landed); the staging records are d_ops32 / d_base
  // (two copy streams, chunks alternating: two DMA engines read host memory
  // at once; measured 52-53 GB/s with one, 57 GB/s with two on one GPU)
  hipStream_t cst = nullptr, cst2 = nullptr;
  std::vector<hipEvent_t> cev;
  // lc_check's small calls from pageable memory: inputs and outputs pass
  // through this pinned buffer (kStageMax)
  char *h_stage = nullptr;

  // ---- statistics ----
  double kernel_ms = 0, fast_ms = 0, gap_ms = 0, jit_ms = 0, hbm_ms = 0;
  int64_t n_gap = 0, n_jit = 0, n_hbm = 0;
  int malformed = 0;
  lc_counted_stats counted{};               // this device's share of lc_last_counted_stats
  lc_witness_stats wit{};                   // this device's share of lc_last_witness_stats
  lc_counted_witness_stats cwit{};          // this device's share of lc_last_counted_witness_stats
  lc_device_stats last{};                   // this device's share of the last lc_check
  double t_start = 0, t_end = 0;            // lc_call_profile: this thread's span (ms since the call began)
  // this device's share of lc_last_totals: written only by the device's own
  // thread during a call (check_host runs one per device), summed by
  // lc_last_totals after the threads are joined
  lc_totals tot{};
};

// A side checker's state: one grow-only arena on the context's first device,
// carved into the call's arrays (workspace.h); events and the pinned words
// (the checker's own struct) made by its first call (side_begin);
// release() frees everything (lc_close).  No device pointer outlives a call
// but through EvState::w.
constexpr int kSideEvents = 8;  // (lc_wr_check_lin uses two beside lc_wr_check's six)
struct SideState {
  Buf<char> arena;
  void *pinned = nullptr;
  hipEvent_t ev[kSideEvents] = {};
  template <class T>
  T *words() const {
    return static_cast<T *>(pinned);
  }
};

// lc_check_events / lc_events_pack.  w: the last events_device call's arrays;
// events_copy_out and events_check read the packed records through it, so
// nothing grows the arena in between.  The pinned words are an lcev::Status.
struct EvState : SideState {
  Buf<lc_key_result> d_res;  // events_check's results
  lcev::Ws w{};
  lc_events_stats stats{};
};

void release(SideState &s);
void release(EvState &s);

void set_err(lc_ctx *c, const std::string &s);
// key_off[0] >= 0 and key_off monotone over n_keys > 0 keys, or -EINVAL with
// the context's error naming the call `who`.
int check_offsets(lc_ctx *c, const char *who, const int64_t *key_off, int64_t n_keys);

#define HIP_TRY(ctx, expr)                                                   \
  do {                                                                       \
    hipError_t e_ = (expr);                                                  \
    if (e_ != hipSuccess) {                                                  \
      lcrt::set_err(ctx, std::string(#expr) + ": " + hipGetErrorString(e_)); \
      return -EIO;                                                           \
    }                                                                        \
  } while (0)

template <class T>
int ensure(lc_ctx *c, Buf<T> &b, size_t bytes) {
  if (b.cap >= bytes && b.p) return 0;
  if (b.p) (void)hipFree(b.p);
  b = Buf<T>{};
  const size_t n = bytes > 256 ? bytes : 256;
  hipError_t e = hipMalloc(reinterpret_cast<void **>(&b.p), n);
  if (e != hipSuccess) {
    b.p = nullptr;
    set_err(c, std::string("hipMalloc: ") + hipGetErrorString(e));
    return -ENOMEM;
  }
  b.cap = n;
  return 0;
}

constexpr int64_t kDefaultBudget = 1 << 24;   // configurations per key
// HBM tiers: (configurations per set, concurrent keys).  Workspace per key
// is ~128 B per configuration of capacity (3 regions + 2 hash tables).
// Each tier's workspace is <= 4 GiB; the first has the most waves (the
// lane-parallel expansion is latency-bound per wave).
constexpr int kHbmTiers = 3;
constexpr int64_t kHbmCap[kHbmTiers] = {1 << 14, 1 << 18, 1 << 21};
constexpr int kHbmWaves[kHbmTiers] = {2048, 128, 16};
// A call whose pageable inputs and outputs fit in kStageMax bytes copies them
// through the device's pinned staging buffer (a memcpy on the host, then a
// DMA from pinned memory): the runtime's pageable path costs tens of
// microseconds per copy, which small calls (C1, C4) pay in full.  At a few
// MB the runtime's path is the faster one again (a 4.8 MB input staged:
// 0.07-0.15 ms slower, profiles/r05/stage_ab.txt).
constexpr size_t kStageMax = size_t(2) << 20;

// lc_check's host-to-device pipeline on one device (check_host.cpp): the
// device's key range cut into chunks of about kChunkBytes of records
// (plan_host.h).  run_device calls issue(i), which enqueues chunk i's record
// copy on the copy stream and records ready[i]; the compute stream waits for
// that event, widens 24-byte records (lc_check32), and runs the version-order
// (or fused) pass over the chunk's keys while the copy engine moves the next
// chunk.  (A pageable copy may block the issuing thread until it has landed;
// issuing each chunk's copy right before its kernels keeps the overlap
// either way.)
struct Chunks : ChunkPlan {
  std::function<int(int)> issue;
  const hipEvent_t *ready = nullptr;
  const lc_op32 *d_ops32 = nullptr;  // staging records to widen into d_ops (null: 48-byte copies)
  const lc_op16 *d_ops16 = nullptr;  // (lc_check16) the same for 16-byte records
  const int64_t *d_base = nullptr;   // key bases for the widening (null: 0)
  int64_t max_len = 0;               // longest key (records)
};

// Device-side lc_aux outputs of one run_device call (null: not wanted).
struct AuxOut {
  int32_t *wit = nullptr;   // per record, indexed like d_ops
  int32_t *kind = nullptr;  // per key
  int32_t *cert = nullptr;  // per key, 4 int32 (infeasibility certificates)
  int32_t *cset = nullptr;  // per record (HALL position sets)
  int64_t n_records = 0;
};

// Where a run_device call's records come from, beyond d_ops / d_off
// (default: 48-byte records in place, offsets on the device only).
struct Source {
  // the shard's key offsets in host memory when the caller has them
  // (lc_check_ex): the gap tier may then be launched early
  const int64_t *h_off = nullptr;
  // lc_check's chunked copies, or null: the records are in place
  const Chunks *chunks = nullptr;
  // the first pass over lc_op32 records (lc_check32 / lc_check_device32
  // without lc_aux outputs): ops32 and the keys' bases (null: 0), indexed
  // like d_ops / d_off; `widen` fills the 48-byte records the later tiers
  // read (and names them) once a key is handed over
  const lc_op32 *ops32 = nullptr;
  const int64_t *base32 = nullptr;
  std::function<int(const lc_op **)> widen;
};

bool env_is_off(const char *name);
int opts_to_params(lc_ctx *c, const lc_opts *o, lcdev::KParams *p);
bool is_pinned(lc_ctx *c, const void *p, size_t n);
char *stage_buf(lc_ctx *c, Dev &d);
int64_t settle_status(Dev &d);
void settle_timing(lc_ctx *c, Dev &d);
int read_status(lc_ctx *c, Dev &d, hipStream_t st);
void fill_stats(lc_stats &s, const Dev &d);
int res_stop(lc_ctx *c, Dev &d);
int run_device(lc_ctx *c, Dev &d, const lc_op *d_ops, const int64_t *d_off, int64_t n_keys,
               const lcdev::KParams &p, lc_key_result *d_out, hipStream_t st, int64_t flags,
               const AuxOut &ao = AuxOut(), const Source &src = Source());
int run_certificates(lc_ctx *c, Dev &d, const lc_op *d_ops, const int64_t *d_off, int64_t n_keys,
                     const lcdev::KParams &p, const lc_key_result *d_out, hipStream_t st,
                     const AuxOut &wo);

// whole_gpu.cpp — LC_FLAG_WHOLE_GPU: the keys of `todo` searched again by
// the frontier exchange; fetch(k, records) and store(k, result) move a key
// between the caller's memory (host or device) and the engine.
int whole_gpu(lc_ctx *c, const std::vector<int64_t> &todo, const lc_opts *opts,
              const std::function<int(int64_t, std::vector<lc_op> &)> &fetch,
              const std::function<int(int64_t, const lc_key_result &)> &store);
void unknown_keys(const lc_key_result *res, int64_t n_keys, std::vector<int64_t> &budget,
                  std::vector<int64_t> &window);
int whole_gpu_device(lc_ctx *c, const lc_op *d_ops, const int64_t *d_key_off, int64_t n_keys,
                     const lc_opts *opts, lc_key_result *d_out, int32_t *d_cert, hipStream_t st);
int check_device(lc_ctx *c, const char *who, const void *ops, bool rec32, const int64_t *d_key_off,
                 const int64_t *d_key_base, int64_t n_keys, const lc_opts *opts, lc_key_result *d_out,
                 void *stream, const lc_aux *aux);

// How a side checker's call begins: the context's first device selected, a
// pending status settled, the resident grid gone (it leaves before other
// work runs).  *st is that device's stream.
int side_begin(lc_ctx *c, hipStream_t *st);
// The same for a checker with a state of its own, whose first n_events events
// and pinned_bytes of pinned words are made where they are missing.
int side_begin(lc_ctx *c, SideState &s, int n_events, size_t pinned_bytes, hipStream_t *st);

// A side checker's entry point: body(), with the host's std::bad_alloc (its
// arrays are sized by the caller's arguments) as -ENOMEM and the call's name
// in the context's error.
template <class Body>
int no_bad_alloc(lc_ctx *c, const char *who, Body body) {
  try {
    return body();
  } catch (const std::bad_alloc &) {
    set_err(c, std::string(who) + ": out of host memory");
    return -ENOMEM;
  }
}

// An input's device copy, which the kernels only read (const in their Ws), as
// the destination of the host's copy.
template <class T>
inline T *writable(const T *p) {
  return const_cast<T *>(p);
}

// The time between two recorded events that have completed, or 0.
inline float elapsed_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0;
}

}  // namespace lcrt

struct lc_ctx {
  std::vector<lcrt::Dev> devs;
  // LC_FLAG_WHOLE_GPU: frontier-exchange engines, opened on first use —
  // single-GPU ones (engine, device) and one over every GPU of the context
  std::vector<std::pair<lc_fx *, int>> fxs;
  lc_fx *fx_all = nullptr;
  bool fx_all_failed = false;
  std::string err;
  std::mutex err_mu;
  lc_stats stats{};
  // lc_host_register: caller buffers page-locked for this context's devices
  std::vector<std::pair<const char *, uint64_t>> pinned;
  std::mutex pin_mu;
  lc_call_profile prof{};  // lc_last_call_profile
  lcrt::EvState evs;       // lc_check_events
  lcrt::SideState sfs;     // lc_set_full
  lcrt::SideState aps;     // lc_append_check
  lcrt::SideState wrs;     // lc_wr_check
  lcrt::SideState wts;     // lc_watch_check
  lcrt::SideState pfs;     // lc_perf_stats
  lcrt::SideState scs;     // lc_cycle_screen
  lcrt::SideState cys;     // lc_cycle_reach
};
