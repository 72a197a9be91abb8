// watch.h — what lc_watch_check's host code (watch_host.cpp, g++), its driver
// (watch_dev.cpp) and its kernels (watch.hip) share: the log hash, rule 5's
// choice rule, the kernels' geometry, the work records, and the host steps the
// driver runs between the kernels.  The rules are include/lincheck_watch.h's.
#pragma once
#include <stdint.h>

#include <utility>
#include <vector>

#include "../../../include/lincheck_watch.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define LCWT_HD __host__ __device__ __forceinline__
#else
#define LCWT_HD inline
#endif

namespace lcwt {

constexpr int64_t kMaxLen = 0x7FFFFFFF;             // rule 10: logs are shorter
constexpr int64_t kMaxDeviceLen = int64_t(1) << 30; // x + d stays an int32 on the device
constexpr int64_t kDefaultMaxD = 4096;
constexpr int64_t kDefaultTraceBytes = int64_t(1) << 30;

// The kernels' geometry.  A workgroup is kBlock lanes, kWaves waves.  A wave's
// tile of a compare is kTile elements (kTileU per lane); the workgroup's stride
// is kStride.  A lane follows its own snake for kLone steps at most.
constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTileU = 4;
constexpr int kTile = 64 * kTileU;
constexpr int kStride = kWaves * kTile;
constexpr int kLone = 8;

// The log hash: two polynomial hashes mod 2^64 over the mixed elements,
//   H_j(v[0 .. n)) = sum_i mix_j(v[i]) * B_j^(n - 1 - i),
// so (H, B^n) of a concatenation is an associative combination of the parts',
// and a strided pass may sum its lanes' shares in any order.  Order-sensitive;
// equal logs have equal hashes; unequal ones are told apart by the exact
// compare whatever the hashes say.
constexpr uint64_t kBase1 = 0x9E3779B97F4A7C15ull, kBase2 = 0xD6E8FEB86659FD93ull;  // odd

struct Hash {
  uint64_t h1, h2;
};

LCWT_HD uint64_t mix64(uint64_t x) {  // murmur3's 64-bit finaliser
  x ^= x >> 33;
  x *= 0xFF51AFD7ED558CCDull;
  x ^= x >> 33;
  x *= 0xC4CEB9FE1A85EC53ull;
  x ^= x >> 33;
  return x;
}
LCWT_HD uint64_t mix1(int64_t v) { return mix64((uint64_t)v + 0x9E3779B97F4A7C15ull); }
LCWT_HD uint64_t mix2(int64_t v) { return mix64((uint64_t)v ^ 0xC2B2AE3D27D4EB4Full); }
LCWT_HD uint64_t pow64(uint64_t b, uint64_t e) {  // b^e mod 2^64: 31 rounds, e < 2^31
  uint64_t r = 1;
  for (int i = 0; i < 31; i++) {
    if (e & 1) r *= b;
    b *= b;
    e >>= 1;
  }
  return r;
}

// Rule 5's choice on diagonal k of round d, from V_{d-1}[k-1] and V_{d-1}[k+1]
// (the one the rule does not read may be anything): true when the path comes
// down (an insertion).
LCWT_HD bool comes_down(int64_t k, int64_t d, int64_t v_km1, int64_t v_kp1) {
  return k == -d || (k != d && v_km1 < v_kp1);
}
// A round's row of the trace starts at entry d (d + 1) / 2 and holds the
// diagonals -d, -d + 2, .., d in that order.
LCWT_HD int64_t trace_row(int64_t d) { return d * (d + 1) / 2; }
LCWT_HD int64_t trace_entries(int64_t dcap) { return (dcap + 1) * (dcap + 2) / 2; }

// One exact compare: logs values[a_off ..) and values[b_off ..).
struct Pair {
  int64_t a_off, b_off;
  int32_t a_len, b_len;
};
struct PairRes {
  int32_t p, s;  // rule 4's prefix and suffix
};
// One forward pass and backtrack: the middles a = values[a_off .. a_off + n)
// and b = values[b_off .. b_off + m); `base` is p, added to every `at`.
struct Item {
  int64_t a_off, b_off;
  int64_t trace_off;  // entries into the batch's trace
  int64_t edit_off;   // entries into the batch's edits
  int64_t base;
  int32_t n, m;
  int32_t dcap, pad;  // min(max_d, n + m): the pass stops there
};

struct Limits {
  int64_t max_d, trace_bytes;
  uint64_t mask, mask_hi;  // onto Hash::h1 and h2 (the hash as h2 : h1, the environment's mask a 64-bit number)
};
Limits limits();

// 0 or -EINVAL with the text in err.
int validate(const lc_wt_thread *threads, int64_t n_threads, const int64_t *values, int64_t n_values,
             int64_t n_nonmonotonic, uint32_t flags, const lc_wt_out *out, const char **err);

// Rule 2 from proposed classes: threads of one (len, masked hash) form a
// group; each round every undecided thread of a group is compared with the
// group's newest representative; a thread found unequal counts one collision
// and the lowest such becomes the next representative.
struct ClassRounds {
  std::vector<int32_t> cls;
  int64_t n_collisions = 0;
  void init(const lc_wt_thread *threads, int64_t n_threads, const Hash *hashes, uint64_t mask, uint64_t mask_hi);
  // this round's (thread, representative) pairs; empty: the classes are exact
  const std::vector<std::pair<int32_t, int32_t>> &pairs() const { return pairs_; }
  void feed(const std::vector<uint8_t> &equal);  // one per pair, in order

 private:
  std::vector<std::vector<int32_t>> pending_;  // per group, ascending
  std::vector<int32_t> rep_;
  std::vector<std::pair<int32_t, int32_t>> pairs_;
  void make_pairs();
};

// Rule 3: the canonical thread (-1 without threads), its class's size, the number of classes.
int32_t pick_canonical(const lc_wt_thread *threads, int64_t n_threads, const std::vector<int32_t> &cls,
                       int64_t *size, int64_t *n_classes);

// Rules 5 and 6 on the host: the distance of the middles; with max_d >= 0 and
// the distance within it, the script (every at has `base` added) and true in
// *scripted.  max_d < 0: the distance alone, in O(D) memory.
int64_t myers_host(const int64_t *a, int64_t n, const int64_t *b, int64_t m, int64_t max_d, int64_t base,
                   std::vector<lc_wt_edit> *script, bool *scripted);

// One differing thread, as both paths know it before the scripts are placed.
struct Diff {
  int32_t thread;
  bool no_script;
  int64_t dist, p, s;
};
// Rule 7's order, the scripts' offsets, out->cls / distance / deltas and the
// summary but for the times and n_by_host (rules 8 and 9).  With more edits
// than out->edit_cap: -ENOSPC, nothing written to out, *sum zero but n_edits.
// diffs comes back in rule 7's order, aligned with out->deltas.
int place_and_summarize(const lc_wt_thread *threads, int64_t n_threads, int64_t n_nonmonotonic,
                        const std::vector<int32_t> &cls, int32_t canonical, int64_t canonical_size, int64_t n_classes,
                        int64_t n_collisions, std::vector<Diff> *diffs, const lc_wt_out *out, lc_wt_summary *sum);

#if defined(__HIPCC__)
// kernels (watch.hip); every pointer is device memory
hipError_t launch_hashes(const int64_t *values, const int64_t *off, const int32_t *len, int n_threads, Hash *out,
                         hipStream_t st);
hipError_t launch_compare(const int64_t *values, const Pair *pairs, int n_pairs, PairRes *res, hipStream_t st);
// dist[i]: the distance, or -1 when the pass stopped at dcap undone
hipError_t launch_forward(const int64_t *values, const Item *items, int n_items, int32_t *trace, int32_t *dist,
                          hipStream_t st);
// the scripts of the items with dist >= 0
hipError_t launch_backtrack(const int64_t *values, const Item *items, int n_items, const int32_t *trace,
                            const int32_t *dist, lc_wt_edit *edits, hipStream_t st);
#endif

}  // namespace lcwt
