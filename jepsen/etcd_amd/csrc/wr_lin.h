// wr_lin.h — what lc_wr_check_lin's host code (wr_lin_host.cpp, g++), its
// driver (wr_dev.cpp) and its kernels (wr_lin.hip) share.  The rules are
// include/lincheck_wrlin.h's; everything of lc_wr_check is wr.h's.
#pragma once
#include "../../../include/lincheck_wrlin.h"
#include "wr.h"

namespace lcwr {

constexpr int kWaveKeyVersions = 64;  // a key's rows in one wavefront's registers, a row per lane
// a workgroup's rows in the LDS: 512 rows of 8 words are 32 KiB, so four workgroups fit a CU's 160 KiB
// (DESIGN.md §9 has the choice)
constexpr int kMaxKeyVersions = 512;
constexpr int kMaxRowWords = kMaxKeyVersions / 64;

bool lin_flags_ok(uint32_t flags);
// the records of a call without the lin bit
void lin_zero(lc_wr_lin_key *lin_keys, int64_t n_keys, lc_wr_lin_summary *lin_sum);

// 64-bit words of the keys' bit matrices: the versions number n_mops at most, a row has as many
// words as the largest key it could belong to
inline int64_t lin_matrix_words(int64_t n_mops) {
  const int64_t v = n_mops < kMaxKeyVersions ? n_mops : kMaxKeyVersions;
  return n_mops * ((v + 63) / 64);
}

#if defined(__HIPCC__)
// The lin call's device arrays beside Ws.  "touch" arrays are indexed by mop
// before the sort and by rank after it.
struct LinWs {
  int32_t *vlocal;   // vcap: a version's index among its key's versions
  int32_t *kv;       // kcap + 1: versions per key slot ([kcap] stays 0)
  int32_t *kvoff;    // kcap + 1: kv's prefix sums
  int64_t *kwords;   // kcap + 1: the key's matrix words, V x ceil(V / 64); 0 above the limit
  int64_t *kmoff;    // kcap + 1: kwords' prefix sums
  int32_t *vlist;    // n_mops: version slots grouped by key, local order
  unsigned long long *mat;  // mat_words: the adjacency rows
  int64_t mat_words;
  unsigned long long *tkey, *skey;  // n_mops: kslot << 32 | inv_pos, ~0: no touch; skey sorted
  int32_t *tidx, *sidx;             // n_mops: the mop, and the sorted touches' mops
  int32_t *tcomp, *tfirst, *tlast;  // n_mops, by mop: comp_pos, the slots of first and last
  uint8_t *twfr;                    // n_mops, by mop: the touch has an external read and a write
  int32_t *s_comp, *s_first, *s_last;  // n_mops, by rank
  int32_t *r_ks, *r_comp, *r_suf;  // n_mops, by n_mops - 1 - rank: key slot (-1: no touch), comp, and the
                                   // least comp from the rank to its key's end
  int32_t *plo;                    // n_mops, by rank: the first successor's rank
  int64_t *npairs, *pair_off;      // n_mops + 1: successors per rank, and their prefix sums
  int32_t *kntouch, *ktoff;        // kcap + 1: touches per key slot and their prefix sums
  int32_t *knvedges, *kninit;      // kcap: version edges; initial edges whose tail (nil) nobody read
  lc_wr_lin_key *lin_keys;         // n_mops: records parallel to Ws::keys
};

size_t lin_temp_bytes(int64_t n_mops, uint64_t vcap, uint64_t kcap);
// Everything of launch_rules with rules 4', 6' and 7' in the place of 4, 6
// and 7: status[2] is raised by a key above kMaxKeyVersions, status[3] is the
// most versions of a key; item_off[vcap] is the number of ww / rw items.
// ev0 / ev1 are recorded round the lin steps proper.
hipError_t launch_lin_rules(const Ws &w, const LinWs &l, int32_t *kslots, int64_t *d_n_keys, void *temp,
                            size_t temp_bytes, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st);
// The ww / rw slots: n_items work items into slots[n_mops ..].
hipError_t launch_lin_items(const Ws &w, const LinWs &l, int64_t n_items, hipStream_t st);

// wr.hip: wr_mop_kernel and wr_txn_kernel alone; and wr_keys_kernel alone.
hipError_t launch_tables(const Ws &w, hipStream_t st);
hipError_t launch_key_records(const Ws &w, const int32_t *kslots, const int64_t *d_n_keys, hipStream_t st);
#endif

}  // namespace lcwr
