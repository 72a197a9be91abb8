// wr_lin.hip — the kernels of lc_wr_check_lin (include/lincheck_wrlin.h): rules
// 4', 6' and 7'.  Rules 1-3 and 5, the tables and the wr slots are wr.hip's
// wr_mop_kernel and wr_txn_kernel (launch_tables); the key records are its
// wr_keys_kernel (launch_key_records).
//
// What changes against wr.hip: with real-time edges a version has many parents,
// so a key's version graph is no set of parent pointers any more.  It is a bit
// matrix, a row per version, and rule 6' is Warshall's closure of it.
//
//  lin_vlocal_kernel (a thread per version slot): the version's index among
//    its key's versions, by a counter per key.  The order is arbitrary; nothing
//    that leaves the device depends on it.
//  lin_kshape_kernel (a thread per key slot): the key's matrix words; a key
//    above kMaxKeyVersions raises status[2] and gets none.  Two scans give the
//    keys' offsets into the version list and the matrices; lin_vlist_kernel
//    fills the list.
//  lin_touch_kernel (a thread per txn): for each mop that is an OK txn's first
//    on its key a touch at the mop's index — no atomics but the key's count.
//    A radix sort by (key slot, inv_pos) groups them; lin_gather_kernel brings
//    the fields along, and comp_pos mirrored, so that one forward segmented
//    min-scan is the suffix minimum rule 4''s range form needs.
//  lin_range_kernel (a thread per touch): two binary searches inside the
//    touch's segment: its successors' ranks [lb, ub).  A scan: pair offsets.
//  lin_edge_kernel (a thread per mop): the initial and the wfr edges' bits.
//  lin_pair_kernel: one work item per key-successor pair, found through the
//    prefix sums as wr_item_kernel finds its items; no thread loops over a
//    range.  Bits are set by 64-bit atomicOr, so the graph is a set for free.
//  lin_close_wave_kernel: a wavefront per key of at most 64 versions, lane i
//    holding row i in one 64-bit register; Warshall in V steps with the pivot
//    row broadcast across the wave; no LDS, no barrier.
//  lin_close_block_kernel: a workgroup per larger key, rows in the LDS, a
//    barrier before the first pivot and one after each.
//    Both leave the children count per version (the row's popcount before the
//    closure), the key's edge count, the cyclic flag and cyc_value; the
//    matrices keep the adjacency.
//  lin_readers_kernel, lin_rc_kernel and two scans: the readers' groups and
//    the items' prefix sums: (readers(a) + [a has a writer]) x children(a), 0
//    under a cyclic key — a version's writer is one more "reader", of type ww.
//  lin_item_kernel: an item's child is the j-th set bit of the adjacency row;
//    a child without a writer leaves its slot empty.
//  lin_keys_kernel: the lc_wr_lin_key records.
//
// Every loop is bounded by a txn, mop, version, word, touch or table count;
// no workgroup waits for another; results leave through vector stores and
// 32- / 64-bit vector atomics.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_scan_by_key.hpp>

#include <algorithm>

#include "txngraph_dev.h"
#include "wr_lin.h"

namespace lcwr {

namespace {

constexpr unsigned long long kSign = 1ull << 63;  // value ^ this: unsigned order is the int64 order
constexpr unsigned long long kNoTouch = ~0ull;
constexpr int32_t kNoComp = 0x7FFFFFFF;

struct MinOp {
  __host__ __device__ int32_t operator()(int32_t a, int32_t b) const { return a < b ? a : b; }
};

__global__ __launch_bounds__(kThreads) void lin_vlocal_kernel(Ws w, LinWs l) {
  for (int64_t s = blockIdx.x * (int64_t)kThreads + threadIdx.x; s < (int64_t)w.vcap;
       s += (int64_t)gridDim.x * kThreads) {
    const unsigned long long word = w.vtab[s];
    if (word == kEmptyWord) continue;
    l.vlocal[s] = atomicAdd(&l.kv[w.mop_kslot[(uint32_t)word]], 1);
  }
}

__global__ __launch_bounds__(kThreads) void lin_kshape_kernel(Ws w, LinWs l) {
  int32_t most = 0;
  for (int64_t s = blockIdx.x * (int64_t)kThreads + threadIdx.x; s < (int64_t)w.kcap;
       s += (int64_t)gridDim.x * kThreads) {
    const int64_t v = l.kv[s];
    most = v > most ? (int32_t)v : most;
    l.kwords[s] = v > kMaxKeyVersions ? 0 : v * ((v + 63) >> 6);
  }
  if (most > kMaxKeyVersions) w.status[2] = 1;
  if (most) atomicMax(&w.status[3], most);
}

__global__ __launch_bounds__(kThreads) void lin_vlist_kernel(Ws w, LinWs l) {
  for (int64_t s = blockIdx.x * (int64_t)kThreads + threadIdx.x; s < (int64_t)w.vcap;
       s += (int64_t)gridDim.x * kThreads) {
    const unsigned long long word = w.vtab[s];
    if (word == kEmptyWord) continue;
    const int64_t at = (int64_t)l.kvoff[w.mop_kslot[(uint32_t)word]] + l.vlocal[s];
    if (at < w.n_mops) l.vlist[at] = (int32_t)s;  // (always: a version has a mop of its own)
  }
}

__global__ __launch_bounds__(kThreads) void lin_iota_kernel(Ws w, LinWs l) {
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    l.tkey[m] = kNoTouch;
    l.tidx[m] = (int32_t)m;
  }
}

__global__ __launch_bounds__(kThreads) void lin_touch_kernel(Ws w, LinWs l) {
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < w.n_txns; t += (int64_t)gridDim.x * kThreads) {
    const lc_wr_txn x = w.txns[t];
    if (x.type != LC_WR_OK) continue;
    const int64_t end = x.mop_off + x.mop_len;
    for (int64_t m = x.mop_off; m < end; m++) {
      const lc_wr_mop o = w.mops[m];
      bool first_on_key = true;
      for (int64_t j = x.mop_off; j < m; j++)
        if (w.mops[j].key == o.key) first_on_key = false;
      if (!first_on_key) continue;
      int64_t mb = -1;  // the txn's external write of the key
      for (int64_t j = m; j < end; j++)
        if (w.mops[j].f == LC_WR_WRITE && w.mops[j].key == o.key) mb = j;
      const int32_t ext = o.f == LC_WR_READ ? w.mop_vslot[m] : -1;
      const int32_t wv = mb >= 0 ? w.mop_vslot[mb] : -1;
      const int32_t first = ext >= 0 ? ext : wv, last = wv >= 0 ? wv : ext;
      if (first < 0 || last < 0) continue;  // (never: an OK txn's read is known, a write has its version)
      const int32_t ks = w.mop_kslot[m];
      l.tkey[m] = ((unsigned long long)(uint32_t)ks << 32) | (uint32_t)x.inv_pos;
      l.tcomp[m] = (int32_t)x.comp_pos;
      l.tfirst[m] = first;
      l.tlast[m] = last;
      l.twfr[m] = ext >= 0 && wv >= 0;
      atomicAdd(&l.kntouch[ks], 1);
    }
  }
}

__global__ __launch_bounds__(kThreads) void lin_gather_kernel(Ws w, LinWs l) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < w.n_mops; i += (int64_t)gridDim.x * kThreads) {
    const unsigned long long key = l.skey[i];
    const int64_t r = w.n_mops - 1 - i;
    if (key == kNoTouch) {
      l.r_ks[r] = -1;
      l.r_comp[r] = kNoComp;
      continue;
    }
    const int32_t m = l.sidx[i];
    l.s_comp[i] = l.tcomp[m];
    l.s_first[i] = l.tfirst[m];
    l.s_last[i] = l.tlast[m];
    l.r_ks[r] = (int32_t)(key >> 32);
    l.r_comp[r] = l.tcomp[m];
  }
}

__global__ __launch_bounds__(kThreads) void lin_range_kernel(Ws w, LinWs l) {
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < w.n_mops; i += (int64_t)gridDim.x * kThreads) {
    const unsigned long long key = l.skey[i];
    if (key == kNoTouch) continue;  // (npairs was zeroed)
    const int32_t ks = (int32_t)(key >> 32);
    const int64_t s1 = (int64_t)l.ktoff[ks] + l.kntouch[ks];  // the segment's end; i lies inside it
    const uint32_t comp = (uint32_t)l.s_comp[i];
    int64_t lo = i + 1, hi = s1 < w.n_mops ? s1 : w.n_mops;  // the first rank invoked after comp
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((uint32_t)l.skey[mid] > comp) hi = mid;
      else lo = mid + 1;
    }
    const int64_t lb = lo;
    hi = s1 < w.n_mops ? s1 : w.n_mops;
    if (lb >= hi) continue;
    const uint32_t least = (uint32_t)l.r_suf[w.n_mops - 1 - lb];  // the least comp among them
    while (lo < hi) {  // the first rank invoked at or after it
      const int64_t mid = (lo + hi) >> 1;
      if ((uint32_t)l.skey[mid] < least) lo = mid + 1;
      else hi = mid;
    }
    l.plo[i] = (int32_t)lb;
    l.npairs[i] = lo - lb;
  }
}

// the bit of version edge a -> b (slots of one key's versions)
__device__ __forceinline__ void set_edge(const Ws &w, const LinWs &l, int32_t ks, int32_t a, int32_t b) {
  const int64_t v = l.kv[ks];
  if (v > kMaxKeyVersions) return;
  const int64_t la = l.vlocal[a], lb = l.vlocal[b];
  const int64_t at = l.kmoff[ks] + la * ((v + 63) >> 6) + (lb >> 6);
  if (la < v && lb < v && at < l.mat_words) atomicOr(&l.mat[at], 1ull << (lb & 63));
}

__global__ __launch_bounds__(kThreads) void lin_edge_kernel(Ws w, LinWs l) {
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    const int32_t ks = w.mop_kslot[m];
    if ((w.flags & LC_WR_WFR_KEYS) && l.tkey[m] != kNoTouch && l.twfr[m])
      set_edge(w, l, ks, l.tfirst[m], l.tlast[m]);  // (a self-loop where they are one)
    const lc_wr_mop o = w.mops[m];
    if (o.f != LC_WR_WRITE || w.txns[w.mop_txn[m]].type == LC_WR_FAIL) continue;
    const int32_t ns = pair_find(w.vtab, w.vcap, w.mops, o.key, kReserved);
    if (ns >= 0) set_edge(w, l, ks, ns, w.mop_vslot[m]);
    else atomicAdd(&l.kninit[ks], 1);
  }
}

// The largest s in [lo, hi] with off[s] <= i (off[lo] <= i holds).
__device__ __forceinline__ int64_t owner_of(const int64_t *__restrict__ off, int64_t lo, int64_t hi, int64_t i) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void lin_pair_kernel(Ws w, LinWs l) {
  const int64_t n_items = l.pair_off[w.n_mops];
  const int64_t n_chunks = (n_items + kItemChunk - 1) / kItemChunk;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t i0 = c * kItemChunk;
    const int64_t i1 = i0 + kItemChunk < n_items ? i0 + kItemChunk : n_items;
    const int64_t r_lo = owner_of(l.pair_off, 0, w.n_mops - 1, i0);
    const int64_t r_hi = owner_of(l.pair_off, r_lo, w.n_mops - 1, i1 - 1);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
      const int64_t r = owner_of(l.pair_off, r_lo, r_hi, i);
      const int64_t j = i - l.pair_off[r];
      if (j < 0 || j >= l.npairs[r]) continue;  // (never: the sums are of these counts)
      const int64_t r2 = (int64_t)l.plo[r] + j;
      if (r2 >= w.n_mops) continue;
      const int32_t a = l.s_last[r], b = l.s_first[r2];
      if (a != b) set_edge(w, l, (int32_t)(l.skey[r] >> 32), a, b);
    }
  }
}

__device__ __forceinline__ unsigned long long enc_value(const Ws &w, int32_t vs) {
  const int64_t v = w.mops[(uint32_t)w.vtab[vs]].value;
  return v == kReserved ? ~0ull : (unsigned long long)v ^ kSign;  // (nil is on no key's record)
}

__device__ __forceinline__ void key_verdict(const Ws &w, const LinWs &l, int64_t s, int32_t n_vedges, bool cyclic,
                                            unsigned long long cyc) {
  l.knvedges[s] = n_vedges + l.kninit[s];
  if (!cyclic) return;  // (every cycle holds a non-nil value: cyc is one)
  w.kflags[s] |= LC_WR_K_CYCLIC;  // (beside wr_txn_kernel's lost-update bit; that kernel is done)
  if (cyc < w.kcyc[s]) w.kcyc[s] = cyc;
}

__global__ __launch_bounds__(kThreads) void lin_close_wave_kernel(Ws w, LinWs l, const int32_t *__restrict__ kslots,
                                                                  const int64_t *__restrict__ n_keys) {
  const int lane = threadIdx.x & 63;
  const int64_t n = *n_keys < w.n_mops ? *n_keys : w.n_mops;
  for (int64_t i = blockIdx.x * (int64_t)kWaves + (threadIdx.x >> 6); i < n; i += (int64_t)gridDim.x * kWaves) {
    const int64_t s = kslots[i];
    const int32_t v = l.kv[s];
    if (v > kWaveKeyVersions) continue;  // (the whole wave)
    unsigned long long row = 0;
    int32_t vs = -1;
    if (lane < v && l.kmoff[s] + lane < l.mat_words) {
      row = l.mat[l.kmoff[s] + lane];
      vs = l.vlist[l.kvoff[s] + lane];
      w.vnchild[vs] = __popcll(row);
    }
    int32_t n_vedges = __popcll(row);
    for (int o = 32; o; o >>= 1) n_vedges += __shfl_xor(n_vedges, o);
    for (int p = 0; p < v; p++) {
      const unsigned long long pivot = __shfl(row, p);
      if ((row >> p) & 1) row |= pivot;
    }
    const bool on = vs >= 0 && ((row >> lane) & 1);  // the version reaches itself
    unsigned long long cyc = on ? enc_value(w, vs) : ~0ull;
    const bool cyclic = __ballot(on) != 0;
    for (int o = 32; o; o >>= 1) {
      const unsigned long long other = __shfl_xor(cyc, o);
      cyc = other < cyc ? other : cyc;
    }
    if (lane == 0) key_verdict(w, l, s, n_vedges, cyclic, cyc);
  }
}

__global__ __launch_bounds__(kThreads) void lin_close_block_kernel(Ws w, LinWs l, const int32_t *__restrict__ kslots,
                                                                   const int64_t *__restrict__ n_keys) {
  // a row has kMaxRowWords words whatever the key's size: a word's row and column are shifts
  __shared__ unsigned long long rows[kMaxKeyVersions * kMaxRowWords];
  __shared__ unsigned long long s_cyc;
  __shared__ int32_t s_vedges, s_cyclic;
  const int64_t n = *n_keys < w.n_mops ? *n_keys : w.n_mops;
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    const int64_t s = kslots[i];
    const int32_t v = l.kv[s];
    if (v <= kWaveKeyVersions || v > kMaxKeyVersions) continue;  // (the whole workgroup)
    const int32_t words = (v + 63) >> 6;
    const int64_t base = l.kmoff[s];
    if (threadIdx.x == 0) {
      s_cyc = ~0ull;
      s_vedges = s_cyclic = 0;
    }
    for (int32_t e = threadIdx.x; e < v * kMaxRowWords; e += kThreads) {
      const int32_t r = e / kMaxRowWords, c = e % kMaxRowWords;
      const int64_t at = base + (int64_t)r * words + c;
      rows[e] = c < words && at < l.mat_words ? l.mat[at] : 0;
    }
    __syncthreads();
    for (int32_t r = threadIdx.x; r < v; r += kThreads) {
      int32_t nc = 0;
      for (int c = 0; c < kMaxRowWords; c++) nc += __popcll(rows[r * kMaxRowWords + c]);
      w.vnchild[l.vlist[l.kvoff[s] + r]] = nc;
      atomicAdd(&s_vedges, nc);
    }
    __syncthreads();  // the popcounts are of the adjacency: no wave starts the closure before every row is counted
    // One barrier after each step, beside the one above.  Within step p threads read words that other threads
    // write in the same step, without atomics: row r's word with bit p, and row p.  What they read cannot
    // change — step p alters neither row p (row p |= row p) nor anybody's bit p (it is set where a row is
    // written at all) — provided an aligned 64-bit LDS access does not tear, which this relies on
    // (ds_read_b64 / ds_write_b64 move the word whole).
    for (int32_t p = 0; p < v; p++) {
      for (int32_t e = threadIdx.x; e < v * kMaxRowWords; e += kThreads) {
        const int32_t r = e / kMaxRowWords, c = e % kMaxRowWords;
        if (c < words && ((rows[r * kMaxRowWords + (p >> 6)] >> (p & 63)) & 1)) rows[e] |= rows[p * kMaxRowWords + c];
      }
      __syncthreads();
    }
    for (int32_t r = threadIdx.x; r < v; r += kThreads)
      if ((rows[r * kMaxRowWords + (r >> 6)] >> (r & 63)) & 1) {  // the version reaches itself
        s_cyclic = 1;
        atomicMin(&s_cyc, enc_value(w, l.vlist[l.kvoff[s] + r]));
      }
    __syncthreads();
    if (threadIdx.x == 0) key_verdict(w, l, s, s_vedges, s_cyclic != 0, s_cyc);
    __syncthreads();  // (before the next key's rows)
  }
}

__global__ __launch_bounds__(kThreads) void lin_readers_kernel(Ws w) {
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    if (!(w.mop_flags[m] & LC_WR_R_EXTERNAL)) continue;
    const int32_t s = w.mop_vslot[m];
    const int64_t at = (int64_t)w.rd_off[s] + atomicAdd(&w.rd_cur[s], 1);
    if (at < w.n_mops) w.readers[at] = w.mop_txn[m];
  }
}

__global__ __launch_bounds__(kThreads) void lin_rc_kernel(Ws w, LinWs l) {
  for (int64_t s = blockIdx.x * (int64_t)kThreads + threadIdx.x; s < (int64_t)w.vcap;
       s += (int64_t)gridDim.x * kThreads) {
    const unsigned long long word = w.vtab[s];
    int64_t v = 0;
    if (word != kEmptyWord) {
      const int32_t ks = w.mop_kslot[(uint32_t)word];
      if (!(w.kflags[ks] & LC_WR_K_CYCLIC) && l.kv[ks] <= kMaxKeyVersions)
        v = ((int64_t)w.vnread[s] + (w.vwriter[s] >= 0)) * w.vnchild[s];
    }
    w.rc[s] = v;
  }
}

// The j-th set bit of a row of `words` words (j below its popcount), or -1.
__device__ __forceinline__ int32_t nth_bit(const unsigned long long *__restrict__ row, int32_t words, int32_t j) {
  for (int32_t c = 0; c < words; c++) {
    unsigned long long x = row[c];
    const int32_t pc = __popcll(x);
    if (j >= pc) {
      j -= pc;
      continue;
    }
    for (; j > 0; j--) x &= x - 1;
    return c * 64 + __ffsll((long long)x) - 1;
  }
  return -1;
}

__global__ __launch_bounds__(kThreads) void lin_item_kernel(Ws w, LinWs l, int64_t n_items) {
  const int64_t n_chunks = (n_items + kItemChunk - 1) / kItemChunk;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t i0 = c * kItemChunk;
    const int64_t i1 = i0 + kItemChunk < n_items ? i0 + kItemChunk : n_items;
    const int64_t s_lo = owner_of(w.item_off, 0, (int64_t)w.vcap - 1, i0);
    const int64_t s_hi = owner_of(w.item_off, s_lo, (int64_t)w.vcap - 1, i1 - 1);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
      const int64_t s = owner_of(w.item_off, s_lo, s_hi, i);
      const int64_t j = i - w.item_off[s], nc = w.vnchild[s], nr = w.vnread[s];
      const int32_t wa = w.vwriter[s];
      if (nc <= 0 || j < 0 || j >= nc * (nr + (wa >= 0))) continue;  // (never: the sums are of these products)
      const int32_t ks = w.mop_kslot[(uint32_t)w.vtab[s]];
      const int64_t v = l.kv[ks];
      const int32_t words = (int32_t)((v + 63) >> 6);
      const int64_t row = l.kmoff[ks] + (int64_t)l.vlocal[s] * words;
      if (v > kMaxKeyVersions || row + words > l.mat_words) continue;  // (never: such a key has no items)
      const int32_t child = nth_bit(l.mat + row, words, (int32_t)(j % nc));
      if (child < 0 || child >= v) continue;
      const int32_t cm = w.vwriter[l.vlist[l.kvoff[ks] + child]];
      if (cm < 0) continue;  // the head has no writer: nil or a phantom
      const int64_t reader = j / nc;
      const int32_t t = reader < nr ? w.readers[w.rd_off[s] + reader] : w.mop_txn[wa];
      const int32_t tw = w.mop_txn[cm];
      if (t != tw && w.txns[tw].type != LC_WR_FAIL && w.txns[t].type != LC_WR_FAIL)
        w.slots[w.n_mops + i] = lc_wr_edge{t, tw, reader < nr ? LC_AP_RW : LC_AP_WW, 0, w.mops[cm].key};
    }
  }
}

__global__ __launch_bounds__(kThreads) void lin_keys_kernel(Ws w, LinWs l, const int32_t *__restrict__ kslots,
                                                            const int64_t *__restrict__ n_keys) {
  const int64_t n = *n_keys < w.n_mops ? *n_keys : w.n_mops;
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t s = kslots[i];
    int64_t t0 = l.ktoff[s], t1 = t0 + l.kntouch[s];
    t0 = t0 < w.n_mops ? t0 : w.n_mops;
    t1 = t1 < w.n_mops ? t1 : w.n_mops;
    l.lin_keys[i] = lc_wr_lin_key{l.pair_off[t1] - l.pair_off[t0], l.kntouch[s], l.knvedges[s]};
  }
}

}  // namespace

size_t lin_temp_bytes(int64_t n_mops, uint64_t vcap, uint64_t kcap) {
  size_t a = 0, b = 0, c = 0, d = 0;
  unsigned long long *k = nullptr;
  int32_t *p = nullptr;
  int64_t *q = nullptr;
  const size_t n = (size_t)(n_mops > 0 ? n_mops : 1);
  (void)rocprim::radix_sort_pairs(nullptr, a, k, k, p, p, n);
  (void)rocprim::inclusive_scan_by_key(nullptr, b, p, p, p, n, MinOp());
  (void)rocprim::exclusive_scan(nullptr, c, q, q, int64_t(0), std::max<size_t>(n, (size_t)kcap) + 1,
                                rocprim::plus<int64_t>());
  (void)rocprim::exclusive_scan(nullptr, d, p, p, int32_t(0), (size_t)kcap + 1, rocprim::plus<int32_t>());
  return std::max(std::max(a, b), std::max(std::max(c, d), scan_temp_bytes(vcap, kcap)));
}

hipError_t launch_lin_rules(const Ws &w, const LinWs &l, int32_t *kslots, int64_t *d_n_keys, void *temp,
                            size_t temp_bytes, hipEvent_t ev0, hipEvent_t ev1, hipStream_t st) {
  const int g_mops = grid_for(w.n_mops, kThreads), g_vers = grid_for((int64_t)w.vcap, kThreads);
  const int g_keys = grid_for((int64_t)w.kcap, kThreads);
  const size_t nm = (size_t)w.n_mops, kc = (size_t)w.kcap;
  hipError_t e = launch_tables(w, st);
  if (e != hipSuccess) return e;
  e = hipEventRecord(ev0, st);
  if (e != hipSuccess) return e;
  size_t bytes;
#define LIN_SCAN(in, out, zero, n, T)                                                                   \
  bytes = temp_bytes;                                                                                   \
  e = rocprim::exclusive_scan(temp, bytes, in, out, zero, n, rocprim::plus<T>(), st);                   \
  if (e != hipSuccess) return e
  // the versions' local indices and the matrices' places
  lin_vlocal_kernel<<<g_vers, kThreads, 0, st>>>(w, l);
  lin_kshape_kernel<<<g_keys, kThreads, 0, st>>>(w, l);
  LIN_SCAN(l.kv, l.kvoff, int32_t(0), kc + 1, int32_t);
  LIN_SCAN(l.kwords, l.kmoff, int64_t(0), kc + 1, int64_t);
  lin_vlist_kernel<<<g_vers, kThreads, 0, st>>>(w, l);
  // the touches, sorted by (key slot, inv_pos)
  lin_iota_kernel<<<g_mops, kThreads, 0, st>>>(w, l);
  lin_touch_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w, l);
  bytes = temp_bytes;
  e = rocprim::radix_sort_pairs(temp, bytes, l.tkey, l.skey, l.tidx, l.sidx, nm, 0, 64, st);
  if (e != hipSuccess) return e;
  LIN_SCAN(l.kntouch, l.ktoff, int32_t(0), kc + 1, int32_t);
  lin_gather_kernel<<<g_mops, kThreads, 0, st>>>(w, l);
  bytes = temp_bytes;
  e = rocprim::inclusive_scan_by_key(temp, bytes, l.r_ks, l.r_comp, l.r_suf, nm, MinOp(),
                                     rocprim::equal_to<int32_t>(), st);
  if (e != hipSuccess) return e;
  lin_range_kernel<<<g_mops, kThreads, 0, st>>>(w, l);
  LIN_SCAN(l.npairs, l.pair_off, int64_t(0), nm + 1, int64_t);
  // the version graphs and their closure
  lin_edge_kernel<<<g_mops, kThreads, 0, st>>>(w, l);
  lin_pair_kernel<<<g_mops, kThreads, 0, st>>>(w, l);  // (the pairs' number stays on the device)
  e = launch_key_slots(w.ktab, w.kcap, kslots, d_n_keys, temp, temp_bytes, st);
  if (e != hipSuccess) return e;
  lin_close_wave_kernel<<<grid_for(w.n_mops, kWaves), kThreads, 0, st>>>(w, l, kslots, d_n_keys);
  lin_close_block_kernel<<<grid_for(w.n_mops, 1), kThreads, 0, st>>>(w, l, kslots, d_n_keys);
  e = hipEventRecord(ev1, st);
  if (e != hipSuccess) return e;
  // rule 7''s groups and the items' prefix sums
  LIN_SCAN(w.vnread, w.rd_off, int32_t(0), (size_t)w.vcap, int32_t);
  lin_readers_kernel<<<g_mops, kThreads, 0, st>>>(w);
  lin_rc_kernel<<<g_vers, kThreads, 0, st>>>(w, l);
  LIN_SCAN(w.rc, w.item_off, int64_t(0), (size_t)w.vcap + 1, int64_t);  // (rc[vcap] is 0)
#undef LIN_SCAN
  e = launch_key_records(w, kslots, d_n_keys, st);
  if (e != hipSuccess) return e;
  lin_keys_kernel<<<g_mops, kThreads, 0, st>>>(w, l, kslots, d_n_keys);
  return hipGetLastError();
}

hipError_t launch_lin_items(const Ws &w, const LinWs &l, int64_t n_items, hipStream_t st) {
  if (n_items > 0) lin_item_kernel<<<grid_for(n_items, kItemChunk), kThreads, 0, st>>>(w, l, n_items);
  return hipGetLastError();
}

}  // namespace lcwr
