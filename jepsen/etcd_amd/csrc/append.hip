// append.hip — the kernels of lc_append_check (include/lincheck_append.h):
// rules 1 to 6 over flat arrays.  Rule 7 is the host's (append_host.cpp).
//
//  ap_mop_kernel (one thread per mop): the mop's key into the key table; an
//    append into the writer table, a pair table over (key, element); a second
//    insertion of one pair raises status[0].  Also rule 1's "last append".
//  ap_best_kernel (one thread per real read): one 64-bit atomicMax of
//    (len, ~read) on its key's slot.
//  ap_item_kernel (the bandwidth pass; one work item per (read, payload
//    entry), found through the prefix sums of the lengths).  An item of its
//    key's longest read does the order pass's work: it probes the entry's
//    writer, writes it to ord_w, stamps its index into the table entry with
//    atomicMin (a second stamp is a duplicate) and lowers first_failed /
//    first_phantom.  Every other item compares its entry with the order's at
//    the same index: two streaming loads; a mismatch marks the read and the
//    key.  The first_* atomics fire on anomalies only, so they are not
//    reduced across the wave first.
//  ap_txn_kernel (one thread per txn): rules 3 and 4 of its reads from
//    first_* and the order in O(own mops); G1b from ord_w; the wr / rw slots.
//    A txn with a non-prefix read, or a read of a key whose order has two
//    phantoms, is left to the host (kTxnSlow).  Counts: per wave, onto
//    counters 128 B apart.
//  ap_item_kernel<1> (the same enumeration, once the keys' flags are final):
//    the ww slots, one per order position.
//  ap_keys_kernel: a thread per occupied slot of the key table, which
//    txngraph.hip's launch_key_slots lists, writes its record.
//  The edges' select, sort and unique and real time (rule 6) are
//  txngraph.hip's, the two table formats txngraph_dev.h's.
//
// Every loop is bounded by a txn, mop, read, payload or table count; no
// workgroup waits for another; results leave through vector stores.
#include "append.h"
#include "txngraph_dev.h"

namespace lcap {

namespace {

constexpr uint32_t kNoIndex = 0xFFFFFFFFu;  // first_* and stamps on the device: unsigned, so -1 once cast

__global__ __launch_bounds__(kThreads) void ap_mop_kernel(Ws w) {
  unsigned long long *ktab = reinterpret_cast<unsigned long long *>(w.ktab);
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    const lc_ap_mop o = w.mops[m];
    w.mop_kslot[m] = key_claim(ktab, w.kcap, o.key);
    if (o.f != LC_AP_APPEND) continue;
    const lc_ap_txn x = w.txns[w.mop_txn[m]];
    uint8_t last = 1;
    for (int64_t j = m + 1; j < x.mop_off + x.mop_len; j++)
      if (w.mops[j].f == LC_AP_APPEND && w.mops[j].key == o.key) {
        last = 0;
        break;
      }
    w.mop_last[m] = last;
    bool inserted;  // found, not inserted: two appends of one pair
    if (pair_claim(w.wtab, w.wcap, w.mops, m, o.key, o.value, &inserted) >= 0 && !inserted) {
      w.status[1] = (int32_t)m;
      w.status[0] = 1;
    }
  }
}

__global__ __launch_bounds__(kThreads) void ap_best_kernel(Ws w) {
  for (int64_t r = blockIdx.x * (int64_t)kThreads + threadIdx.x; r < w.n_real; r += (int64_t)gridDim.x * kThreads) {
    const int32_t m = w.rd_mop[r];
    atomicMax(&w.kbest[w.mop_kslot[m]], (unsigned long long)pack_best(w.mops[m].len, (int32_t)r));
  }
}

// The largest r in [lo, hi] with work_off[r] <= i (work_off[lo] <= i holds).
__device__ __forceinline__ int64_t read_of(const int64_t *__restrict__ work_off, int64_t lo, int64_t hi, int64_t i) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (work_off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ bool key_has_order(const Ws &w, int32_t ks) {
  const uint32_t *kf = reinterpret_cast<const uint32_t *>(w.kfirst) + 3 * (int64_t)ks;
  return !(w.kflags[ks] & LC_AP_K_INCOMPATIBLE) && kf[0] == kNoIndex && kf[2] == kNoIndex;
}

// kind 0: the item pass; kind 1: the ww slots.
template <int kKind>
__global__ __launch_bounds__(kThreads) void ap_item_kernel(Ws w) {
  uint32_t *stamp = reinterpret_cast<uint32_t *>(w.stamp);
  uint32_t *kfirst = reinterpret_cast<uint32_t *>(w.kfirst);
  const int64_t n_chunks = (w.n_work + kItemChunk - 1) / kItemChunk;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t i0 = c * kItemChunk;
    const int64_t i1 = i0 + kItemChunk < w.n_work ? i0 + kItemChunk : w.n_work;
    // the chunk's reads: every item's search stays inside [r_lo, r_hi]
    const int64_t r_lo = read_of(w.work_off, 0, w.n_real - 1, i0);
    const int64_t r_hi = read_of(w.work_off, r_lo, w.n_real - 1, i1 - 1);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
      const int64_t r = read_of(w.work_off, r_lo, r_hi, i);
      const int32_t j = (int32_t)(i - w.work_off[r]);
      const lc_ap_mop o = w.mops[w.rd_mop[r]];
      const int32_t ks = w.mop_kslot[w.rd_mop[r]];
      const unsigned long long best = w.kbest[ks];
      const int32_t rl = best_read(best);
      if (kKind == 1) {
        if (rl != r || j + 1 >= o.len || !key_has_order(w, ks)) continue;
        const int32_t ta = w.mop_txn[w.ord_w[i]], tb = w.mop_txn[w.ord_w[i + 1]];
        if (ta != tb && w.txns[ta].type != LC_AP_FAIL && w.txns[tb].type != LC_AP_FAIL)
          w.slots[2 * w.n_real + i] = lc_ap_edge{ta, tb, LC_AP_WW, 0, o.key};
        continue;
      }
      const int64_t v = w.values[o.value + j];
      if (rl != r) {  // against the order's entry at the same index
        if (v != w.values[w.mops[w.rd_mop[rl]].value + j]) {
          w.nonprefix[r] = 1;
          atomicOr(&w.kflags[ks], LC_AP_K_INCOMPATIBLE);
        }
        continue;
      }
      int32_t wm = -1;  // the entry's writer: its slot and its mop
      const int32_t s = pair_find(w.wtab, w.wcap, w.mops, o.key, v, &wm);
      w.ord_w[i] = wm;
      if (wm < 0) {
        if (atomicMin(&kfirst[3 * (int64_t)ks + 2], (uint32_t)j) != kNoIndex) atomicOr(&w.kflags[ks], kKeyTwoPhantoms);
        continue;
      }
      const uint32_t old = atomicMin(&stamp[s], (uint32_t)j);
      if (old != kNoIndex)  // the entry was named before: the later of the two indices repeats it
        atomicMin(&kfirst[3 * (int64_t)ks], old > (uint32_t)j ? old : (uint32_t)j);
      if (w.txns[w.mop_txn[wm]].type == LC_AP_FAIL) atomicMin(&kfirst[3 * (int64_t)ks + 1], (uint32_t)j);
    }
  }
}

__global__ __launch_bounds__(kThreads) void ap_txn_kernel(Ws w) {
  const int32_t *kfirst = w.kfirst;
  long long cnt[kCounters] = {0, 0, 0, 0, 0, 0};
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < w.n_txns; t += (int64_t)gridDim.x * kThreads) {
    const lc_ap_txn x = w.txns[t];
    if (x.type != LC_AP_OK) {
      w.txn_flags[t] = 0;
      continue;
    }
    const int32_t r0 = w.txn_r0[t], r1 = w.txn_r0[t + 1];
    bool slow = false;
    for (int32_t r = r0; r < r1; r++)
      slow = slow || w.nonprefix[r] || (w.kflags[w.mop_kslot[w.rd_mop[r]]] & kKeyTwoPhantoms);
    int32_t tf = 0;
    for (int32_t r = r0; r < r1; r++) {
      const int64_t m = w.rd_mop[r];
      const lc_ap_mop o = w.mops[m];
      const int32_t ks = w.mop_kslot[m];
      const int32_t fd = kfirst[3 * (int64_t)ks], ff = kfirst[3 * (int64_t)ks + 1], fp = kfirst[3 * (int64_t)ks + 2];
      const unsigned long long best = w.kbest[ks];
      const int64_t base = w.work_off[best_read(best)];
      int32_t f = w.nonprefix[r] ? LC_AP_R_NONPREFIX : 0;
      // the txn's earlier mops on this key: back to its latest read of it
      int64_t p = -1, a = 0;
      for (int64_t j = m - 1; j >= x.mop_off; j--)
        if (w.mops[j].key == o.key) {
          if (w.mops[j].f == LC_AP_READ) {
            p = j;
            break;
          }
          a++;
        }
      const bool external = p < 0 && a == 0;
      if (external) f |= LC_AP_R_EXTERNAL;
      if (!slow) {
        if (fd >= 0 && o.len > fd) f |= LC_AP_R_DUPLICATE;
        if (ff >= 0 && o.len > ff) f |= LC_AP_R_G1A;
        if (fp >= 0 && o.len > fp) f |= LC_AP_R_PHANTOM;
        if (o.len > 0) {
          const int32_t wm = w.ord_w[base + o.len - 1];
          if (wm >= 0 && w.mop_txn[wm] != t && !w.mop_last[wm]) f |= LC_AP_R_G1B;
        }
        if (!external) {
          // every read here is a prefix of one order: it equals the earlier
          // read's entries iff it is long enough; only the tail is compared
          const int64_t at = p >= 0 ? w.mops[p].len : o.len - a;
          bool ok = p >= 0 ? o.len == at + a : o.len >= a;
          int64_t i = 0;
          for (int64_t j = (p >= 0 ? p + 1 : x.mop_off); ok && j < m; j++)
            if (w.mops[j].key == o.key) ok = w.values[o.value + at + i++] == w.mops[j].value;
          if (!ok) f |= LC_AP_R_INTERNAL;
        }
        for (int b = 0; b < 5; b++) cnt[b] += (f >> (b + 1)) & 1;
      } else {
        cnt[5]++;
      }
      if (external && !(f & LC_AP_R_NONPREFIX) && !(w.kflags[ks] & LC_AP_K_INCOMPATIBLE) && fd < 0 && fp < 0) {
        const int32_t n = best_len(best);
        if (o.len > 0) {
          const int32_t tw = w.mop_txn[w.ord_w[base + o.len - 1]];
          if (tw != t && w.txns[tw].type != LC_AP_FAIL)
            w.slots[2 * (int64_t)r] = lc_ap_edge{tw, (int32_t)t, LC_AP_WR, 0, o.key};
        }
        if (o.len < n) {
          const int32_t tw = w.mop_txn[w.ord_w[base + o.len]];
          if (tw != t && w.txns[tw].type != LC_AP_FAIL)
            w.slots[2 * (int64_t)r + 1] = lc_ap_edge{(int32_t)t, tw, LC_AP_RW, 0, o.key};
        }
      }
      w.mop_flags[m] = f;
      tf |= f & LC_AP_R_ANOMALY;
    }
    w.txn_flags[t] = tf | (slow ? kTxnSlow : 0);
  }
  flush_counters(cnt, w.counters);
}

__global__ __launch_bounds__(kThreads) void ap_keys_kernel(Ws w, const int32_t *__restrict__ kslots,
                                                           const int64_t *__restrict__ n_keys) {
  const int64_t n = *n_keys < w.n_mops ? *n_keys : w.n_mops;  // (keys has room for n_mops records)
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t s = kslots[i];
    const unsigned long long best = w.kbest[s];
    const int32_t *kf = w.kfirst + 3 * s;
    lc_ap_key k;
    k.key = w.ktab[s] ^ kKeyXor;
    k.longest = best ? w.rd_mop[best_read(best)] : -1;
    k.len = best ? best_len(best) : 0;
    k.flags = w.kflags[s];
    if ((k.flags & LC_AP_K_INCOMPATIBLE) || kf[0] >= 0 || kf[2] >= 0) k.flags |= LC_AP_K_NO_ORDER;
    k.first_dup = kf[0];
    k.first_failed = kf[1];
    k.first_phantom = kf[2];
    k.pad = 0;
    w.keys[i] = k;
  }
}

}  // namespace

hipError_t launch_rules(const Ws &w, int32_t *kslots, int64_t *d_n_keys, void *temp, size_t temp_bytes,
                        hipStream_t st) {
  ap_mop_kernel<<<grid_for(w.n_mops, kThreads), kThreads, 0, st>>>(w);
  if (w.n_real > 0) ap_best_kernel<<<grid_for(w.n_real, kThreads), kThreads, 0, st>>>(w);
  if (w.n_work > 0) ap_item_kernel<0><<<grid_for(w.n_work, kItemChunk), kThreads, 0, st>>>(w);
  ap_txn_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w);
  if (w.n_work > 0) ap_item_kernel<1><<<grid_for(w.n_work, kItemChunk), kThreads, 0, st>>>(w);
  // the occupied slots of the key table, in slot order; at most n_mops of them
  hipError_t e = launch_key_slots(w.ktab, w.kcap, kslots, d_n_keys, temp, temp_bytes, st);
  if (e != hipSuccess) return e;
  ap_keys_kernel<<<grid_for(w.n_mops, kThreads), kThreads, 0, st>>>(w, kslots, d_n_keys);
  return hipGetLastError();
}

}  // namespace lcap
