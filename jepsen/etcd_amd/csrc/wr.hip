// wr.hip — the kernels of lc_wr_check (include/lincheck_wr.h): rules 1 to 7
// over flat arrays.  Rule 8, the key table's occupied slots and the edges'
// select / sort / unique are txngraph.hip's launchers, which lc_append_check
// calls too; rule 9 is the host's.
//
// What the design rests on: in the wfr graph of rule 4 every version has at
// most one incoming edge (its value has one writer, and a txn gives one edge
// per key), so the graph is a set of parent pointers and rule 6 is pointer
// jumping, not a graph search.
//
//  wr_mop_kernel (a thread per mop): the mop's key into the key table and its
//    (key, value) into the version table — written and read values alike, nil
//    once it is read — the two table formats of txngraph_dev.h.  A write
//    claims the entry's writer word; a second claim raises status[0].  Also
//    rule 1's "last write".
//  wr_txn_kernel (a thread per txn): rules 2, 3 and 5, the wr slots, the
//    per-version reader counts, each wfr edge as its head's parent pointer, a
//    self-loop marking its key at once.  Counts: per wave, onto counters 128 B
//    apart.
//  wr_jump_kernel, `rounds` times: ptr'[v] = ptr[ptr[v]], from one array into
//    the other.  After k rounds a pointer is the ancestor 2^k edges up, or -1
//    where the chain ends sooner; with 2^rounds above the number of versions
//    every pointer left is on or below a cycle, and the pointers' images are
//    exactly the versions on cycles.
//  wr_mark_kernel (a thread per mop): those keys marked cyclic, cyc_value an
//    atomicMin over the images; and the children counted per version — the
//    wfr edges' heads under their tails, every node txn's write under (key, nil).
//  wr_rc_kernel, then three rocprim scans: the readers' and children's group
//    offsets and the prefix sums of readers x children (0 under a cyclic key).
//  wr_fill_kernel (a thread per mop): the groups filled, the ww slots.
//  wr_item_kernel: one work item per (reader, child) pair, found through the
//    prefix sums as ap_item_kernel finds payload entries; a workgroup steps
//    through chunks of items, no thread loops over a product.
//  wr_keys_kernel: a thread per occupied key slot writes its record.
//
// Every loop is bounded by a txn, mop, version, edge, round or table count; no
// workgroup waits for another; results leave through vector stores.
#include <rocprim/device/device_scan.hpp>

#include <algorithm>

#include "txngraph_dev.h"
#include "wr.h"
#include "wr_lin.h"

namespace lcwr {

namespace {

constexpr unsigned long long kSign = 1ull << 63;  // value ^ this: unsigned order is the int64 order

__global__ __launch_bounds__(kThreads) void wr_mop_kernel(Ws w) {
  unsigned long long *ktab = reinterpret_cast<unsigned long long *>(w.ktab);
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    const lc_wr_mop o = w.mops[m];
    const int32_t ks = key_claim(ktab, w.kcap, o.key);
    w.mop_kslot[m] = ks;
    int32_t vs = -1;
    if (o.f == LC_WR_WRITE || o.known) {
      bool inserted;
      vs = pair_claim(w.vtab, w.vcap, w.mops, m, o.key, o.value, &inserted);
      // a new version; nil is counted by the key record itself
      if (inserted && o.value != kReserved) atomicAdd(&w.kcount[3 * (int64_t)ks + 1], 1);
    }
    w.mop_vslot[m] = vs;
    if (o.f != LC_WR_WRITE || vs < 0) continue;
    atomicAdd(&w.kcount[3 * (int64_t)ks], 1);
    const lc_wr_txn x = w.txns[w.mop_txn[m]];
    uint8_t last = 1;
    for (int64_t j = m + 1; j < x.mop_off + x.mop_len; j++)
      if (w.mops[j].f == LC_WR_WRITE && w.mops[j].key == o.key) {
        last = 0;
        break;
      }
    w.mop_last[m] = last;
    if (atomicCAS(&w.vwriter[vs], -1, (int32_t)m) != -1) {  // two writes of one pair
      w.status[1] = (int32_t)m;
      w.status[0] = 1;
    }
  }
}

__global__ __launch_bounds__(kThreads) void wr_txn_kernel(Ws w) {
  long long cnt[kCounters] = {0, 0, 0, 0, 0};
  for (int64_t t = blockIdx.x * (int64_t)kThreads + threadIdx.x; t < w.n_txns; t += (int64_t)gridDim.x * kThreads) {
    const lc_wr_txn x = w.txns[t];
    if (x.type != LC_WR_OK) continue;  // (the flags were zeroed)
    int32_t tf = 0;
    const int64_t end = x.mop_off + x.mop_len;
    for (int64_t m = x.mop_off; m < end; m++) {
      const lc_wr_mop o = w.mops[m];
      const int32_t vs = w.mop_vslot[m], ks = w.mop_kslot[m];
      if (o.f != LC_WR_READ || vs < 0) continue;
      int64_t prev = -1;
      for (int64_t j = m - 1; j >= x.mop_off; j--)
        if (w.mops[j].key == o.key) {
          prev = j;
          break;
        }
      int32_t f = 0;
      if (prev < 0) f |= LC_WR_R_EXTERNAL;
      else if (w.mops[prev].value != o.value) f |= LC_WR_R_INTERNAL;
      int32_t tw = -1;  // the writer's txn where it is another node
      if (o.value != kReserved) {
        const int32_t wm = w.vwriter[vs];
        if (wm < 0) {
          f |= LC_WR_R_PHANTOM;
        } else {
          const int32_t t2 = w.mop_txn[wm];
          const bool failed = w.txns[t2].type == LC_WR_FAIL;
          if (failed) f |= LC_WR_R_G1A;
          if (t2 != t && !w.mop_last[wm]) f |= LC_WR_R_G1B;
          if (t2 != t && !failed) tw = t2;
        }
      }
      for (int b = 0; b < 4; b++) cnt[b] += (f >> b) & 1;
      w.mop_flags[m] = f;
      tf |= f & LC_WR_R_ANOMALY;
      if (prev >= 0) continue;
      atomicAdd(&w.vnread[vs], 1);
      atomicAdd(&w.kcount[3 * (int64_t)ks + 2], 1);
      if (tw >= 0) w.slots[m] = lc_wr_edge{tw, (int32_t)t, LC_AP_WR, 0, o.key};
      int64_t mb = -1;  // the txn's external write of the key
      for (int64_t j = m + 1; j < end; j++)
        if (w.mops[j].f == LC_WR_WRITE && w.mops[j].key == o.key) mb = j;
      if (mb < 0) continue;
      if (atomicAdd(&w.vnrw[vs], 1) == 1) {  // the second such reader: a lost update
        cnt[4]++;
        atomicOr(&w.kflags[ks], LC_WR_K_LOST_UPDATE);
      }
      if (!(w.flags & LC_WR_WFR_KEYS)) continue;
      const int32_t bs = w.mop_vslot[mb];
      if (bs == vs) {  // a self-loop
        atomicOr(&w.kflags[ks], LC_WR_K_CYCLIC);
        atomicMin(&w.kcyc[ks], (unsigned long long)o.value ^ kSign);
      } else if (o.value != kReserved && bs >= 0) {  // (nil -> b is an initial edge anyway, and nil is a root)
        w.mop_par[mb] = vs;
        w.ptr_a[bs] = vs;
      }
    }
    w.txn_flags[t] = tf;
  }
  flush_counters(cnt, w.counters);
}

__global__ __launch_bounds__(kThreads) void wr_jump_kernel(Ws w, const int32_t *__restrict__ in,
                                                           int32_t *__restrict__ out) {
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    if (w.mop_par[m] < 0) continue;  // (only a wfr edge's head has a pointer; every other slot stays -1 in both)
    const int32_t s = w.mop_vslot[m];
    const int32_t p = in[s];
    out[s] = p < 0 ? -1 : in[p];
  }
}

__global__ __launch_bounds__(kThreads) void wr_mark_kernel(Ws w, const int32_t *__restrict__ fin) {
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    const lc_wr_mop o = w.mops[m];
    if (o.f != LC_WR_WRITE) continue;
    const int32_t par = w.mop_par[m];
    if (par >= 0) {
      atomicAdd(&w.vnchild[par], 1);
      const int32_t p = fin[w.mop_vslot[m]];
      if (p >= 0) {  // on or below a cycle; p itself is on it
        const int32_t ks = w.mop_kslot[m];
        atomicOr(&w.kflags[ks], LC_WR_K_CYCLIC);
        atomicMin(&w.kcyc[ks], (unsigned long long)w.mops[(uint32_t)w.vtab[p]].value ^ kSign);
      }
    }
    if (w.txns[w.mop_txn[m]].type == LC_WR_FAIL) continue;
    const int32_t ns = pair_find(w.vtab, w.vcap, w.mops, o.key, kReserved);
    w.mop_nil[m] = ns;
    if (ns >= 0) atomicAdd(&w.vnchild[ns], 1);
  }
}

__global__ __launch_bounds__(kThreads) void wr_rc_kernel(Ws w, int64_t *__restrict__ rc) {
  for (int64_t s = blockIdx.x * (int64_t)kThreads + threadIdx.x; s < (int64_t)w.vcap;
       s += (int64_t)gridDim.x * kThreads) {
    const unsigned long long word = w.vtab[s];
    int64_t v = 0;
    if (word != kEmptyWord && !(w.kflags[w.mop_kslot[(uint32_t)word]] & LC_WR_K_CYCLIC))
      v = (int64_t)w.vnread[s] * w.vnchild[s];
    rc[s] = v;
  }
}

__global__ __launch_bounds__(kThreads) void wr_fill_kernel(Ws w) {
  for (int64_t m = blockIdx.x * (int64_t)kThreads + threadIdx.x; m < w.n_mops; m += (int64_t)gridDim.x * kThreads) {
    const lc_wr_mop o = w.mops[m];
    const int32_t t = w.mop_txn[m];
    if (o.f == LC_WR_READ) {
      if (!(w.mop_flags[m] & LC_WR_R_EXTERNAL)) continue;
      const int32_t s = w.mop_vslot[m];
      const int64_t at = (int64_t)w.rd_off[s] + atomicAdd(&w.rd_cur[s], 1);
      if (at < w.n_mops) w.readers[at] = t;
      continue;
    }
    const int32_t ns = w.mop_nil[m], par = w.mop_par[m];
    if (ns >= 0) {
      const int64_t at = (int64_t)w.ch_off[ns] + atomicAdd(&w.ch_cur[ns], 1);
      if (at < 2 * w.n_mops) w.children[at] = (int32_t)m;
    }
    if (par < 0) continue;
    const int64_t at = (int64_t)w.ch_off[par] + atomicAdd(&w.ch_cur[par], 1);
    if (at < 2 * w.n_mops) w.children[at] = (int32_t)m;
    if (w.kflags[w.mop_kslot[m]] & LC_WR_K_CYCLIC) continue;
    const int32_t wa = w.vwriter[par];
    if (wa < 0) continue;
    const int32_t ta = w.mop_txn[wa];  // (t itself is an OK txn: it has a wfr edge)
    if (ta != t && w.txns[ta].type != LC_WR_FAIL) w.slots[m] = lc_wr_edge{ta, t, LC_AP_WW, 0, o.key};
  }
}

// The largest s in [lo, hi] with off[s] <= i (off[lo] <= i holds): the one
// version whose items hold i, as versions without items share their
// successor's offset.
__device__ __forceinline__ int64_t slot_of(const int64_t *__restrict__ off, int64_t lo, int64_t hi, int64_t i) {
  while (lo < hi) {
    const int64_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(kThreads) void wr_item_kernel(Ws w, int64_t n_items) {
  const int64_t n_chunks = (n_items + kItemChunk - 1) / kItemChunk;
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t i0 = c * kItemChunk;
    const int64_t i1 = i0 + kItemChunk < n_items ? i0 + kItemChunk : n_items;
    const int64_t s_lo = slot_of(w.item_off, 0, (int64_t)w.vcap - 1, i0);
    const int64_t s_hi = slot_of(w.item_off, s_lo, (int64_t)w.vcap - 1, i1 - 1);
    for (int64_t i = i0 + threadIdx.x; i < i1; i += kThreads) {
      const int64_t s = slot_of(w.item_off, s_lo, s_hi, i);
      const int64_t j = i - w.item_off[s], nc = w.vnchild[s];
      if (nc <= 0 || j < 0 || j >= nc * w.vnread[s]) continue;  // (never: the sums are of these products)
      const int32_t t = w.readers[w.rd_off[s] + j / nc];
      const int32_t cm = w.children[w.ch_off[s] + j % nc];
      const int32_t tw = w.mop_txn[cm];
      if (t != tw && w.txns[tw].type != LC_WR_FAIL)
        w.slots[w.n_mops + i] = lc_wr_edge{t, tw, LC_AP_RW, 0, w.mops[cm].key};
    }
  }
}

__global__ __launch_bounds__(kThreads) void wr_keys_kernel(Ws w, const int32_t *__restrict__ kslots,
                                                           const int64_t *__restrict__ n_keys) {
  const int64_t n = *n_keys < w.n_mops ? *n_keys : w.n_mops;  // (keys has room for n_mops records)
  for (int64_t i = blockIdx.x * (int64_t)kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
    const int64_t s = kslots[i];
    lc_wr_key k;
    k.key = w.ktab[s] ^ kKeyXor;
    k.flags = w.kflags[s];
    k.cyc_value = (k.flags & LC_WR_K_CYCLIC) ? (int64_t)(w.kcyc[s] ^ kSign) : kReserved;
    k.n_writes = w.kcount[3 * s];
    k.n_versions = w.kcount[3 * s + 1] + 1;
    k.n_ext_reads = w.kcount[3 * s + 2];
    w.keys[i] = k;
  }
}

}  // namespace

size_t scan_temp_bytes(uint64_t vcap, uint64_t kcap) {
  size_t a = 0, b = 0;
  int32_t *p = nullptr;
  int64_t *q = nullptr;
  (void)rocprim::exclusive_scan(nullptr, a, p, p, int32_t(0), (size_t)vcap, rocprim::plus<int32_t>());
  (void)rocprim::exclusive_scan(nullptr, b, q, q, int64_t(0), (size_t)vcap + 1, rocprim::plus<int64_t>());
  return std::max(a, std::max(b, key_temp_bytes(kcap)));
}

hipError_t launch_rules(const Ws &w, int rounds, int32_t *kslots, int64_t *d_n_keys, void *temp, size_t temp_bytes,
                        hipStream_t st) {
  const int g_mops = grid_for(w.n_mops, kThreads);
  wr_mop_kernel<<<g_mops, kThreads, 0, st>>>(w);
  wr_txn_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w);
  const int32_t *fin = w.ptr_a;
  if (w.flags & LC_WR_WFR_KEYS)
    for (int r = 0; r < rounds; r++) {
      int32_t *to = (r & 1) ? w.ptr_a : w.ptr_b;
      wr_jump_kernel<<<g_mops, kThreads, 0, st>>>(w, fin, to);
      fin = to;
    }
  wr_mark_kernel<<<g_mops, kThreads, 0, st>>>(w, fin);
  wr_rc_kernel<<<grid_for((int64_t)w.vcap, kThreads), kThreads, 0, st>>>(w, w.rc);
  size_t bytes = temp_bytes;
  hipError_t e = rocprim::exclusive_scan(temp, bytes, w.vnread, w.rd_off, int32_t(0), (size_t)w.vcap,
                                         rocprim::plus<int32_t>(), st);
  if (e != hipSuccess) return e;
  bytes = temp_bytes;
  e = rocprim::exclusive_scan(temp, bytes, w.vnchild, w.ch_off, int32_t(0), (size_t)w.vcap, rocprim::plus<int32_t>(),
                              st);
  if (e != hipSuccess) return e;
  bytes = temp_bytes;  // (rc[vcap] is 0: item_off[vcap] is the total)
  e = rocprim::exclusive_scan(temp, bytes, w.rc, w.item_off, int64_t(0), (size_t)w.vcap + 1, rocprim::plus<int64_t>(),
                              st);
  if (e != hipSuccess) return e;
  wr_fill_kernel<<<g_mops, kThreads, 0, st>>>(w);
  e = launch_key_slots(w.ktab, w.kcap, kslots, d_n_keys, temp, temp_bytes, st);
  if (e != hipSuccess) return e;
  wr_keys_kernel<<<g_mops, kThreads, 0, st>>>(w, kslots, d_n_keys);
  return hipGetLastError();
}

// lc_wr_check_lin (wr_lin.hip) runs the tables' and the records' kernels alone.
hipError_t launch_tables(const Ws &w, hipStream_t st) {
  wr_mop_kernel<<<grid_for(w.n_mops, kThreads), kThreads, 0, st>>>(w);
  wr_txn_kernel<<<grid_for(w.n_txns, kThreads), kThreads, 0, st>>>(w);
  return hipGetLastError();
}

hipError_t launch_key_records(const Ws &w, const int32_t *kslots, const int64_t *d_n_keys, hipStream_t st) {
  wr_keys_kernel<<<grid_for(w.n_mops, kThreads), kThreads, 0, st>>>(w, kslots, d_n_keys);
  return hipGetLastError();
}

hipError_t launch_items(const Ws &w, int64_t n_items, hipStream_t st) {
  if (n_items > 0) wr_item_kernel<<<grid_for(n_items, kItemChunk), kThreads, 0, st>>>(w, n_items);
  return hipGetLastError();
}

}  // namespace lcwr
