// witness_search.hip — LC_FLAG_SEARCH_WITNESS: linearization witnesses for
// the keys a search tier decided (include/lincheck.h, LC_WITNESS_ORDER_FULL /
// LC_WITNESS_ORDER_PREFIX).
//
// The frontier searches of check_kernel.hip hold sets of (mask, state)
// configurations without parent links, so they cannot name an order.  This
// stage runs behind them, over the keys that are decided but carry no
// witness, as the other knossos analyzer does (knossos.wgl, Wing-Gong-Lowe):
// a depth-first search whose stack IS the linearization, with a cache of the
// configurations found to be dead ends.  One wavefront per key; no wave ever
// waits for another.
//
// Per key:
//   1. Event pass.  Calls and returns are walked in history order (returns
//      before calls at equal indices: an op ranked before b must have been
//      called strictly before b returned).  Every record gets a window slot
//      at its call (the lowest free one); an :ok op frees it at its return, a
//      crashed op keeps it.  So the slot of a record, and the window at an
//      event, depend on the history alone, not on the search path.  The pass
//      writes slot[r] per record and, per return k (in order), the returning
//      record, its slot, and the number of records called before it.  A 65th
//      open op ends the key (n_window).  An invalid key's events stop at
//      cut = fail_prefix_end - 1.
//   2. Search.  A node is (k, mask, state): the next return to serve, the
//      open ops already linearized (by slot), the register.  If return k's
//      op x is linearized, its slot is freed and the calls up to return k + 1
//      enter theirs.  Otherwise one open, unlinearized op whose precondition
//      holds (one ballot over the window, a slot per lane) is linearized: a
//      frame (record, k, untried candidates, mask and state before) is pushed
//      and the state stepped.  A legal read goes first and is forced (it does
//      not change the state, so taking it now loses nothing); else x itself,
//      else the earliest deadline.  A node without candidates, or found in the
//      cache, is a dead end: the top frame's next candidate is tried, from
//      the frame's position — the window is rebuilt from the event pass's
//      arrays: the records called since leave, the ops returned since come
//      back — and a frame without candidates left puts its node in the cache.
//   3. On success frame j's record has rank j.
// The order is checked against the definition by the caller (witness.py,
// tests/order_ref.py), so a fault of the search shows as a missing witness,
// never as a wrong one.
//
// A key this stage leaves at a 65th open op is listed for the counted stage
// (LC_FLAG_COUNTED_WITNESS, at the end of this file), which counts crashed
// writes/CAS per class instead of giving each a slot.
#include <hip/hip_runtime.h>

#include "counted.h"
#include "kernels.h"
#include "records.h"
#include "wave.h"

namespace lcdev {
namespace {

// One linearization step.  `rem`: the node's candidates not yet tried;
// (mask, ver, val): the node itself.
struct WsFrame {
  int32_t rec, k;
  uint64_t rem, mask;
  int32_t ver, val;
};
static_assert(sizeof(WsFrame) == 32, "WsFrame");

// Return k of the event pass: the record, its slot, the records called
// before it.
struct WsEvent {
  int32_t rec, ncalls, slot, pad;
};

// Dead-end cache: open addressing over 128-byte buckets of five nodes, the
// whole (k, mask, state) stored — a hit is exact.  An entry is live when its
// gen is the current key's (the workspace is zeroed once per launch, keys
// count from 1).  A node goes into the first bucket of its probe sequence
// with a free entry, and nothing is ever removed, so a lookup stops at the
// first bucket with a free entry.  When kWitnessProbes buckets are full the
// node is not stored.
struct alignas(128) WsBucket {
  uint64_t mask[5];
  uint32_t gen[5];
  int32_t k[5], ver[5], val[5];
  uint32_t pad[2];
};
static_assert(sizeof(WsBucket) == 128, "WsBucket");
constexpr int kWitnessProbes = 8;

enum { kWsFound = 0, kWsBudget = 1, kWsWindow = 2 };

__device__ __forceinline__ uint64_t uni64(uint64_t v) {
  const uint32_t lo = (uint32_t)uni((int)(uint32_t)v), hi = (uint32_t)uni((int)(uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ bool ws_pre_ok(int nv, int nvm, int nl, int nlm, int ver, int val) {
  return (((ver ^ nv) & nvm) | ((val ^ nl) & nlm)) == 0;
}

// The window: per slot the record it holds (-1: free), its precondition, kind,
// the value it writes and its return.  In LDS so that a lane can fill
// another lane's slot; each lane keeps a copy of its own slot in registers.
struct WsWindow {
  int rec[kWave], nv[kWave], nvm[kWave], nl[kWave], nlm[kWave], f[kWave], val[kWave];
  uint32_t ret[kWave];
};
struct WsLane {
  int rec, nv, nvm, nl, nlm, f, val;
  uint32_t ret;
};

struct WsKey {
  const lc_op *kops;
  int n;
  int64_t base_idx;
  uint8_t *slots;
  WsEvent *ev;
  WsFrame *fr;
  WsBucket *cache;
  uint32_t bmask;  // buckets - 1
  uint32_t gen;
};

__device__ __forceinline__ void ws_refresh(const WsWindow &w, WsLane &l, int lane) {
  __syncthreads();
  l.rec = w.rec[lane];
  l.nv = w.nv[lane];
  l.nvm = w.nvm[lane];
  l.nl = w.nl[lane];
  l.nlm = w.nlm[lane];
  l.f = w.f[lane];
  l.val = w.val[lane];
  l.ret = w.ret[lane];
}

// Record r into slot s (one lane per record).
__device__ __forceinline__ void ws_put(WsWindow &w, const WsKey &key, int r, int s) {
  const Rec d = decode(load_raw(key.kops, r, key.n), key.base_idx);
  w.rec[s] = r;
  w.nv[s] = d.nv;
  w.nvm[s] = d.nvm;
  w.nl[s] = d.nl;
  w.nlm[s] = d.nlm;
  w.f[s] = d.f;
  w.val[s] = d.val;
  w.ret[s] = d.ret;
}

// Records [r0, r1) enter their slots (all open at once: distinct slots).
__device__ __forceinline__ void ws_admit(WsWindow &w, const WsKey &key, int r0, int r1, int lane) {
  for (int b = r0; b < r1; b += kWave) {
    const int r = b + lane;
    if (r < r1) ws_put(w, key, r, key.slots[r]);
  }
}

// The window of return k_from becomes the window of the earlier return k_to.
__device__ __forceinline__ void ws_rewind(WsWindow &w, const WsKey &key, int k_from, int k_to,
                                          int lane) {
  const int c_to = uni(key.ev[k_to].ncalls), c_from = uni(key.ev[k_from].ncalls);
  for (int b = c_to; b < c_from; b += kWave) {  // called since: out
    const int r = b + lane;
    if (r < c_from) w.rec[key.slots[r]] = -1;
  }
  __syncthreads();
  for (int b = k_to; b < k_from; b += kWave) {  // returned since, called before: back in
    const int j = b + lane;
    if (j < k_from) {
      const WsEvent e = key.ev[j];
      if (e.rec < c_to) ws_put(w, key, e.rec, e.slot);
    }
  }
}

__device__ __forceinline__ uint32_t ws_hash(int k, uint64_t mask, int ver, int val) {
  uint64_t h = mask * 0x9E3779B97F4A7C15ull;
  h ^= ((uint64_t)(uint32_t)k << 32 | (uint32_t)ver) * 0xC2B2AE3D27D4EB4Full;
  h ^= (uint64_t)(uint32_t)val * 0x165667B19E3779F9ull;
  h ^= h >> 29;
  h *= 0xBF58476D1CE4E5B9ull;
  return (uint32_t)(h >> 32);
}

// Is the node in the cache?  With `insert`, store it when it is not (and
// there is room).  Wave-uniform.
__device__ __forceinline__ bool ws_cache(const WsKey &key, int k, uint64_t mask, int ver, int val,
                                         bool insert, int lane) {
  const uint32_t b0 = ws_hash(k, mask, ver, val);
  for (int probe = 0; probe < kWitnessProbes; probe++) {
    WsBucket *B = key.cache + ((b0 + (uint32_t)probe) & key.bmask);
    bool hit = false, free_ = false;
    if (lane < 5) {
      if (B->gen[lane] == key.gen)
        hit = B->k[lane] == k && B->mask[lane] == mask && B->ver[lane] == ver && B->val[lane] == val;
      else
        free_ = true;
    }
    if (__ballot(hit)) return true;
    const uint64_t fm = __ballot(free_);
    if (fm) {
      if (insert && lane == first_lane(fm)) {
        B->mask[lane] = mask;
        B->k[lane] = k;
        B->ver[lane] = ver;
        B->val[lane] = val;
        B->gen[lane] = key.gen;
      }
      if (insert) __syncthreads();
      return false;
    }
  }
  return false;
}

// The candidate of `cs` (not empty) to try next: x's slot if it is one, else
// the earliest return (crashed ops last), ties by slot.
__device__ __forceinline__ int ws_pick(uint64_t cs, int sx, const WsLane &l, int lane) {
  if ((cs >> sx) & 1) return sx;
  const bool in = (cs >> lane) & 1;
  const uint32_t m = wave_min_u32(in ? l.ret : kNever);
  return first_lane(__ballot(in && l.ret == m));
}

struct WsCount {
  int64_t nodes, hits;
};

// Search one key; on kWsFound *depth frames hold the order.
__device__ int ws_search(WsWindow &w, const WsKey &key, const KParams &p, uint32_t cut, int *depth_out,
                         WsCount &cnt, int lane) {
  const int n = key.n;
  // ---- 1. event pass
  int K = 0;
  {
    uint64_t occ = 0;
    uint32_t wret = kNever;
    int wrec = -1, myslot = 0, i = 0, base = 0, bad = 0;
    Rec cur = decode(load_raw(key.kops, lane, n), key.base_idx);
    bad |= cur.bad;
    for (;;) {
      if (i < n && i - base >= kWave) {  // next chunk of records
        if (base + lane < n) key.slots[base + lane] = (uint8_t)myslot;
        base += kWave;
        cur = decode(load_raw(key.kops, base + lane, n), key.base_idx);
        bad |= cur.bad;
      }
      const uint32_t ncall = i < n ? (uint32_t)__builtin_amdgcn_readlane((int)cur.call, i - base) : kNever;
      const uint32_t mret = wave_min_u32(wret);
      const uint32_t t = umin(ncall, mret);
      if (t == kNever || t > cut) break;
      if (mret <= ncall) {  // a return
        const int sm = first_lane(__ballot(wret == mret));
        const int x = __builtin_amdgcn_readlane(wrec, sm);
        if (lane == 0) key.ev[K] = WsEvent{x, i, sm, 0};
        K++;
        occ &= ~(1ull << sm);
        if (lane == sm) {
          wret = kNever;
          wrec = -1;
        }
      } else {  // the call of record i
        if (~occ == 0) return kWsWindow;
        const int s = first_lane(~occ);
        occ |= 1ull << s;
        const uint32_t rt = (uint32_t)__builtin_amdgcn_readlane((int)cur.ret, i - base);
        if (lane == s) {
          wret = rt;
          wrec = i;
        }
        if (lane == i - base) myslot = s;
        i++;
      }
    }
    if (base + lane < n) key.slots[base + lane] = (uint8_t)myslot;
    if (__ballot(bad != 0)) return kWsBudget;  // (no tier decides such a key)
  }
  w.rec[lane] = -1;
  __syncthreads();
  *depth_out = 0;
  if (K == 0) return kWsFound;

  // ---- 2. search
  const uint64_t t0 = p.time_ticks ? wall_clock64() : 0;
  // (a step is followed by the returns it unblocks and, after a dead end, by
  // the frames popped: a few iterations each; this bounds the loop outright)
  const int64_t iter_limit = 16 * p.budget + 4 * (int64_t)n + 1024;
  int k = 0, depth = 0, ver = p.init_ver, val = p.init_val, n_ins = 0;
  uint64_t mask = 0;
  int64_t iters = 0;
  WsLane l;
  // return k's event: the records called before it, its op's slot
  int ec = uni(key.ev[0].ncalls), es = uni(key.ev[0].slot);
  ws_admit(w, key, 0, ec, lane);
  ws_refresh(w, l, lane);
  for (;;) {
    if (k == K) break;
    if (++iters > iter_limit || cnt.nodes > p.budget) return kWsBudget;
    if ((iters & 255) == 0 && p.time_ticks && wall_clock64() - t0 > p.time_ticks) return kWsBudget;
    const uint64_t xb = 1ull << es;
    if (mask & xb) {  // x is linearized: its return
      mask &= ~xb;
      if (lane == es) w.rec[es] = -1;
      __syncthreads();
      const int c0 = ec;
      k++;
      if (k < K) {
        ec = uni(key.ev[k].ncalls);
        es = uni(key.ev[k].slot);
        ws_admit(w, key, c0, ec, lane);
      }
      ws_refresh(w, l, lane);
      continue;
    }
    bool dead = false;
    if (n_ins > 0 && ws_cache(key, k, mask, ver, val, false, lane)) {
      dead = true;
      cnt.hits++;
    }
    uint64_t cand = 0;
    if (!dead) {
      cand = __ballot(l.rec >= 0 && ws_pre_ok(l.nv, l.nvm, l.nl, l.nlm, ver, val)) & ~mask;
      if (!cand) {
        ws_cache(key, k, mask, ver, val, true, lane);
        n_ins++;
      }
    }
    int s;
    uint64_t rem;
    if (cand) {
      const uint64_t reads = cand & __ballot(l.f == LC_F_READ);
      if (reads) {
        s = (reads >> es) & 1 ? es : first_lane(reads);
        rem = 0;
      } else {
        s = ws_pick(cand, es, l, lane);
        rem = cand & ~(1ull << s);
      }
      depth++;
    } else {
      // dead end: back to the last frame with a candidate left
      for (;;) {
        if (depth == 0) return kWsBudget;  // no order: the tiers' verdict is not reproduced
        const WsFrame f = key.fr[depth - 1];
        const int fk = uni(f.k);
        if (fk != k) {
          ws_rewind(w, key, k, fk, lane);
          ws_refresh(w, l, lane);
          k = fk;
          ec = uni(key.ev[k].ncalls);
          es = uni(key.ev[k].slot);
        }
        mask = uni64(f.mask);
        ver = uni(f.ver);
        val = uni(f.val);
        rem = uni64(f.rem);
        if (rem) break;
        ws_cache(key, k, mask, ver, val, true, lane);
        n_ins++;
        depth--;
        if (++iters > iter_limit) return kWsBudget;
      }
      s = ws_pick(rem, es, l, lane);
      rem &= ~(1ull << s);
    }
    // linearize the op in slot s: frame depth - 1
    const int rec = __builtin_amdgcn_readlane(l.rec, s);
    if (lane == 0) key.fr[depth - 1] = WsFrame{rec, k, rem, mask, ver, val};
    __syncthreads();
    if (__builtin_amdgcn_readlane(l.f, s) != LC_F_READ) {
      ver += 1;
      val = __builtin_amdgcn_readlane(l.val, s);
    }
    mask |= 1ull << s;
    cnt.nodes++;
  }
  *depth_out = depth;
  return kWsFound;
}

// Decided keys without a witness, listed for the search; the longest of them.
__global__ __launch_bounds__(256) void witness_compact_kernel(
    const lc_key_result *__restrict__ out, const int32_t *__restrict__ kind,
    const int64_t *__restrict__ key_off, const int64_t n_keys, int32_t *__restrict__ keys,
    WitnessStatus *__restrict__ st) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; k0 < n_keys; k0 += stride) {
    const int64_t k = k0 + lane;
    bool take = false;
    int64_t len = 0;
    if (k < n_keys) {
      const int v = out[k].verdict;
      take = (v == LC_VALID || v == LC_INVALID) && kind[k] == LC_WITNESS_NONE;
      len = key_off[k + 1] - key_off[k];
    }
    const uint64_t b = __ballot(take);
    if (!b) continue;
    int pos = 0;
    if (lane == 0) pos = atomicAdd(&st->n_list, __popcll(b));
    pos = uni(pos);
    if (take) {
      keys[pos + lanes_below(b)] = (int32_t)k;
      atomicMax(&st->max_len, (int32_t)(len > INT32_MAX ? INT32_MAX : len));
    }
  }
}

__global__ __launch_bounds__(kWave) void witness_search_kernel(
    const lc_op *__restrict__ ops, const int64_t *__restrict__ key_off,
    const int32_t *__restrict__ keys, const int32_t n_list, const KParams p,
    const lc_key_result *__restrict__ out, int32_t *__restrict__ wit, int32_t *__restrict__ wkind,
    char *__restrict__ ws, const int64_t max_n, WitnessStatus *__restrict__ st,
    int32_t *__restrict__ wlist) {
  __shared__ WsWindow w;
  const int lane = threadIdx.x;
  char *mine = ws + (size_t)blockIdx.x * witness_wave_bytes(max_n);
  const int64_t cap_n = witness_round(max_n);
  WsKey key;
  key.cache = reinterpret_cast<WsBucket *>(mine);
  key.bmask = kWitnessBuckets - 1;
  key.fr = reinterpret_cast<WsFrame *>(mine + (size_t)kWitnessBuckets * sizeof(WsBucket));
  key.ev = reinterpret_cast<WsEvent *>(reinterpret_cast<char *>(key.fr) + (size_t)cap_n * sizeof(WsFrame));
  key.slots = reinterpret_cast<uint8_t *>(reinterpret_cast<char *>(key.ev) + (size_t)cap_n * sizeof(WsEvent));
  {  // every cache entry stale
    uint4 *z = reinterpret_cast<uint4 *>(key.cache);
    for (int i = lane; i < kWitnessBuckets * (int)(sizeof(WsBucket) / sizeof(uint4)); i += kWave)
      z[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
  }
  key.gen = 0;
  const int64_t first = key_off[0];
  for (;;) {  // list entries claimed one at a time
    int li = 0;
    if (lane == 0) li = atomicAdd(&st->next, 1);
    li = uni(li);
    if (li >= n_list) break;
    const int64_t kid = uni(keys[li]);
    const int64_t beg = (int64_t)uni64((uint64_t)key_off[kid]);
    const int64_t end = (int64_t)uni64((uint64_t)key_off[kid + 1]);
    const int64_t len = end - beg;
    const lc_key_result res = out[kid];
    const bool valid = uni(res.verdict) == LC_VALID;
    int32_t *kw = wit + (beg - first);
    int r = kWsBudget, depth = 0;
    WsCount cnt{0, 0};
    if (len <= 0) {
      r = kWsFound;
    } else if (len <= max_n) {
      key.kops = ops + (beg - first);
      key.n = (int)len;
      key.base_idx = (int64_t)uni64((uint64_t)key.kops[0].call);
      key.gen++;
      const int64_t rel = uni64((uint64_t)res.fail_prefix_end) - 1 - key.base_idx;
      const uint32_t cut = valid ? kNever - 1 : (uint32_t)(rel < 0 ? 0 : rel > (int64_t)(kNever - 1) ? kNever - 1 : rel);
      if (valid || rel >= 0) r = ws_search(w, key, p, cut, &depth, cnt, lane);
      __syncthreads();
    }
    if (r == kWsFound) {
      for (int64_t j = lane; j < len; j += kWave) kw[j] = -1;
      __syncthreads();
      for (int j = lane; j < depth; j += kWave) kw[key.fr[j].rec] = j;
      if (lane == 0) wkind[kid] = valid ? LC_WITNESS_ORDER_FULL : LC_WITNESS_ORDER_PREFIX;
    }
    if (lane == 0) {
      atomicAdd(r == kWsFound ? &st->n_found : r == kWsWindow ? &st->n_window : &st->n_budget, 1);
      atomicAdd(&st->nodes, (unsigned long long)cnt.nodes);
      atomicAdd(&st->cache_hits, (unsigned long long)cnt.hits);
      if (r == kWsWindow) wlist[atomicAdd(&st->n_wlist, 1)] = (int32_t)kid;  // for the counted stage
    }
  }
}

// ==================================================================
// Counted witness stage (LC_FLAG_COUNTED_WITNESS)
// ==================================================================
//
// The stage above gives every open op a window slot and lets a crashed op
// keep its slot, so a key with more than 64 ops open at once (n_window) gets
// no order: the keys the counted tier decides.  This stage searches those
// keys again with the counted tier's layout (counted.h): crashed writes/CAS
// with equal (f, value, expected, version) are interchangeable and are
// linearized in call order, so a node needs only HOW MANY members of each
// class it has linearized.
//   * Class c owns a count field of the node's mask (shift_c, width_c) and
//     lane 63 - c, whose window entry holds the class's precondition and
//     effect; the low `slots` bits / lanes are the window slots of the :ok ops.
//   * Event pass: the call of a crashed write/CAS takes no slot; the record's
//     byte names its class (kCwClass | c) and the record joins its class's
//     member list (call order; the lists lie one behind the other in `mem`).
//     A crashed read takes no slot and is never ranked (kCwNone): it has no
//     return to honour.  Every other record takes the lowest free slot.
//   * Search: ws_search's loop.  `called` (per class lane) counts the class's
//     members among the records admitted; class lane c is a candidate iff its
//     precondition holds, field(mask, c) < called and no slot holds an
//     unlinearized :ok op of the same tuple (deadline order: crashed members
//     go last).  Taking it ranks member number field(mask, c), steps the
//     state and adds 1 << shift_c to the mask.  Class lanes are tried last
//     (their return is "never"), ties by lane, as ws_pick does.
// A key outside the layout rule, or with more than `slots` :ok ops open at
// once, is left as it was (n_unfit).
enum { kCwFound = 0, kCwBudget = 1, kCwUnfit = 2 };
constexpr int kCwClass = 0x80, kCwNone = 0xFF;  // a record's byte: slot | kCwClass + class | kCwNone

// The class table: lane 63 - c holds class c, every other lane zeros.
struct CwClasses {
  int f, val, exp, ver;     // the tuple
  int nv, nvm, nl, nlm;     // its precondition
  int shift, width;         // its count field
  int members, start;       // members in the whole key; where its list starts in mem
  int called;               // members among the records admitted (search)
  uint64_t clsmask;         // lanes that hold a class
  uint64_t slotmask;        // lanes / mask bits that are window slots
};

// Pre-pass over the key's records: the classes in order of first call and the
// layout by counted.h's rule (what lc_counted_plan reports).  Returns whether
// the key fits.
__device__ bool cw_classes(const WsKey &key, CwClasses &cc, int lane) {
  cc = CwClasses{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0ull, ~0ull};
  int ncls = 0;
  for (int b = 0; b < key.n; b += kWave) {
    const Rec r = decode(load_raw(key.kops, b + lane, key.n), key.base_idx);
    uint64_t todo = __ballot((r.f == LC_F_WRITE || r.f == LC_F_CAS) && r.ret == kNever &&
                             r.call != kNever);
    while (todo) {
      const int l = first_lane(todo);
      const int f = __builtin_amdgcn_readlane(r.f, l), val = __builtin_amdgcn_readlane(r.val, l);
      const int ex = __builtin_amdgcn_readlane(r.exp, l), ver = __builtin_amdgcn_readlane(r.ver, l);
      const uint64_t same = todo & __ballot(r.f == f && r.val == val && r.exp == ex && r.ver == ver);
      todo &= ~same;  // (l included)
      const uint64_t hit =
          __ballot(cc.f == f && cc.val == val && cc.exp == ex && cc.ver == ver) & cc.clsmask;
      int cl;  // the class's lane
      if (hit) {
        cl = first_lane(hit);
      } else {
        if (ncls == lccount::kCountedMaxClasses) return false;
        cl = kWave - 1 - ncls++;
        cc.clsmask |= 1ull << cl;
        const int nv = __builtin_amdgcn_readlane(r.nv, l), nvm = __builtin_amdgcn_readlane(r.nvm, l);
        const int nl = __builtin_amdgcn_readlane(r.nl, l), nlm = __builtin_amdgcn_readlane(r.nlm, l);
        if (lane == cl) {
          cc.f = f;
          cc.val = val;
          cc.exp = ex;
          cc.ver = ver;
          cc.nv = nv;
          cc.nvm = nvm;
          cc.nl = nl;
          cc.nlm = nlm;
        }
      }
      if (lane == cl) cc.members += __popcll(same);
    }
  }
  int bits = 0, start = 0;
  for (int c = 0; c < ncls; c++) {
    const int cl = kWave - 1 - c;
    const int m = __builtin_amdgcn_readlane(cc.members, cl);
    const int wd = lccount::counted_width(m);
    bits += wd;
    if (lane == cl) {
      cc.width = wd;
      cc.shift = 64 - bits;
      cc.start = start;
    }
    start += m;
  }
  const int slots = lccount::counted_slots(bits, ncls);
  if (!lccount::counted_fits(ncls, slots)) return false;
  cc.slotmask = slots == 64 ? ~0ull : (1ull << slots) - 1;
  return true;
}

// `byte`: one record's byte per lane (kCwNone on idle lanes).  Every class's
// `called` moves by `sign` per member among them.
__device__ __forceinline__ void cw_count(int byte, int sign, CwClasses &cc, int lane) {
  uint64_t todo = __ballot((byte & 0xC0) == kCwClass);
  while (todo) {
    const int b = __builtin_amdgcn_readlane(byte, first_lane(todo));
    const uint64_t same = __ballot(byte == b);
    todo &= ~same;
    if (lane == kWave - 1 - (b & 0x3F)) cc.called += sign * __popcll(same);
  }
}

// Records [r0, r1) are called: slots filled, class members counted.
__device__ __forceinline__ void cw_admit(WsWindow &w, const WsKey &key, CwClasses &cc, int r0, int r1,
                                         int lane) {
  for (int b = r0; b < r1; b += kWave) {
    const int r = b + lane;
    int byte = kCwNone;
    if (r < r1) {
      byte = key.slots[r];
      if (byte < kWave) ws_put(w, key, r, byte);
    }
    cw_count(byte, 1, cc, lane);
  }
}

// ws_rewind with class members: the ones called since are counted out.
__device__ __forceinline__ void cw_rewind(WsWindow &w, const WsKey &key, CwClasses &cc, int k_from,
                                          int k_to, int lane) {
  const int c_to = uni(key.ev[k_to].ncalls), c_from = uni(key.ev[k_from].ncalls);
  for (int b = c_to; b < c_from; b += kWave) {  // called since: out
    const int r = b + lane;
    int byte = kCwNone;
    if (r < c_from) {
      byte = key.slots[r];
      if (byte < kWave) w.rec[byte] = -1;
    }
    cw_count(byte, -1, cc, lane);
  }
  __syncthreads();
  for (int b = k_to; b < k_from; b += kWave) {  // returned since, called before: back in
    const int j = b + lane;
    if (j < k_from) {
      const WsEvent e = key.ev[j];
      if (e.rec < c_to) ws_put(w, key, e.rec, e.slot);
    }
  }
}

// Search one key; on kCwFound *depth frames hold the order.  mem: the member
// lists (one int32 per record of room).
__device__ int cw_search(WsWindow &w, const WsKey &key, int32_t *mem, const KParams &p, uint32_t cut,
                         int *depth_out, WsCount &cnt, int lane) {
  const int n = key.n;
  CwClasses cc;
  if (!cw_classes(key, cc, lane)) return kCwUnfit;
  const bool iscls = (cc.clsmask >> lane) & 1;
  // ---- 1. event pass
  int K = 0;
  {
    uint64_t occ = 0;
    uint32_t wret = kNever;
    int wrec = -1, mybyte = kCwNone, seen = 0, i = 0, base = 0, bad = 0;
    Rec cur = decode(load_raw(key.kops, lane, n), key.base_idx);
    bad |= cur.bad;
    for (;;) {
      if (i < n && i - base >= kWave) {  // next chunk of records
        if (base + lane < n) key.slots[base + lane] = (uint8_t)mybyte;
        base += kWave;
        cur = decode(load_raw(key.kops, base + lane, n), key.base_idx);
        bad |= cur.bad;
      }
      const uint32_t ncall = i < n ? (uint32_t)__builtin_amdgcn_readlane((int)cur.call, i - base) : kNever;
      const uint32_t mret = wave_min_u32(wret);
      const uint32_t t = umin(ncall, mret);
      if (t == kNever || t > cut) break;
      if (mret <= ncall) {  // a return
        const int sm = first_lane(__ballot(wret == mret));
        const int x = __builtin_amdgcn_readlane(wrec, sm);
        if (lane == 0) key.ev[K] = WsEvent{x, i, sm, 0};
        K++;
        occ &= ~(1ull << sm);
        if (lane == sm) {
          wret = kNever;
          wrec = -1;
        }
      } else {  // the call of record i
        const int li = i - base;
        const uint32_t rt = (uint32_t)__builtin_amdgcn_readlane((int)cur.ret, li);
        int byte = kCwNone;
        if (rt == kNever) {  // crashed: a class member, or a read left out
          const int f = __builtin_amdgcn_readlane(cur.f, li);
          if (f == LC_F_WRITE || f == LC_F_CAS) {
            const int val = __builtin_amdgcn_readlane(cur.val, li);
            const int ex = __builtin_amdgcn_readlane(cur.exp, li);
            const int ver = __builtin_amdgcn_readlane(cur.ver, li);
            const uint64_t hit =
                __ballot(cc.f == f && cc.val == val && cc.exp == ex && cc.ver == ver) & cc.clsmask;
            if (!hit) return kCwUnfit;  // (cw_classes saw every such record)
            const int cl = first_lane(hit);
            const int pos = __builtin_amdgcn_readlane(cc.start, cl) + __builtin_amdgcn_readlane(seen, cl);
            if (pos >= n) return kCwUnfit;  // (start + members of all classes <= n)
            if (lane == 0) mem[pos] = i;
            if (lane == cl) seen++;
            byte = kCwClass | (kWave - 1 - cl);
          }
        } else {
          const uint64_t free_ = ~occ & cc.slotmask;
          if (!free_) return kCwUnfit;
          const int s = first_lane(free_);
          occ |= 1ull << s;
          if (lane == s) {
            wret = rt;
            wrec = i;
          }
          byte = s;
        }
        if (lane == li) mybyte = byte;
        i++;
      }
    }
    if (base + lane < n) key.slots[base + lane] = (uint8_t)mybyte;
    if (__ballot(bad != 0)) return kCwBudget;  // (no tier decides such a key)
  }
  // the window: slots free, class lanes hold their class for good
  w.rec[lane] = iscls ? -2 : -1;
  if (iscls) {
    w.nv[lane] = cc.nv;
    w.nvm[lane] = cc.nvm;
    w.nl[lane] = cc.nl;
    w.nlm[lane] = cc.nlm;
    w.f[lane] = cc.f;
    w.val[lane] = cc.val;
    w.ret[lane] = kNever;
  }
  __syncthreads();
  *depth_out = 0;
  if (K == 0) return kCwFound;

  // ---- 2. search
  const uint64_t t0 = p.time_ticks ? wall_clock64() : 0;
  const int64_t iter_limit = 16 * p.budget + 4 * (int64_t)n + 1024;
  int k = 0, depth = 0, ver = p.init_ver, val = p.init_val, n_ins = 0;
  uint64_t mask = 0;
  int64_t iters = 0;
  WsLane l;
  int ec = uni(key.ev[0].ncalls), es = uni(key.ev[0].slot);
  cw_admit(w, key, cc, 0, ec, lane);
  ws_refresh(w, l, lane);
  for (;;) {
    if (k == K) break;
    if (++iters > iter_limit || cnt.nodes > p.budget) return kCwBudget;
    if ((iters & 255) == 0 && p.time_ticks && wall_clock64() - t0 > p.time_ticks) return kCwBudget;
    const uint64_t xb = 1ull << es;
    if (mask & xb) {  // x is linearized: its return
      mask &= ~xb;
      if (lane == es) w.rec[es] = -1;
      __syncthreads();
      const int c0 = ec;
      k++;
      if (k < K) {
        ec = uni(key.ev[k].ncalls);
        es = uni(key.ev[k].slot);
        cw_admit(w, key, cc, c0, ec, lane);
      }
      ws_refresh(w, l, lane);
      continue;
    }
    bool dead = false;
    if (n_ins > 0 && ws_cache(key, k, mask, ver, val, false, lane)) {
      dead = true;
      cnt.hits++;
    }
    uint64_t cand = 0;
    if (!dead) {
      const bool ok = ws_pre_ok(l.nv, l.nvm, l.nl, l.nlm, ver, val);
      const uint64_t pend = __ballot(l.rec >= 0) & ~mask;  // ops in slots, not linearized
      cand = __ballot(ok) & pend;
      const int fld = (int)((mask >> cc.shift) & ((1ull << cc.width) - 1));
      uint64_t cls = __ballot(iscls && ok && fld < cc.called);
      for (uint64_t t = cls; t && pend; t &= t - 1) {  // crashed members after the :ok ones
        const int cl = first_lane(t);
        const int f = __builtin_amdgcn_readlane(l.f, cl), v = __builtin_amdgcn_readlane(l.val, cl);
        const int nl = __builtin_amdgcn_readlane(l.nl, cl), nv = __builtin_amdgcn_readlane(l.nv, cl);
        if (pend & __ballot(l.f == f && l.val == v && l.nl == nl && l.nv == nv)) cls &= ~(1ull << cl);
      }
      cand |= cls;
      if (!cand) {
        ws_cache(key, k, mask, ver, val, true, lane);
        n_ins++;
      }
    }
    int s;
    uint64_t rem;
    if (cand) {
      const uint64_t reads = cand & __ballot(l.f == LC_F_READ);
      if (reads) {
        s = (reads >> es) & 1 ? es : first_lane(reads);
        rem = 0;
      } else {
        s = ws_pick(cand, es, l, lane);
        rem = cand & ~(1ull << s);
      }
      depth++;
    } else {
      // dead end: back to the last frame with a candidate left
      for (;;) {
        if (depth == 0) return kCwBudget;  // no order: the tiers' verdict is not reproduced
        const WsFrame f = key.fr[depth - 1];
        const int fk = uni(f.k);
        if (fk != k) {
          cw_rewind(w, key, cc, k, fk, lane);
          ws_refresh(w, l, lane);
          k = fk;
          ec = uni(key.ev[k].ncalls);
          es = uni(key.ev[k].slot);
        }
        mask = uni64(f.mask);
        ver = uni(f.ver);
        val = uni(f.val);
        rem = uni64(f.rem);
        if (rem) break;
        ws_cache(key, k, mask, ver, val, true, lane);
        n_ins++;
        depth--;
        if (++iters > iter_limit) return kCwBudget;
      }
      s = ws_pick(rem, es, l, lane);
      rem &= ~(1ull << s);
    }
    // linearize lane s: frame depth - 1
    int rec;
    uint64_t nmask;
    if ((cc.clsmask >> s) & 1) {  // the class's next member
      const int sh = __builtin_amdgcn_readlane(cc.shift, s), wd = __builtin_amdgcn_readlane(cc.width, s);
      const int fld = (int)((mask >> sh) & ((1ull << wd) - 1));
      rec = uni(mem[__builtin_amdgcn_readlane(cc.start, s) + fld]);
      nmask = mask + (1ull << sh);
    } else {
      rec = __builtin_amdgcn_readlane(l.rec, s);
      nmask = mask | 1ull << s;
    }
    if ((unsigned)rec >= (unsigned)n || depth > n) return kCwBudget;  // (cannot be: the stores below stay inside)
    if (lane == 0) key.fr[depth - 1] = WsFrame{rec, k, rem, mask, ver, val};
    __syncthreads();
    if (__builtin_amdgcn_readlane(l.f, s) != LC_F_READ) {
      ver += 1;
      val = __builtin_amdgcn_readlane(l.val, s);
    }
    mask = nmask;
    cnt.nodes++;
  }
  *depth_out = depth;
  return kCwFound;
}

// The keys witness_search_kernel left at n_window (its list), one wavefront
// per key, claimed from st->cw_next.  Workspace per wave:
// witness_counted_wave_bytes(max_n), the first stage's layout and the member
// lists behind it.
__global__ __launch_bounds__(kWave) void witness_counted_kernel(
    const lc_op *__restrict__ ops, const int64_t *__restrict__ key_off,
    const int32_t *__restrict__ keys, const int32_t n_list, const KParams p,
    const lc_key_result *__restrict__ out, int32_t *__restrict__ wit, int32_t *__restrict__ wkind,
    char *__restrict__ ws, const int64_t max_n, WitnessStatus *__restrict__ st) {
  __shared__ WsWindow w;
  const int lane = threadIdx.x;
  char *mine = ws + (size_t)blockIdx.x * witness_counted_wave_bytes(max_n);
  const int64_t cap_n = witness_round(max_n);
  WsKey key;
  key.cache = reinterpret_cast<WsBucket *>(mine);
  key.bmask = kWitnessBuckets - 1;
  key.fr = reinterpret_cast<WsFrame *>(mine + (size_t)kWitnessBuckets * sizeof(WsBucket));
  key.ev = reinterpret_cast<WsEvent *>(reinterpret_cast<char *>(key.fr) + (size_t)cap_n * sizeof(WsFrame));
  key.slots = reinterpret_cast<uint8_t *>(reinterpret_cast<char *>(key.ev) + (size_t)cap_n * sizeof(WsEvent));
  int32_t *mem = reinterpret_cast<int32_t *>(mine + witness_wave_bytes(max_n));
  {  // every cache entry stale
    uint4 *z = reinterpret_cast<uint4 *>(key.cache);
    for (int i = lane; i < kWitnessBuckets * (int)(sizeof(WsBucket) / sizeof(uint4)); i += kWave)
      z[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
  }
  key.gen = 0;
  const int64_t first = key_off[0];
  for (;;) {  // list entries claimed one at a time
    int li = 0;
    if (lane == 0) li = atomicAdd(&st->cw_next, 1);
    li = uni(li);
    if (li >= n_list) break;
    const int64_t kid = uni(keys[li]);
    const int64_t beg = (int64_t)uni64((uint64_t)key_off[kid]);
    const int64_t end = (int64_t)uni64((uint64_t)key_off[kid + 1]);
    const int64_t len = end - beg;
    const lc_key_result res = out[kid];
    const bool valid = uni(res.verdict) == LC_VALID;
    int32_t *kw = wit + (beg - first);
    int r = kCwBudget, depth = 0;
    WsCount cnt{0, 0};
    if (len > 0 && len <= max_n) {  // (the first stage left no empty key)
      key.kops = ops + (beg - first);
      key.n = (int)len;
      key.base_idx = (int64_t)uni64((uint64_t)key.kops[0].call);
      key.gen++;
      const int64_t rel = uni64((uint64_t)res.fail_prefix_end) - 1 - key.base_idx;
      const uint32_t cut = valid ? kNever - 1 : (uint32_t)(rel < 0 ? 0 : rel > (int64_t)(kNever - 1) ? kNever - 1 : rel);
      if (valid || rel >= 0) r = cw_search(w, key, mem, p, cut, &depth, cnt, lane);
      __syncthreads();
    }
    if (r == kCwFound) {
      for (int64_t j = lane; j < len; j += kWave) kw[j] = -1;
      __syncthreads();
      for (int j = lane; j < depth; j += kWave) kw[key.fr[j].rec] = j;
      if (lane == 0) wkind[kid] = valid ? LC_WITNESS_ORDER_FULL : LC_WITNESS_ORDER_PREFIX;
    }
    if (lane == 0) {
      atomicAdd(r == kCwFound ? &st->cw_found : r == kCwUnfit ? &st->cw_unfit : &st->cw_budget, 1);
      atomicAdd(&st->cw_nodes, (unsigned long long)cnt.nodes);
      atomicAdd(&st->cw_hits, (unsigned long long)cnt.hits);
    }
  }
}

}  // namespace

size_t witness_ws_bytes(int n_waves, int64_t max_n) {
  return (size_t)n_waves * witness_wave_bytes(max_n);
}

hipError_t launch_witness_compact(const lc_key_result *d_out, const int32_t *d_kind,
                                  const int64_t *d_key_off, int64_t n_keys, int32_t *d_keys,
                                  WitnessStatus *d_st, hipStream_t stream) {
  if (n_keys <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>((n_keys + 255) / 256, 1024);
  hipLaunchKernelGGL(witness_compact_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, d_out,
                     d_kind, d_key_off, n_keys, d_keys, d_st);
  return hipGetLastError();
}

hipError_t launch_witness_search(const lc_op *d_ops, const int64_t *d_key_off, const int32_t *d_keys,
                                 int32_t n_list, const KParams &p, const lc_key_result *d_out,
                                 int32_t *d_witness, int32_t *d_witness_kind, void *d_ws, int n_waves,
                                 int64_t max_n, WitnessStatus *d_st, int32_t *d_window_keys,
                                 hipStream_t stream) {
  if (n_list <= 0 || n_waves <= 0) return hipSuccess;
  hipLaunchKernelGGL(witness_search_kernel, dim3((unsigned)n_waves), dim3(kWave), 0, stream, d_ops,
                     d_key_off, d_keys, n_list, p, d_out, d_witness, d_witness_kind,
                     static_cast<char *>(d_ws), max_n, d_st, d_window_keys);
  return hipGetLastError();
}

size_t witness_counted_ws_bytes(int n_waves, int64_t max_n) {
  return (size_t)n_waves * witness_counted_wave_bytes(max_n);
}

hipError_t launch_witness_counted(const lc_op *d_ops, const int64_t *d_key_off, const int32_t *d_keys,
                                  int32_t n_list, const KParams &p, const lc_key_result *d_out,
                                  int32_t *d_witness, int32_t *d_witness_kind, void *d_ws, int n_waves,
                                  int64_t max_n, WitnessStatus *d_st, hipStream_t stream) {
  if (n_list <= 0 || n_waves <= 0) return hipSuccess;
  hipLaunchKernelGGL(witness_counted_kernel, dim3((unsigned)n_waves), dim3(kWave), 0, stream, d_ops,
                     d_key_off, d_keys, n_list, p, d_out, d_witness, d_witness_kind,
                     static_cast<char *>(d_ws), max_n, d_st);
  return hipGetLastError();
}

}  // namespace lcdev
