// txngraph_dev.h — what the kernels of the two Elle checkers (append.hip,
// wr.hip, txngraph.hip) share on the device: the launch geometry, the two
// table formats behind functions, and a workgroup's counters flushed onto the
// sharded ones.  Every device function is __device__ __forceinline__.
//
//  The key table: a word is the key xor 2^63 - 1 (kKeyXor), so that the
//    reserved key is ~0: empty.  One 64-bit compare-and-swap on the key,
//    linear probing.
//  A pair table over (key, value): a word is (hash tag << 32) | a mop that
//    names the pair, ~0 when empty — the pair itself is read from the mops,
//    so one 64-bit word decides a 128-bit key.  Both mop records have `key`
//    and `value`.
#pragma once
#include "txngraph.h"

namespace lctg {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxGrid = 256 * 8;
constexpr unsigned long long kEmptyWord = ~0ull;
constexpr int64_t kKeyXor = 0x7FFFFFFFFFFFFFFFll;  // a stored key is key ^ this: the reserved key reads ~0

inline int grid_for(int64_t items, int64_t per_block) {
  int64_t g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (int)(g < kMaxGrid ? g : kMaxGrid);
}

// The key's slot in the key table of kcap slots, claimed if nobody had it.
__device__ __forceinline__ int32_t key_claim(unsigned long long *ktab, uint64_t kcap, int64_t key) {
  const unsigned long long enc = (unsigned long long)(key ^ kKeyXor);
  uint64_t ks = mix64((uint64_t)key) & (kcap - 1);
  for (uint64_t p = 0; p < kcap; p++) {
    const unsigned long long old = atomicCAS(&ktab[ks], kEmptyWord, enc);
    if (old == kEmptyWord || old == enc) break;
    ks = (ks + 1) & (kcap - 1);
  }
  return (int32_t)ks;
}

template <class Mop>
__device__ __forceinline__ bool names_pair(const Mop *mops, unsigned long long word, uint64_t h, int64_t key,
                                           int64_t value) {
  if ((word >> 32) != (h >> 32)) return false;
  const Mop &o = mops[(uint32_t)word];
  return o.key == key && o.value == value;
}

// mop m's pair into the pair table of cap slots: the pair's slot, or -1 where
// the table is full (never: it has two slots per mop); *inserted says whether
// this call made the entry or found it.
template <class Mop>
__device__ __forceinline__ int32_t pair_claim(unsigned long long *tab, uint64_t cap, const Mop *mops, int64_t m,
                                              int64_t key, int64_t value, bool *inserted) {
  const uint64_t h = hash_pair(key, value);
  const unsigned long long word = ((h >> 32) << 32) | (unsigned long long)(uint32_t)m;
  uint64_t s = h & (cap - 1);
  *inserted = false;
  for (uint64_t p = 0; p < cap; p++) {
    const unsigned long long old = atomicCAS(&tab[s], kEmptyWord, word);
    if (old == kEmptyWord) {
      *inserted = true;
      return (int32_t)s;
    }
    if (names_pair(mops, old, h, key, value)) return (int32_t)s;
    s = (s + 1) & (cap - 1);
  }
  return -1;
}

// The slot of (key, value) in the pair table, or -1; *mop, where wanted, the
// mop its word names.
template <class Mop>
__device__ __forceinline__ int32_t pair_find(const unsigned long long *tab, uint64_t cap, const Mop *mops, int64_t key,
                                             int64_t value, int32_t *mop = nullptr) {
  const uint64_t h = hash_pair(key, value);
  uint64_t s = h & (cap - 1);
  for (uint64_t p = 0; p < cap; p++) {
    const unsigned long long word = tab[s];
    if (word == kEmptyWord) return -1;
    if (names_pair(mops, word, h, key, value)) {
      if (mop) *mop = (int32_t)(uint32_t)word;
      return (int32_t)s;
    }
    s = (s + 1) & (cap - 1);
  }
  return -1;
}

// A workgroup's kCounters thread-local counts onto the sharded counters:
// summed per wave, then across the waves through the LDS, then one atomicAdd
// per counter onto the workgroup's shard.  Every thread of the workgroup
// calls it, once.
template <int kCounters>
__device__ __forceinline__ void flush_counters(const long long (&cnt)[kCounters], int64_t *counters) {
  __shared__ long long s_cnt[kWaves][kCounters];
  for (int b = 0; b < kCounters; b++) {
    long long v = cnt[b];
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6][b] = v;
  }
  __syncthreads();
  if (threadIdx.x < kCounters) {
    long long v = 0;
    for (int i = 0; i < kWaves; i++) v += s_cnt[i][threadIdx.x];
    if (v)
      atomicAdd(reinterpret_cast<unsigned long long *>(
                    &counters[((int64_t)threadIdx.x * kCounterShards + blockIdx.x % kCounterShards) * kCounterStride]),
                (unsigned long long)v);
  }
}

}  // namespace lctg
