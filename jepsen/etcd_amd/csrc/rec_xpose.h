// rec_xpose.h — a wave's 64 consecutive 48-byte records read as three fully
// coalesced 1-KB wave-instructions and handed to their lanes by an in-wave
// transpose: no LDS buffer, no barrier.  (No other header needed: the read
// probe in tools/ includes this file too.)
//
// In 16-byte chunks from the first record of the wave, instruction i of
// {0, 1, 2} has lane l load chunk 64 i + l into X_i.  Part p (the first,
// second or third 16 bytes) of lane q's record is chunk 3 q + p: it sits in
// lane (3 q + p) & 63, register X_((3 q + p) >> 6).  Because 64 = 1 (mod 3), a
// source lane l is asked for one register per part whoever asks:
// X_((p - l) mod 3).  So per part each lane selects that register (lane
// dependent) and every lane fetches its four dwords with ds_bpermute_b32.
#pragma once
#include <stdint.h>

namespace lcdev {

constexpr int kXpLanes = 64, kXpParts = 3;
// where part p of lane q's record was loaded
constexpr int xp_src_lane(int q, int p) { return (kXpParts * q + p) & (kXpLanes - 1); }
constexpr int xp_src_reg(int q, int p) { return (kXpParts * q + p) / kXpLanes; }
// the register source lane l offers to the lanes that want a part p of it
constexpr int xp_offer(int l, int p) { return ((p - l) % kXpParts + kXpParts) % kXpParts; }

// (lane, part) -> (source lane, register) is a bijection onto the 192 loaded
// chunks, and the register a source lane offers for part p is the one every
// lane asking it for part p needs.
constexpr bool xp_mapping_ok() {
  bool seen[kXpParts][kXpLanes] = {};
  for (int q = 0; q < kXpLanes; q++)
    for (int p = 0; p < kXpParts; p++) {
      const int l = xp_src_lane(q, p), i = xp_src_reg(q, p);
      if (i < 0 || i >= kXpParts || seen[i][l]) return false;
      seen[i][l] = true;
      if (xp_offer(l, p) != i) return false;
      if (kXpLanes * i + l != kXpParts * q + p) return false;
    }
  return true;
}
static_assert(xp_mapping_ok(), "record transpose: the chunk mapping is not a bijection");

// In place: on entry the 48 bytes of `rec` are (X_0, X_1, X_2) of this lane,
// on return they are this lane's record.  Every lane of the wave must be
// active (a permute reads nothing from an inactive lane).  The select is
// written with masks: as nested conditionals the compiler turns it into
// branches on lane mod 3.
template <class T>
__device__ __forceinline__ void wave_xpose48(T &rec, int lane) {
  static_assert(sizeof(T) == 16 * kXpParts, "a 48-byte record");
  int x[4 * kXpParts], y[4 * kXpParts];
  __builtin_memcpy(x, &rec, sizeof(T));
  const int k = lane % kXpParts;
#pragma unroll
  for (int p = 0; p < kXpParts; p++) {
    // xp_offer(lane, p) with k = lane mod 3: X_0 when k == p, X_1 when
    // k == p - 1 (mod 3), else X_2
    int m0 = -(int)(k == p), m1 = -(int)(k == (p + kXpParts - 1) % kXpParts);
    asm volatile("" : "+v"(m0), "+v"(m1));
    const int src = ((kXpParts * lane + p) & (kXpLanes - 1)) << 2;
#pragma unroll
    for (int d = 0; d < 4; d++) {
      const int x12 = (x[4 + d] & m1) | (x[8 + d] & ~m1);
      const int offer = (x[d] & m0) | (x12 & ~m0);
      y[4 * p + d] = __builtin_amdgcn_ds_bpermute(src, offer);
    }
  }
  __builtin_memcpy(&rec, y, sizeof(T));
}

// The 16-byte chunk index, from the key's first record, that lane `lane` of
// wave `w` loads with instruction i of record group u (records u * threads +
// 64 w ... + 63).
__device__ __forceinline__ int xp_chunk(int u, int w, int i, int lane, int threads) {
  return kXpParts * (u * threads + w * kXpLanes) + kXpLanes * i + lane;
}

// The loads go through a buffer descriptor over the key's bytes (base:
// wave-uniform, 16-byte aligned), whose range check returns zeros at or past
// the key's end: no branch around a load, so each wait counts exactly the
// loads issued after the one it needs.  NT: non-temporal.  Such loads bypass
// L1, which costs nothing here: a line is asked for by one instruction, or by
// two where a key does not start on a line boundary.
typedef unsigned int xp_u32x4 __attribute__((ext_vector_type(4)));
struct XpKey {
  __amdgpu_buffer_rsrc_t rs;
};
__device__ __forceinline__ XpKey xp_key(const void *base, int bytes) {
  const uint64_t a = reinterpret_cast<uint64_t>(base);
  const uint32_t lo = __builtin_amdgcn_readfirstlane((int)(uint32_t)a);
  const uint32_t hi = __builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
  void *b = reinterpret_cast<void *>(((uint64_t)hi << 32) | lo);
  return XpKey{__builtin_amdgcn_make_buffer_rsrc(b, (short)0, __builtin_amdgcn_readfirstlane(bytes),
                                                 0x00020000)};
}
template <bool NT>
__device__ __forceinline__ xp_u32x4 xp_load(const XpKey &k, int ch) {
  return __builtin_amdgcn_raw_buffer_load_b128(k.rs, ch * 16, 0, NT ? 2 : 0);
}

}  // namespace lcdev
