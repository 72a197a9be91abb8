// Dev probe (not product code): read-rate ceilings for the fast tier's access
// shape.  One 256-thread workgroup per 48-KB "key" (1,000 records x 48 B),
// 10,000 keys = the 480 MB C2 launch.  Variants:
//   strided       - lane i loads record i as three 16-B loads at a 48-B stride
//   coal          - each wave-instruction loads 1 KB contiguous (lane i, chunk i)
//   coal_nt       - coal with non-temporal loads
//   coal_xpose    - coal per wave over its own 64 records (range-checked buffer
//                   loads), then the in-wave transpose of rec_xpose.h hands
//                   every lane its record
//   coal_nt_xpose - the same with non-temporal loads
//   coal_lds      - coalesced loads, then the 3 KB per wave transposed through LDS
//   strided_nt    - strided with non-temporal loads
//   hybrid        - parts a, b by register loads, part c by LDS-DMA nt
//   glds, glds_nt - the key straight into LDS by LDS-DMA, folded from LDS
//   persistN      - N workgroups walk the keys, next key's loads issued early
// Residency: fast_tier_kernel runs 7 workgroups per CU (72 VGPRs).  Every
// variant whose own LDS allows it is launched with a dynamic-LDS pad that
// gives it the same 7 (21 KB per workgroup of the CU's 160 KB); the occupancy
// the runtime reports is printed beside each figure.  coal_lds / glds hold 48
// KB and stay at 3.
// Every variant folds what it loaded into one word per key, each 16-byte
// chunk weighted by its index in the key and each dword by its place in the
// chunk, so a record part delivered to the wrong lane or slot changes the
// word; every variant's words are compared with the first strided run's.
// `strided` runs first and last; the gate line at the end says whether a
// transposed variant beat both by more than they differ from each other.
// Build: hipcc --offload-arch=gfx950 -O3 -Ijepsen/etcd_amd/csrc tools/probe_scan.hip -o tools/probe_scan
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

#include "rec_xpose.h"

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e)); return 1; } } while (0)

constexpr int kRec = 1000, kKeys = 10000, kT = 256;
constexpr int kPadTo = 21 * 1024;  // LDS per workgroup for 7 per CU (8 would need <= 20 KB)

struct Chunk {
  longlong2 v[3];
};

typedef long long v2ll __attribute__((ext_vector_type(2)));
// chunk ch of the key at q, zeros at or past nch chunks
template <bool NT>
__device__ __forceinline__ longlong2 ld(const longlong2 *q, int ch, int nch) {
  if (ch >= nch) return make_longlong2(0, 0);
  if constexpr (NT) {
    const v2ll t = __builtin_nontemporal_load(reinterpret_cast<const v2ll *>(q) + ch);
    return make_longlong2(t.x, t.y);
  } else {
    return q[ch];
  }
}

// chunk ch of the key holds v
__device__ __forceinline__ uint32_t fold(int ch, longlong2 v) {
  const uint32_t d0 = (uint32_t)v.x, d1 = (uint32_t)((uint64_t)v.x >> 32);
  const uint32_t d2 = (uint32_t)v.y, d3 = (uint32_t)((uint64_t)v.y >> 32);
  return (d0 * 3u + d1 * 5u + d2 * 7u + d3 * 11u) * (2u * (uint32_t)ch + 1u);
}
__device__ __forceinline__ void finish(uint32_t acc, uint32_t *s, int64_t *out, int key) {
  if (threadIdx.x == 0) *s = 0;
  __syncthreads();
  atomicAdd(s, acc);
  __syncthreads();
  if (threadIdx.x == 0) out[key] = *s;
}

template <bool NT>
__global__ __launch_bounds__(kT) void strided(const longlong2 *__restrict__ p, const int64_t *__restrict__ off,
                                               int64_t *__restrict__ out) {
  __shared__ uint32_t s;
  const int64_t beg = off[blockIdx.x], n = off[blockIdx.x + 1] - beg;
  const longlong2 *q = p + beg * 3;
  const int nch = (int)n * 3;
  Chunk x[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int r = threadIdx.x + u * kT;
#pragma unroll
    for (int i = 0; i < 3; i++) {
      // (r < n: all three chunks are inside the key)
      x[u].v[i] = ld<NT>(q, 3 * r + i, r < n ? nch : 0);
    }
  }
  uint32_t acc = 0;
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int i = 0; i < 3; i++) acc += fold(3 * (threadIdx.x + u * kT) + i, x[u].v[i]);
  finish(acc, &s, out, blockIdx.x);
}

template <bool NT>
__global__ __launch_bounds__(kT) void coal(const longlong2 *__restrict__ p, const int64_t *__restrict__ off,
                                           int64_t *__restrict__ out) {
  __shared__ uint32_t s;
  const int64_t beg = off[blockIdx.x], n = off[blockIdx.x + 1] - beg;
  const longlong2 *q = p + beg * 3;
  const int nch = (int)n * 3;
  longlong2 a[12];
#pragma unroll
  for (int u = 0; u < 12; u++) a[u] = ld<NT>(q, threadIdx.x + u * kT, nch);
  uint32_t acc = 0;
#pragma unroll
  for (int u = 0; u < 12; u++) acc += fold(threadIdx.x + u * kT, a[u]);
  finish(acc, &s, out, blockIdx.x);
}

// The shape proposed for fast_tier_kernel: per wave and record group three
// coalesced 1-KB loads, the group transposed in place as it is consumed.
template <bool NT>
__global__ __launch_bounds__(kT) void coal_xpose(const longlong2 *__restrict__ p, const int64_t *__restrict__ off,
                                                 int64_t *__restrict__ out) {
  __shared__ uint32_t s;
  const int64_t beg = off[blockIdx.x], n = off[blockIdx.x + 1] - beg;
  const longlong2 *q = p + beg * 3;
  const lcdev::XpKey kb = lcdev::xp_key(q, (int)n * 48);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  Chunk x[4];
#pragma unroll
  for (int u = 0; u < 4; u++)
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const lcdev::xp_u32x4 t = lcdev::xp_load<NT>(kb, lcdev::xp_chunk(u, w, i, lane, kT));
      __builtin_memcpy(&x[u].v[i], &t, 16);
    }
  uint32_t acc = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    lcdev::wave_xpose48(x[u], lane);
#pragma unroll
    for (int i = 0; i < 3; i++) acc += fold(3 * (threadIdx.x + u * kT) + i, x[u].v[i]);
  }
  finish(acc, &s, out, blockIdx.x);
}

// coalesced loads, records re-assembled through LDS (48 KB per workgroup)
__global__ __launch_bounds__(kT) void coal_lds(const longlong2 *__restrict__ p, const int64_t *__restrict__ off,
                                               int64_t *__restrict__ out) {
  __shared__ longlong2 L[3 * 1024];
  __shared__ uint32_t s;
  const int64_t beg = off[blockIdx.x], n = off[blockIdx.x + 1] - beg;
  const longlong2 *q = p + beg * 3;
  const int nch = (int)n * 3;
  longlong2 a[12];
#pragma unroll
  for (int u = 0; u < 12; u++) {
    const int ch = threadIdx.x + u * kT;
    a[u] = ch < nch ? q[ch] : make_longlong2(0, 0);
  }
#pragma unroll
  for (int u = 0; u < 12; u++) L[threadIdx.x + u * kT] = a[u];
  __syncthreads();
  uint32_t acc = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int r = threadIdx.x + u * kT;
#pragma unroll
    for (int i = 0; i < 3; i++) acc += fold(3 * r + i, L[3 * r + i]);
  }
  finish(acc, &s, out, blockIdx.x);
}

// Persistent: grid of G workgroups walks keys blockIdx.x, +G, ...; coalesced
// loads of the next key issued before folding the current one.
__global__ __launch_bounds__(kT) void persist(const longlong2 *__restrict__ p, const int64_t *__restrict__ off,
                                              int64_t *__restrict__ out, int nkeys) {
  __shared__ uint32_t s;
  longlong2 a[12];
  int key = blockIdx.x;
  auto issue = [&](int k) {
    const int64_t beg = off[k], n = off[k + 1] - beg;
    const longlong2 *q = p + beg * 3;
    const int nch = (int)n * 3;
#pragma unroll
    for (int u = 0; u < 12; u++) {
      const int ch = threadIdx.x + u * kT;
      a[u] = ch < nch ? q[ch] : make_longlong2(0, 0);
    }
  };
  if (key < nkeys) issue(key);
  for (; key < nkeys; key += gridDim.x) {
    uint32_t acc = 0;
#pragma unroll
    for (int u = 0; u < 12; u++) acc += fold(threadIdx.x + u * kT, a[u]);
    if (key + (int)gridDim.x < nkeys) issue(key + gridDim.x);
    finish(acc, &s, out, key);
    __syncthreads();
  }
}

// LDS-DMA: the key's 48 KB straight into LDS (global_load_lds_dwordx4, 1 KB
// per wave-instruction), then folded from LDS.  AUX 0 = default policy, 2 = nt.
// (A key's last row reads up to 63 chunks past its end: main() pads the
// buffer, and the fold leaves them out.)
template <int AUX>
__global__ __launch_bounds__(kT) void glds(const longlong2 *__restrict__ p, const int64_t *__restrict__ off,
                                           int64_t *__restrict__ out) {
  __shared__ longlong2 L[3 * 1024];
  __shared__ uint32_t s;
  const int64_t beg = off[blockIdx.x], n = off[blockIdx.x + 1] - beg;
  const longlong2 *q = p + beg * 3;
  const int nch = (int)n * 3;
  const int w = threadIdx.x / 64;
#pragma unroll
  for (int u = 0; u < 12; u++) {
    const int ch = threadIdx.x + u * kT;
    if (u * kT + w * 64 < nch)  // wave-uniform
      __builtin_amdgcn_global_load_lds((const void *)(q + ch), (__attribute__((address_space(3))) void *)(L + u * kT + w * 64), 16, 0, AUX);
  }
  __builtin_amdgcn_s_waitcnt(0);  // vmcnt(0) lgkmcnt(0) expcnt(0)
  __syncthreads();
  uint32_t acc = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int r = threadIdx.x + u * kT;
    if (r < n) {
#pragma unroll
      for (int i = 0; i < 3; i++) acc += fold(3 * r + i, L[3 * r + i]);
    }
  }
  finish(acc, &s, out, blockIdx.x);
}

// Hybrid: per record, chunks a and b by register loads, chunk c (call, ret)
// by LDS-DMA nt into a 16 KB per-workgroup LDS array (per-lane source
// addresses, contiguous LDS destination).
__global__ __launch_bounds__(kT) void hybrid(const longlong2 *__restrict__ p, const int64_t *__restrict__ off,
                                             int64_t *__restrict__ out) {
  __shared__ longlong2 C[1024];
  __shared__ uint32_t s;
  const int64_t beg = off[blockIdx.x], n = off[blockIdx.x + 1] - beg;
  const longlong2 *q = p + beg * 3;
  const int w = threadIdx.x / 64;
  longlong2 a[4], b[4];
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int r = threadIdx.x + u * kT;
    if (r < n) {
      __builtin_amdgcn_global_load_lds((const void *)(q + 3 * r + 2),
                                       (__attribute__((address_space(3))) void *)(C + u * kT + w * 64), 16, 0, 2);
      a[u] = q[3 * r];
      b[u] = q[3 * r + 1];
    } else {
      a[u] = b[u] = make_longlong2(0, 0);
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  uint32_t acc = 0;
#pragma unroll
  for (int u = 0; u < 4; u++) {
    const int r = threadIdx.x + u * kT;
    const longlong2 c = r < n ? C[r] : make_longlong2(0, 0);
    acc += fold(3 * r, a[u]) + fold(3 * r + 1, b[u]) + fold(3 * r + 2, c);
  }
  finish(acc, &s, out, blockIdx.x);
}

int main() {
  const size_t nrec = (size_t)kRec * kKeys;
  std::vector<int64_t> h(nrec * 6), ho(kKeys + 1), ref, got(kKeys);
  for (size_t i = 0; i < h.size(); i++) h[i] = (int64_t)(i * 2654435761u);
  for (int k = 0; k <= kKeys; k++) ho[k] = (int64_t)k * kRec;
  longlong2 *d;
  int64_t *doff, *dout;
  CK(hipMalloc(&d, nrec * 48 + 4096));  // (glds reads whole 1-KB rows)
  CK(hipMemset(d, 0, nrec * 48 + 4096));
  CK(hipMalloc(&doff, (kKeys + 1) * 8));
  CK(hipMalloc(&dout, kKeys * 8));
  CK(hipMemcpy(d, h.data(), nrec * 48, hipMemcpyHostToDevice));
  CK(hipMemcpy(doff, ho.data(), (kKeys + 1) * 8, hipMemcpyHostToDevice));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  struct Result {
    std::string name;
    float ms;
    bool ok;
  };
  std::vector<Result> res;
  printf("dynamic-LDS pad: every variant is launched with %d B of LDS per workgroup less its own static LDS,\n"
         "so the register variants run 7 workgroups per CU as fast_tier_kernel does (wg/CU column)\n",
         kPadTo);
  // kern: the kernel's address (occupancy query); lds: its static LDS bytes
  auto run = [&](const char *name, const void *kern, int lds, auto launch) {
    const int pad = lds < kPadTo ? kPadTo - lds : 0;
    int occ = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kern, kT, pad));
    CK(hipMemset(dout, 0xff, kKeys * 8));
    for (int i = 0; i < 3; i++) launch(pad);
    CK(hipDeviceSynchronize());
    CK(hipEventRecord(e0));
    const int it = 100;
    for (int i = 0; i < it; i++) launch(pad);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipGetLastError());
    float ms;
    CK(hipEventElapsedTime(&ms, e0, e1));
    ms /= it;
    CK(hipMemcpy(got.data(), dout, kKeys * 8, hipMemcpyDeviceToHost));
    if (ref.empty()) ref = got;
    const bool ok = memcmp(ref.data(), got.data(), kKeys * 8) == 0;
    printf("%-14s %.4f ms  %5.0f GB/s  wg/CU %d  pad %5d B  words %s\n", name, ms, nrec * 48.0 / ms / 1e6,
           occ, pad, ok ? "= strided" : "DIFFER");
    res.push_back({name, ms, ok});
    return 0;
  };
#define RUN(name, kern, lds, ...) \
  if (run(name, (const void *)(kern), lds, [&](int pad) { kern<<<kKeys, kT, pad>>>(__VA_ARGS__); })) return 1
  RUN("strided", strided<false>, 4, d, doff, dout);
  RUN("coal", coal<false>, 4, d, doff, dout);
  RUN("coal_nt", coal<true>, 4, d, doff, dout);
  RUN("coal_xpose", coal_xpose<false>, 4, d, doff, dout);
  RUN("coal_nt_xpose", coal_xpose<true>, 4, d, doff, dout);
  RUN("coal_lds", coal_lds, 48 * 1024 + 4, d, doff, dout);
  RUN("strided_nt", strided<true>, 4, d, doff, dout);
  RUN("hybrid", hybrid, 16 * 1024 + 4, d, doff, dout);
  RUN("glds", glds<0>, 48 * 1024 + 4, d, doff, dout);
  RUN("glds_nt", glds<2>, 48 * 1024 + 4, d, doff, dout);
  RUN("coal_nt", coal<true>, 4, d, doff, dout);
  RUN("coal_xpose", coal_xpose<false>, 4, d, doff, dout);
  RUN("coal_nt_xpose", coal_xpose<true>, 4, d, doff, dout);
  RUN("strided_nt", strided<true>, 4, d, doff, dout);
  RUN("hybrid", hybrid, 16 * 1024 + 4, d, doff, dout);
  RUN("strided", strided<false>, 4, d, doff, dout);
  for (int g : {256, 512, 1024, 2048}) {
    char nm[32];
    snprintf(nm, sizeof nm, "persist%d", g);
    if (run(nm, (const void *)persist, 4, [&](int pad) { persist<<<g, kT, pad>>>(d, doff, dout, kKeys); })) return 1;
  }
  // The gate: a transposed variant must beat both strided runs by more than
  // the two differ from each other (its slower run counts).
  float s_lo = 1e9f, s_hi = 0;
  for (const Result &r : res)
    if (r.name == "strided") { s_lo = fminf(s_lo, r.ms); s_hi = fmaxf(s_hi, r.ms); }
  const float need = s_lo - (s_hi - s_lo);
  printf("gate: strided %.4f and %.4f ms (differ by %.4f): a transposed variant passes below %.4f ms\n", s_lo,
         s_hi, s_hi - s_lo, need);
  bool all_ok = true;
  for (const Result &r : res) all_ok &= r.ok;
  for (const char *v : {"coal_xpose", "coal_nt_xpose"}) {
    float worst = 0;
    for (const Result &r : res)
      if (r.name == v) worst = fmaxf(worst, r.ms);
    printf("gate: %-14s slower run %.4f ms: %s\n", v, worst, worst < need ? "PASS" : "no");
  }
  if (!all_ok) printf("gate: VOID, a variant's words differ from strided's\n");
  return all_ok ? 0 : 2;
}
