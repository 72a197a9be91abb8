// check_host.cpp — lc_check / lc_check_ex (48-byte lc_op), lc_check32
// (24-byte lc_op32, ABI 4) and lc_check16 from host memory: the keys split
// over the context's devices (plan_devices), one host thread per device.
// Per device (HostShard, run_shard), the key offsets (and the narrow
// records' key bases) are copied first, then the records in chunks of about
// kChunkBytes on the device's copy streams (CopyPipe); the compute stream
// decides each chunk's keys with the version-order (or fused) pass as soon as
// the chunk has landed (run_device, Chunks), widening narrow records on the
// way, so the PCIe copy of chunk i + 1 overlaps the kernels of chunk i.  The
// later tiers run over the whole range once every chunk is in.  Results and
// lc_aux outputs are copied back into the caller's arrays.  Per call,
// lc_call_profile keeps where the host wall time went.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "runtime.h"

using namespace lcrt;

namespace {

// One device's slice of an lc_check call: keys [a, b) of the caller's arrays,
// records of rec bytes (48, 24 or 16) starting at src.
struct HostShard {
  lc_ctx *c;
  Dev &d;
  const lcdev::KParams &p;
  int64_t flags;
  size_t rec;               // the caller's record width
  const char *src;          // the slice's first record
  const int64_t *key_off;   // the call's offsets (key a at key_off[a])
  const int64_t *key_base;  // the narrow records' key bases, or null
  lc_key_result *out;
  const lc_aux *aux;
  int64_t a, b;
  int64_t max_len;  // the call's longest key (the widening's grid)
  bool want_wit, want_cert;
  int64_t nk = 0, r0 = 0, nrec = 0;
  size_t ops_bytes = 0;  // on the device: 48-byte records
  size_t in_bytes = 0;   // what crosses PCIe
  size_t off_bytes = 0, base_bytes = 0;
  bool pinned = false;
  // small pageable calls: inputs (offsets, bases, records) and outputs
  // (results, lc_aux arrays) through the pinned staging buffer
  bool stage = false;
  char *st_off = nullptr, *st_base = nullptr, *st_ops = nullptr, *st_out = nullptr;
  char *dst = nullptr;  // where the records land on the device
  Chunks ch;
  AuxOut ao;
  Source from;
  bool k32() const { return rec == sizeof(lc_op32); }
  bool k16() const { return rec == sizeof(lc_op16); }
  bool narrow() const { return rec != sizeof(lc_op); }  // records widened on the device, key bases
};

int shard_buffers(HostShard &s) {
  lc_ctx *c = s.c;
  Dev &d = s.d;
  const size_t nk = (size_t)s.nk, nrec = (size_t)s.nrec;
  int r = ensure(c, d.d_ops, s.ops_bytes);
  // (the narrow records' staging: d_ops32, whichever width)
  if (!r && s.narrow()) r = ensure(c, d.d_ops32, s.in_bytes);
  if (!r && s.narrow() && s.key_base) r = ensure(c, d.d_base, sizeof(int64_t) * nk);
  if (!r) r = ensure(c, d.d_off, sizeof(int64_t) * (nk + 1));
  if (!r) r = ensure(c, d.d_out, sizeof(lc_key_result) * nk);
  if (!r && s.want_wit) r = ensure(c, d.d_wit, sizeof(int32_t) * nrec);
  if (!r && s.want_wit) r = ensure(c, d.d_kind, sizeof(int32_t) * nk);
  if (!r && s.want_cert) r = ensure(c, d.d_cert, 4 * sizeof(int32_t) * nk);
  if (!r && s.want_cert) r = ensure(c, d.d_cset, sizeof(int32_t) * nrec);
  return r;
}

// Whether the call goes through the staging buffer, and where in it.
int shard_staging(HostShard &s) {
  auto up = up256;
  const size_t nk = (size_t)s.nk, nrec = (size_t)s.nrec;
  s.pinned = is_pinned(s.c, s.src, s.in_bytes);
  s.off_bytes = sizeof(int64_t) * (nk + 1);
  s.base_bytes = s.narrow() && s.key_base ? sizeof(int64_t) * nk : 0;
  const size_t out_bytes =
      up(sizeof(lc_key_result) * nk) +
      (s.want_wit ? up(sizeof(int32_t) * nrec) + up(sizeof(int32_t) * nk) : 0) +
      (s.want_cert ? up(4 * sizeof(int32_t) * nk) + up(sizeof(int32_t) * nrec) : 0);
  const size_t stage_need = up(s.off_bytes) + up(s.base_bytes) + up(s.in_bytes) + out_bytes;
  // (not with lc_aux outputs: the drop-in's C5 call with witnesses and
  // certificates measured 0.05-0.1 ms slower staged)
  s.stage = !s.pinned && !s.want_wit && !s.want_cert && stage_need <= kStageMax;
  if (!s.stage) return 0;
  if (!stage_buf(s.c, s.d)) return -ENOMEM;
  s.st_off = s.d.h_stage;
  s.st_base = s.st_off + up(s.off_bytes);
  s.st_ops = s.st_base + up(s.base_bytes);
  s.st_out = s.st_ops + up(s.in_bytes);
  return 0;
}

// The chunk plan, an event per chunk, and what the widening reads.
int shard_chunks(HostShard &s) {
  Dev &d = s.d;
  Chunks &ch = s.ch;
  plan_chunks(s.key_off + s.a, s.nk, s.rec, ch);
  while ((int)d.cev.size() < ch.n) {
    hipEvent_t e = nullptr;
    if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
      set_err(s.c, "hipEventCreateWithFlags failed");
      return -EIO;
    }
    d.cev.push_back(e);
  }
  ch.ready = d.cev.data();
  ch.max_len = s.max_len;
  if (s.k32()) ch.d_ops32 = reinterpret_cast<const lc_op32 *>(d.d_ops32.p);
  if (s.k16()) ch.d_ops16 = reinterpret_cast<const lc_op16 *>(d.d_ops32.p);
  if (s.narrow()) ch.d_base = s.key_base ? d.d_base.p : nullptr;
  s.dst = s.narrow() ? d.d_ops32.p : reinterpret_cast<char *>(d.d_ops.p);
  return 0;
}

// The key offsets (and bases) lead; the compute stream waits for the first
// chunk's event, which follows them on the copy stream.
int shard_offsets(HostShard &s) {
  lc_ctx *c = s.c;
  Dev &d = s.d;
  hipError_t e = hipEventRecord(d.eh0, d.cst);
  const void *src_off = s.key_off + s.a, *src_base = s.base_bytes ? s.key_base + s.a : nullptr;
  if (s.stage) {
    std::memcpy(s.st_off, src_off, s.off_bytes);
    if (s.base_bytes) std::memcpy(s.st_base, src_base, s.base_bytes);
    src_off = s.st_off;
    src_base = s.st_base;
  }
  if (e == hipSuccess)
    e = hipMemcpyAsync(d.d_off.p, src_off, s.off_bytes, hipMemcpyHostToDevice, d.cst);
  if (e == hipSuccess && s.base_bytes)
    e = hipMemcpyAsync(d.d_base.p, src_base, s.base_bytes, hipMemcpyHostToDevice, d.cst);
  if (e != hipSuccess) {
    set_err(c, std::string("hipMemcpyAsync H2D: ") + hipGetErrorString(e));
    return -EIO;
  }
  // the second copy stream starts behind the offsets too
  e = hipEventRecord(d.cev[0], d.cst);
  if (e == hipSuccess) e = hipStreamWaitEvent(d.cst2, d.cev[0], 0);
  if (e != hipSuccess) {
    set_err(c, std::string("hipStreamWaitEvent: ") + hipGetErrorString(e));
    return -EIO;
  }
  return 0;
}

// The record copies of one shard.  Two copy streams, chunks alternating, the
// odd ones issued by a helper thread (4 chunks or more): a copy call returns
// only once the runtime has staged (pageable) or queued it, so one issuing
// thread left the link idle between copies — two device contexts copying at
// once moved 57 GB/s against 52-53 for one thread (tools/host32_probe.py).
// The destructor stops the helper and joins it.
class CopyPipe {
 public:
  explicit CopyPipe(HostShard &s) : s_(s), issued_((size_t)s.ch.n) {
    for (auto &f : issued_) f.store(0);
    if (s.ch.n >= 4)
      helper_ = std::thread([this] {
        (void)hipSetDevice(s_.d.id);
        for (int i = 1; i < s_.ch.n && !stop_.load(std::memory_order_relaxed); i += 2)
          issued_[(size_t)i].store(copy(i) == hipSuccess ? 1 : -1, std::memory_order_release);
      });
  }
  ~CopyPipe() {
    stop_.store(true);
    if (helper_.joinable()) helper_.join();
  }

  // Chunks::issue: chunk i's copy enqueued (here, or by the helper) and its
  // event recorded; behind the last one, eh1 once both copy streams are done.
  int issue(int i) {
    Dev &d = s_.d;
    hipError_t x = hipSuccess;
    if (i % 2 == 0 || !helper_.joinable()) {
      x = copy(i);
    } else {
      int f;
      while ((f = issued_[(size_t)i].load(std::memory_order_acquire)) == 0) std::this_thread::yield();
      if (f < 0) x = hipErrorUnknown;
    }
    if (x == hipSuccess && i == s_.ch.n - 1) {
      // both copy streams done
      if (s_.ch.n > 1) x = hipStreamWaitEvent(d.cst, d.cev[(size_t)i - 1], 0);
      if (x == hipSuccess) x = hipStreamWaitEvent(d.cst, d.cev[(size_t)i], 0);
      if (x == hipSuccess) x = hipEventRecord(d.eh1, d.cst);
    }
    if (x != hipSuccess) {
      set_err(s_.c, std::string("hipMemcpyAsync H2D: ") + hipGetErrorString(x));
      return -EIO;
    }
    return 0;
  }

 private:
  hipError_t copy(int i) {
    Dev &d = s_.d;
    const size_t o = s_.rec * (size_t)s_.ch.r[i];
    const size_t bytes = s_.rec * (size_t)(s_.ch.r[i + 1] - s_.ch.r[i]);
    hipStream_t cs = i % 2 ? d.cst2 : d.cst;
    const char *from = s_.src + o;
    if (s_.stage && bytes) {
      std::memcpy(s_.st_ops + o, from, bytes);
      from = s_.st_ops + o;
    }
    hipError_t x = bytes ? hipMemcpyAsync(s_.dst + o, from, bytes, hipMemcpyHostToDevice, cs)
                         : hipSuccess;
    if (x == hipSuccess) x = hipEventRecord(d.cev[(size_t)i], cs);
    return x;
  }

  HostShard &s_;
  std::vector<std::atomic<int>> issued_;  // odd chunks: 1 issued, -1 failed
  std::atomic<bool> stop_{false};
  std::thread helper_;
};

// The tiers over the shard's keys, fed by the pipeline, then the
// certificates.  After an error the copy streams may still read the caller's
// buffer: the helper is joined, then both are waited for.
int shard_run(HostShard &s) {
  lc_ctx *c = s.c;
  Dev &d = s.d;
  Chunks &ch = s.ch;
  const int64_t nk = s.nk, max_len = s.max_len;
  s.ao.n_records = s.nrec;
  if (s.want_wit) {
    s.ao.wit = d.d_wit.p;
    s.ao.kind = d.d_kind.p;
  }
  if (s.want_cert) {
    s.ao.cert = d.d_cert.p;
    s.ao.cset = d.d_cset.p;
  }
  s.from.h_off = s.key_off + s.a;
  s.from.chunks = &ch;
  if (s.k32() && !s.want_wit && !s.want_cert && !(s.flags & LC_FLAG_NO_FAST_PATH)) {
    // decided from the 24-byte records; widened only if a key is handed over
    s.from.ops32 = ch.d_ops32;
    s.from.base32 = ch.d_base;
    s.from.widen = [c, &d, &ch, nk, max_len](const lc_op **out) -> int {
      HIP_TRY(c, lcdev::launch_widen32(ch.d_ops32, d.d_off.p, ch.d_base, nk, max_len, d.d_ops.p,
                                       d.stream));
      *out = d.d_ops.p;
      return 0;
    };
  }
  int r;
  {
    CopyPipe pipe(s);
    ch.issue = [&pipe](int i) { return pipe.issue(i); };
    r = run_device(c, d, d.d_ops.p, d.d_off.p, nk, s.p, d.d_out.p, d.stream, s.flags, s.ao, s.from);
  }  // (the helper joined)
  ch.issue = nullptr;
  if (!r) r = run_certificates(c, d, d.d_ops.p, d.d_off.p, nk, s.p, d.d_out.p, d.stream, s.ao);
  if (r) {
    (void)hipStreamSynchronize(d.cst);
    (void)hipStreamSynchronize(d.cst2);
  }
  return r;
}

// A call's outputs back to the host: straight into the caller's buffers, or
// (stage non-null) into the pinned buffer and copied out once the stream is
// done.
struct OutCopy {
  void *to;
  const void *from;
  size_t bytes;
};
hipError_t copy_outputs(const OutCopy *oc, int n, hipStream_t st, char *stage) {
  hipError_t e = hipSuccess;
  size_t so = 0;
  for (int i = 0; i < n && e == hipSuccess; i++) {
    void *to = stage ? stage + so : oc[i].to;
    so += up256(oc[i].bytes);
    e = hipMemcpyAsync(to, oc[i].from, oc[i].bytes, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess || !stage) return e;
  so = 0;
  for (int i = 0; i < n; i++) {
    std::memcpy(oc[i].to, stage + so, oc[i].bytes);
    so += up256(oc[i].bytes);
  }
  return e;
}

int shard_outputs(HostShard &s) {
  Dev &d = s.d;
  const lc_aux *aux = s.aux;
  const size_t nk = (size_t)s.nk, nrec = (size_t)s.nrec;
  OutCopy oc[5];
  int n_oc = 0;
  oc[n_oc++] = {s.out + s.a, d.d_out.p, sizeof(lc_key_result) * nk};
  if (s.want_wit && nrec) oc[n_oc++] = {aux->witness + s.r0, d.d_wit.p, sizeof(int32_t) * nrec};
  if (s.want_wit) oc[n_oc++] = {aux->witness_kind + s.a, d.d_kind.p, sizeof(int32_t) * nk};
  if (s.want_cert) oc[n_oc++] = {aux->certificate + 4 * s.a, d.d_cert.p, 4 * sizeof(int32_t) * nk};
  if (s.want_cert && aux->certificate_set && nrec)
    oc[n_oc++] = {aux->certificate_set + s.r0, d.d_cset.p, sizeof(int32_t) * nrec};
  const hipError_t e = copy_outputs(oc, n_oc, d.stream, s.st_out);
  if (e != hipSuccess) {
    set_err(s.c, std::string("hipMemcpyAsync D2H: ") + hipGetErrorString(e));
    return -EIO;
  }
  return 0;
}

// One device's share of the call, on its own thread.
int run_shard(HostShard &s) {
  Dev &d = s.d;
  const auto tw = std::chrono::steady_clock::now();
  d.last = lc_device_stats{};
  d.last.device = d.id;
  d.last.key_begin = s.a;
  d.last.key_end = s.b;
  d.kernel_ms = 0;
  s.nk = s.b - s.a;
  if (s.nk <= 0) return 0;
  if (hipSetDevice(d.id) != hipSuccess) return -EIO;
  s.r0 = s.key_off[s.a];
  s.nrec = s.key_off[s.b] - s.r0;
  s.ops_bytes = sizeof(lc_op) * (size_t)s.nrec;
  s.in_bytes = s.rec * (size_t)s.nrec;
  if (int e = shard_buffers(s)) return e;
  if (int e = shard_staging(s)) return e;
  if (int e = shard_chunks(s)) return e;
  if (int e = shard_offsets(s)) return e;
  d.last.h2d_bytes = (int64_t)(s.in_bytes + s.off_bytes + s.base_bytes);
  d.last.pinned = s.pinned;
  if (int e = shard_run(s)) return e;
  if (int e = shard_outputs(s)) return e;
  // eh1 follows the last copy on the copy stream, which the compute stream
  // waited for by the chunk's own event: it may complete a moment after the
  // stream synchronised above (several device threads on one GPU), and an
  // elapsed time read before then fails (h2d_ms would read 0)
  float hms = 0;
  if (hipEventSynchronize(d.eh1) == hipSuccess &&
      hipEventElapsedTime(&hms, d.eh0, d.eh1) == hipSuccess)
    d.last.h2d_ms = hms;
  d.last.kernel_ms = d.kernel_ms;
  d.last.total_ms = std::chrono::duration<double, std::milli>(
                        std::chrono::steady_clock::now() - tw).count();
  return 0;
}

template <class Op>
int check_host(lc_ctx *c, const Op *ops, const int64_t *key_off, const int64_t *key_base,
               int64_t n_keys, const lc_opts *opts, lc_key_result *out, const lc_aux *aux) {
  const auto t0 = std::chrono::steady_clock::now();
  auto since = [&t0]() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  };
  c->stats = lc_stats{};
  c->prof = lc_call_profile{};
  for (Dev &d : c->devs) {  // (a device without keys runs nothing)
    d.counted = lc_counted_stats{};
    d.wit = lc_witness_stats{};
    d.cwit = lc_counted_witness_stats{};
  }
  if (n_keys < 0 || (n_keys > 0 && (!ops || !key_off || !out))) {
    set_err(c, "lc_check: null buffer or negative n_keys");
    return -EINVAL;
  }
  if (n_keys == 0) return 0;
  if (int e = check_offsets(c, "lc_check", key_off, n_keys)) return e;
  lcdev::KParams p;
  int rc = opts_to_params(c, opts, &p);
  if (rc) return rc;
  const int64_t flags = opts ? opts->flags : 0;
  const bool want_wit = aux && aux->witness && aux->witness_kind;
  const bool want_cert = aux && aux->certificate;
  const int nd = (int)c->devs.size();
  c->prof.checked_ms = since();
  std::vector<int64_t> bounds(nd + 1);
  if (nd > 1) plan_devices(ops, key_off, n_keys, nd, bounds.data());
  else bounds[0] = 0, bounds[1] = n_keys;
  c->prof.planned_ms = since();
  // the longest key (the widening's grid); C4's 5,000-op key takes more
  // workgroups than a C2 key
  int64_t max_len = 0;
  if (sizeof(Op) != sizeof(lc_op))
    for (int64_t k = 0; k < n_keys; k++) max_len = std::max(max_len, key_off[k + 1] - key_off[k]);

  std::vector<int> rcs(nd, 0);
  std::vector<int> nchunks(nd, 0);
  auto work = [&](int di) {
    Dev &d = c->devs[di];
    d.t_start = since();
    d.t_end = d.t_start;
    const int64_t a = bounds[di], b = bounds[di + 1];
    HostShard s{c, d, p, flags, sizeof(Op), reinterpret_cast<const char *>(ops + key_off[a]),
                key_off, sizeof(Op) != sizeof(lc_op) ? key_base : nullptr, out, aux, a, b, max_len,
                want_wit, want_cert};
    rcs[di] = run_shard(s);
    nchunks[di] = s.ch.n;
    if (!rcs[di] && b > a) d.t_end = since();
  };
  if (nd == 1) {
    work(0);
  } else {
    std::vector<std::thread> th;
    for (int di = 0; di < nd; di++) th.emplace_back(work, di);
    for (auto &t : th) t.join();
  }
  c->prof.first_start_ms = c->prof.first_end_ms = 1e300;
  for (int di = 0; di < nd; di++) {
    const Dev &d = c->devs[di];
    if (rcs[di] && !rc) rc = rcs[di];
    fill_stats(c->stats, d);
    c->prof.first_start_ms = std::min(c->prof.first_start_ms, d.t_start);
    c->prof.last_start_ms = std::max(c->prof.last_start_ms, d.t_start);
    c->prof.first_end_ms = std::min(c->prof.first_end_ms, d.t_end);
    c->prof.last_end_ms = std::max(c->prof.last_end_ms, d.t_end);
    c->prof.n_chunks += nchunks[di];
  }
  c->prof.joined_ms = since();
  if (!rc && (flags & LC_FLAG_WHOLE_GPU)) {
    std::vector<int64_t> todo, todo_w;
    unknown_keys(out, n_keys, todo, todo_w);
    auto fetch = [&](int64_t k, std::vector<lc_op> &v) {
      v.resize((size_t)(key_off[k + 1] - key_off[k]));
      const int64_t base = key_base ? key_base[k] : 0;
      for (size_t i = 0; i < v.size(); i++) v[i] = widen_op(ops[key_off[k] + (int64_t)i], base);
      return 0;
    };
    auto store = [&](int64_t k, const lc_key_result &r) {
      out[k] = r;
      // re-decided by the frontier exchange: no certificate (cert.hip covers
      // the tiers' decisions)
      if (want_cert)
        for (int j = 0; j < 4; j++) aux->certificate[4 * k + j] = j == 0 ? LC_CERT_NONE : j < 3 ? -1 : 0;
      return 0;
    };
    rc = whole_gpu(c, todo, opts, fetch, store);
    if (!rc) rc = whole_gpu(c, todo_w, opts, fetch, store);
  }
  c->prof.whole_gpu_ms = since();
  c->stats.n_keys = n_keys;
  c->stats.n_ops = key_off[n_keys] - key_off[0];
  c->stats.n_devices = nd;
  c->stats.total_ms = since();
  c->prof.total_ms = c->stats.total_ms;
  c->prof.n_devices = nd;
  return rc;
}

}  // namespace

extern "C" {

int lc_check_ex(lc_ctx *c, const lc_op *ops, const int64_t *key_off,
                int64_t n_keys, const lc_opts *opts, lc_key_result *out, const lc_aux *aux) {
  if (!c) return -EINVAL;
  return check_host(c, ops, key_off, nullptr, n_keys, opts, out, aux);
}

int lc_check(lc_ctx *c, const lc_op *ops, const int64_t *key_off,
             int64_t n_keys, const lc_opts *opts, lc_key_result *out) {
  return lc_check_ex(c, ops, key_off, n_keys, opts, out, nullptr);
}

int lc_check32(lc_ctx *c, const lc_op32 *ops, const int64_t *key_off, const int64_t *key_base,
               int64_t n_keys, const lc_opts *opts, lc_key_result *out, const lc_aux *aux) {
  if (!c) return -EINVAL;
  if (reinterpret_cast<uintptr_t>(ops) % 4) {
    set_err(c, "lc_check32: ops must be 4-byte aligned");
    return -EINVAL;
  }
  return check_host(c, ops, key_off, key_base, n_keys, opts, out, aux);
}

int lc_check16(lc_ctx *c, const lc_op16 *ops, const int64_t *key_off, const int64_t *key_base,
               int64_t n_keys, const lc_opts *opts, lc_key_result *out, const lc_aux *aux) {
  if (!c) return -EINVAL;
  if (reinterpret_cast<uintptr_t>(ops) % 4) {
    set_err(c, "lc_check16: ops must be 4-byte aligned");
    return -EINVAL;
  }
  return check_host(c, ops, key_off, key_base, n_keys, opts, out, aux);
}

}  // extern "C"
