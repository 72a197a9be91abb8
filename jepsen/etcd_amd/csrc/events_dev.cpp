// events_dev.cpp — the driver of lc_events_pack / lc_check_events
// (include/lincheck_events.h): the events copied to the context's first
// device and split, completed and packed there (events.hip); lc_check_events
// then checks the packed records where they lie, through lc_check_device32's
// path (lincheck.cpp, check_device).
#include <chrono>
#include <string>

#include "runtime.h"

using namespace lcrt;

namespace {

// On return the stream has drained, the pinned words hold the call's counts, and
// the records are in s.w's ops32 / completion / key_off / key_base.
int events_device(lc_ctx *c, const char *who, const lc_event *ev, int64_t n_events, int64_t n_keys) {
  const std::string name(who);
  EvState &s = c->evs;
  s.stats = lc_events_stats{};
  if (n_events < 0 || n_keys < 0 || (n_events > 0 && !ev)) {
    set_err(c, name + ": null events or a negative count");
    return -EINVAL;
  }
  if (n_events >= (int64_t(1) << 31) || n_keys >= (int64_t(1) << 31)) {
    set_err(c, name + ": 2^31 or more events or keys");
    return -EINVAL;
  }
  hipStream_t st;
  if (int e = side_begin(c, s, 3, sizeof(lcev::Status), &st)) return e;
  const hipEvent_t e0 = s.ev[0], e1 = s.ev[1], e2 = s.ev[2];
  lcev::Status *h_status = s.words<lcev::Status>();
  const size_t n = (size_t)n_events, k = (size_t)n_keys;
  lcev::Ws &w = s.w;
  w = lcev::Ws{};
  w.n = n_events;
  w.k = n_keys;
  auto layout = [&](Carver ws) {
    w.ev = ws.take<lc_event>(n);
    w.cnt = ws.take<int32_t>(k);
    w.cursor = ws.take<int32_t>(k);
    w.seg_off = ws.take<int64_t>(k + 1);
    w.seg = ws.take<uint32_t>(n);
    w.match = ws.take<int32_t>(n);
    w.gtab = ws.take<unsigned long long>(2 * n);
    w.nops = ws.take<int32_t>(k);
    w.nfail = ws.take<int32_t>(k);
    w.nign = ws.take<int32_t>(k);
    w.key_off = ws.take<int64_t>(k + 1);
    w.key_base = ws.take<int64_t>(k);
    w.ops32 = ws.take<lc_op32>(n);
    w.completion = ws.take<int32_t>(n);
    w.status = ws.take<lcev::Status>(1);
    return ws.size;
  };
  if (int e = ensure(c, s.arena, layout(Carver{}))) return e;
  layout(Carver{s.arena.p});
  HIP_TRY(c, hipEventRecord(e0, st));
  if (n) HIP_TRY(c, hipMemcpyAsync(writable(w.ev), ev, sizeof(lc_event) * n, hipMemcpyHostToDevice, st));
  HIP_TRY(c, hipEventRecord(e1, st));
  // no counter of an earlier call, larger or smaller, survives
  HIP_TRY(c, hipMemsetAsync(w.status, 0, sizeof(lcev::Status), st));
  if (k > 1) {
    HIP_TRY(c, hipMemsetAsync(w.cnt, 0, sizeof(int32_t) * k, st));
    HIP_TRY(c, hipMemsetAsync(w.cursor, 0, sizeof(int32_t) * k, st));
  }
  HIP_TRY(c, lcev::launch_events(w, st));
  HIP_TRY(c, hipEventRecord(e2, st));
  HIP_TRY(c, hipMemcpyAsync(h_status, w.status, sizeof(lcev::Status), hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  s.stats.h2d_ms = elapsed_ms(e0, e1);
  s.stats.split_ms = elapsed_ms(e1, e2);
  const lcev::Status &h = *s.words<lcev::Status>();
  s.stats.n_events = n_events;
  s.stats.n_client = h.n_client;
  s.stats.n_ops = h.n_ops;
  s.stats.n_fail_pairs = h.n_fail;
  s.stats.n_ignored_completions = h.n_ignored;
  s.stats.n_big_keys = h.n_big;
  if (h.err) {
    set_err(c, name + ": an event with a key outside [-1, n_keys) or a type above 3 (the last one at position " +
                   std::to_string(h.err_pos) + ")");
    return -EINVAL;
  }
  return 0;
}

// The packed records of the last events_device call into the caller's arrays.
int events_copy_out(lc_ctx *c, const char *who, int64_t n_keys, lc_events_out *out) {
  EvState &s = c->evs;
  const lcev::Status &h = *s.words<lcev::Status>();
  if (!out->key_off || (n_keys > 0 && !out->key_base) || out->cap < h.n_invoke ||
      (h.n_ops > 0 && (!out->ops32 || !out->completion))) {
    set_err(c, std::string(who) + ": lc_events_out: a null array, or cap below the number of invokes");
    return -EINVAL;
  }
  hipStream_t st = c->devs[0].stream;
  const size_t k = (size_t)n_keys, m = (size_t)h.n_ops;
  if (m) {
    HIP_TRY(c, hipMemcpyAsync(out->ops32, s.w.ops32, sizeof(lc_op32) * m, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(out->completion, s.w.completion, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipMemcpyAsync(out->key_off, s.w.key_off, sizeof(int64_t) * (k + 1), hipMemcpyDeviceToHost, st));
  if (k) HIP_TRY(c, hipMemcpyAsync(out->key_base, s.w.key_base, sizeof(int64_t) * k, hipMemcpyDeviceToHost, st));
  HIP_TRY(c, hipStreamSynchronize(st));
  out->n_ops = h.n_ops;
  return 0;
}

// lc_check_events after events_device: the records, resident, through
// lc_check_device32's path; results and lc_aux outputs copied to the host.
// (Nothing here grows s.arena, where the records are: d_res and the lc_aux
// outputs have buffers of their own.)
int events_check(lc_ctx *c, int64_t n_keys, const lc_opts *opts, lc_key_result *out, const lc_aux *aux) {
  EvState &s = c->evs;
  Dev &d = c->devs[0];
  if (n_keys == 0) return 0;
  if (!out) {
    set_err(c, "lc_check_events: null out");
    return -EINVAL;
  }
  const size_t k = (size_t)n_keys, m = (size_t)s.words<lcev::Status>()->n_ops;
  const bool want_wit = aux && aux->witness && aux->witness_kind;
  const bool want_cert = aux && aux->certificate;
  if (aux && (aux->witness || aux->certificate) && !(aux->witness && aux->witness_kind)) {
    set_err(c, "lc_check_events: lc_aux needs witness and witness_kind");
    return -EINVAL;
  }
  int e = ensure(c, s.d_res, sizeof(lc_key_result) * k);
  if (!e && want_wit) e = ensure(c, d.d_wit, sizeof(int32_t) * m);
  if (!e && want_wit) e = ensure(c, d.d_kind, sizeof(int32_t) * k);
  if (!e && want_cert) e = ensure(c, d.d_cert, 4 * sizeof(int32_t) * k);
  if (!e && want_cert) e = ensure(c, d.d_cset, sizeof(int32_t) * m);
  if (e) return e;
  lc_aux dev_aux{};
  if (want_wit) {
    dev_aux.witness = d.d_wit.p;
    dev_aux.witness_kind = d.d_kind.p;
  }
  if (want_cert) {
    dev_aux.certificate = d.d_cert.p;
    dev_aux.certificate_set = d.d_cset.p;
  }
  e = check_device(c, "lc_check_events", s.w.ops32, true, s.w.key_off, s.w.key_base, n_keys, opts, s.d_res.p,
                   nullptr, want_wit ? &dev_aux : nullptr);
  if (e) return e;
  hipStream_t st = d.stream;
  HIP_TRY(c, hipMemcpyAsync(out, s.d_res.p, sizeof(lc_key_result) * k, hipMemcpyDeviceToHost, st));
  if (want_wit) {
    if (m)
      HIP_TRY(c, hipMemcpyAsync(aux->witness, d.d_wit.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
    HIP_TRY(c, hipMemcpyAsync(aux->witness_kind, d.d_kind.p, sizeof(int32_t) * k, hipMemcpyDeviceToHost, st));
  }
  if (want_cert) {
    HIP_TRY(c, hipMemcpyAsync(aux->certificate, d.d_cert.p, 4 * sizeof(int32_t) * k, hipMemcpyDeviceToHost, st));
    if (m && aux->certificate_set)
      HIP_TRY(c, hipMemcpyAsync(aux->certificate_set, d.d_cset.p, sizeof(int32_t) * m, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(c, hipStreamSynchronize(st));
  return 0;
}

}  // namespace

void lcrt::release(EvState &s) {
  if (s.d_res.p) (void)hipFree(s.d_res.p);
  release(static_cast<SideState &>(s));
}

extern "C" {

int lc_events_pack(lc_ctx *c, const lc_event *ev, int64_t n_events, int64_t n_keys, lc_events_out *out) {
  if (!c) return -EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  if (!out) {
    set_err(c, "lc_events_pack: null out");
    return -EINVAL;
  }
  int rc = events_device(c, "lc_events_pack", ev, n_events, n_keys);
  if (!rc) rc = events_copy_out(c, "lc_events_pack", n_keys, out);
  c->evs.stats.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return rc;
}

int lc_check_events(lc_ctx *c, const lc_event *ev, int64_t n_events, int64_t n_keys, const lc_opts *opts,
                    lc_key_result *out, const lc_aux *aux, lc_events_out *packed) {
  if (!c) return -EINVAL;
  const auto t0 = std::chrono::steady_clock::now();
  auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
  int rc = events_device(c, "lc_check_events", ev, n_events, n_keys);
  if (!rc && packed) rc = events_copy_out(c, "lc_check_events", n_keys, packed);
  const double t1 = ms();
  if (!rc) rc = events_check(c, n_keys, opts, out, aux);
  c->evs.stats.check_ms = ms() - t1;
  c->evs.stats.total_ms = ms();
  return rc;
}

int lc_last_events_stats(lc_ctx *c, lc_events_stats *out) {
  if (!c || !out) return -EINVAL;
  *out = c->evs.stats;
  return 0;
}

}  // extern "C"
