"""jepsen.checker/stats and the data of jepsen.checker/perf on the device
(include/lincheck_perf.h), and the `checker/compose` of etcd.clj:129-141 for
the keys this library answers.

`encode` makes lc_perf_stats' 16-byte records from Jepsen op maps in one pass.
`StatsChecker` is the drop-in for `(checker/stats)`; `PerfChecker` returns the
data behind `(checker/perf)`'s three graphs (the latency points, the latency
quantiles and the rate per time bucket) — rendering them is gnuplot's business
and out of scope.  `compose` merges checkers' results as jepsen does.  The
rules are a re-derivation of jepsen 0.3.x; parity with jepsen itself is
unpinned.  `:clock`, `:exceptions` and `:crash` of the composed
checker are not arithmetic on client ops and are not here.

The Clojure shim and the native EDN reader do not reach these checkers yet.
"""
import numpy as np

from . import abi, dist, history as H
from .checker import UNKNOWN, check_safe
from .setfull import Unsupported

TYPES = {"invoke": abi.LC_EV_INVOKE, "ok": abi.LC_EV_OK, "fail": abi.LC_EV_FAIL, "info": abi.LC_EV_INFO}
TYPE_NAMES = {v: k for k, v in TYPES.items()}
NS_PER_S, NS_PER_MS = 10 ** 9, 10 ** 6


def encode(history):
    """One pass over the op maps -> (events, f_names): an abi.PS_EVENT_DTYPE
    array, one record per op map, and the :f values in the order of their ids.
    An op map whose :process is no integer is a non-client event (process -1);
    Unsupported is raised for an op map without an integer :time or with an
    unknown :type."""
    history = list(history)
    events = np.zeros(len(history), dtype=abi.PS_EVENT_DTYPE)
    ids, f_names = {}, []
    for pos, op in enumerate(history):
        t = op.get("time")
        if type(t) is not int:
            raise Unsupported("op %d has no integer :time" % pos)
        ty = TYPES.get(H._kw(op.get("type")))
        if ty is None:
            raise Unsupported("op %d has the unknown :type %r" % (pos, op.get("type")))
        f = H._kw(op.get("f"))
        client = H.is_client(op) and 0 <= op["process"] < 2 ** 31
        if client and f not in ids:
            if len(f_names) >= 65536:
                raise Unsupported("more than 65,536 different :f")
            ids[f] = len(f_names)
            f_names.append(f)
        events[pos] = (t, op["process"] if client else -1, ids[f] if client else 0, ty, 0)
    return events, f_names


def _run(ctx_of, device, events, n_f, **kw):
    if device:
        return ctx_of().perf_stats(events, n_f, **kw)
    return abi.perf_stats_host(events, n_f, **kw)


class _Checker:
    """device=True computes on the first GPU of ctx (an abi.Context; None: one
    of its own over device_mask, opened at the first check) with lc_perf_stats:
    the library must have it, there is no quiet fallback; device=False uses
    lc_perf_stats_host and needs no GPU."""

    def __init__(self, ctx=None, device=True, device_mask=0):
        self.device, self.device_mask = device, device_mask
        self._ctx, self._own = ctx, False
        self.last_summary = None  # the library's lc_ps_summary of the last check, as a dict

    def _context(self):
        if self._ctx is None:
            self._ctx, self._own = abi.Context(self.device_mask), True
        return self._ctx

    def close(self):
        if self._own and self._ctx is not None:
            self._ctx.close()
        self._ctx, self._own = None, False


class StatsChecker(_Checker):
    """Drop-in for `(checker/stats)`: valid? is False as soon as some :f never
    got an :ok."""

    def check(self, test, history, opts=None):
        events, f_names = encode(history)
        out, s = _run(self._context, self.device, events, max(len(f_names), 1), qs=(), points=False)
        self.last_summary = s

        def row(count, ok, fail, info):
            return {"valid?": bool(ok > 0), "count": int(count), "ok-count": int(ok), "fail-count": int(fail),
                    "info-count": int(info)}

        by_f = {f: row(*out["by_f"][i]) for i, f in enumerate(f_names) if out["by_f"][i][0] > 0}
        total = row(s["count"], s["ok"], s["fail"], s["info"])
        total["valid?"] = bool(s["valid"])
        total["by-f"] = by_f
        return total


class PerfChecker(_Checker):
    """The data of `(checker/perf)`'s graphs; valid? is always True.  Times
    are the buckets' midpoints in seconds, latencies milliseconds, rates
    hertz; `latencies` (the point graph: per f and completion type, [invoke
    time s, latency ms] in history order) only with points=True."""

    def __init__(self, ctx=None, device=True, device_mask=0, qs=abi.PS_DEFAULT_QS,
                 rate_dt_ns=abi.PS_DEFAULT_RATE_DT_NS, quant_dt_ns=abi.PS_DEFAULT_QUANT_DT_NS, points=False):
        super().__init__(ctx, device, device_mask)
        self.qs, self.rate_dt_ns, self.quant_dt_ns, self.points = tuple(qs), rate_dt_ns, quant_dt_ns, points

    def check(self, test, history, opts=None):
        events, f_names = encode(history)
        out, s = _run(self._context, self.device, events, max(len(f_names), 1), qs=self.qs,
                      rate_dt_ns=self.rate_dt_ns, quant_dt_ns=self.quant_dt_ns, points=self.points)
        self.last_summary = s
        quantiles, rate = {}, {}
        for i, f in enumerate(f_names):
            buckets = np.nonzero(out["quant_n"][i])[0]
            if len(buckets):
                quantiles[f] = {q: [[(b + 0.5) * self.quant_dt_ns / NS_PER_S, int(out["quant"][i, b, k]) / NS_PER_MS]
                                    for b in buckets] for k, q in enumerate(self.qs)}
            for t in (abi.LC_EV_OK, abi.LC_EV_FAIL, abi.LC_EV_INFO):
                buckets = np.nonzero(out["rate"][i, t - 1])[0]
                if len(buckets):
                    rate.setdefault(f, {})[TYPE_NAMES[t]] = [
                        [(b + 0.5) * self.rate_dt_ns / NS_PER_S, int(out["rate"][i, t - 1, b]) * NS_PER_S / self.rate_dt_ns]
                        for b in buckets]
        res = {"valid?": True, "latency-quantiles": quantiles, "rate": rate}
        if self.points:
            lat = {}
            for pos in np.nonzero(out["comp_pos"] >= 0)[0]:
                comp = int(out["comp_pos"][pos])
                lat.setdefault(f_names[events["f"][pos]], {}).setdefault(TYPE_NAMES[int(events["type"][comp])], []).append(
                    [int(events["time"][pos]) / NS_PER_S, int(out["latency_ns"][pos]) / NS_PER_MS])
            res["latencies"] = lat
        for k in ("n_events", "n_client", "n_pairs", "n_pending", "n_ignored_completions", "n_mismatched_f",
                  "t_max", "n_rate_buckets", "n_quant_buckets"):
            res[k.replace("_", "-")] = int(s[k])
        return res


def _verdict(valid):
    """A result map's valid? as the verdict code dist.merge_verdicts merges."""
    return abi.LC_VALID if valid is True else abi.LC_INVALID if valid is False else abi.LC_UNKNOWN


class compose:
    """`(checker/compose {name checker ...})`: every checker on the same
    history, each through check_safe (one that raises gives {"valid?":
    "unknown", "error": ...} for its key); the result is {name: result, ...,
    "valid?": merged}, merged as false over unknown over true
    (dist.merge_verdicts, jepsen's merge-valid)."""

    def __init__(self, checkers):
        self.checkers = dict(checkers)

    def check(self, test, history, opts=None):
        history = list(history)
        res = {name: check_safe(ch, test, history, opts) for name, ch in self.checkers.items()}
        res["valid?"] = dist.merge_verdicts([_verdict(r.get("valid?")) for r in res.values()])
        return res
