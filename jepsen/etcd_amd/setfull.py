"""jepsen.checker/set-full on the device (include/lincheck_setfull.h).

`encode` makes lc_set_full's three flat arrays from Jepsen op maps in one pass
(the header's rules 1, 2 and 9); `SetFullChecker` is the drop-in for
`(checker/set-full {:linearizable? true})` as set.clj:46 and lock.clj:258 /
:265 build it: `.check(test, history, opts)` returns jepsen's result map.
The rules are a re-derivation of jepsen 0.3.x's set-full; parity with jepsen
itself is unpinned.

The Clojure shim and the native EDN reader do not reach this checker yet.
"""
import math
from collections import namedtuple

import numpy as np

from . import abi, history as H

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
UNKNOWN = "unknown"
OUTCOMES = {abi.LC_SF_NEVER_READ: "never-read", abi.LC_SF_STABLE: "stable", abi.LC_SF_LOST: "lost"}
LATENCY_POINTS = (0, 0.5, 0.95, 0.99, 1)
WORST_STALE = 8


class Unsupported(ValueError):
    """The history cannot be written as lc_set_full's arrays (rule 9: two add
    invokes of one value, an add or read op map without :time)."""


# adds / reads: abi.SF_ADD_DTYPE / SF_READ_DTYPE arrays; values: the payloads,
# int64; index: position -> op["index"] where present, else the position;
# elements: the adds' :value in add order (values holds them as they are when
# every element and payload entry is an integer, and interned ids otherwise);
# n_orphan_reads: :ok reads without a pending invoke (ignored)
Encoded = namedtuple("Encoded", "adds reads values index elements n_orphan_reads")


def _is_int(v):
    return type(v) is int and INT64_MIN < v <= INT64_MAX


def _key(v):
    """What makes two :value the same element (history.Interner's equality)."""
    return (type(v).__name__, v) if not isinstance(v, (list, dict, set)) else repr(v)


def _time(op, pos):
    t = op.get("time")
    if type(t) is not int:
        raise Unsupported("op %d has no integer :time" % pos)
    return t


def encode(history):
    """One pass over the op maps -> Encoded."""
    n = len(history)
    index = np.arange(n, dtype=np.int64)
    elements, element_of = [], {}   # :value in add order; _key -> element number
    add_rows = []                   # [inv_pos, ok_pos, ok_time]
    pending = {}                    # process -> (position, time) of its pending read invoke
    read_rows, payloads = [], []    # (inv_time, ok_time, inv_pos, ok_pos); the payload as a list
    orphans = 0
    for pos, op in enumerate(history):
        if "index" in op:
            index[pos] = op["index"]
        if not H.is_client(op):
            continue
        f, t = H._kw(op.get("f")), H._kw(op.get("type"))
        if f == "add":
            k = _key(op.get("value"))
            if t == "invoke":
                _time(op, pos)
                if k in element_of:
                    raise Unsupported("op %d: a second add invoke of %r" % (pos, op.get("value")))
                element_of[k] = len(elements)
                elements.append(op.get("value"))
                add_rows.append([pos, -1, 0])
            elif t == "ok":
                e = element_of.get(k)
                if e is not None and add_rows[e][1] < 0:  # (an add :ok of no element: ignored)
                    add_rows[e][1:] = [pos, _time(op, pos)]
        elif f == "read":
            p = op["process"]
            if t == "invoke":
                pending[p] = (pos, _time(op, pos))
            elif t == "fail":
                pending.pop(p, None)
            elif t == "ok":
                inv = pending.get(p)
                if inv is None:
                    orphans += 1
                    continue
                v = op.get("value")
                read_rows.append((inv[1], _time(op, pos), inv[0], pos))
                payloads.append([] if v is None else list(v))
    as_is = all(_is_int(v) for v in elements) and \
        all(set(map(type, pl)) <= {int} and all(INT64_MIN < x <= INT64_MAX for x in pl)
            for pl in payloads)
    if as_is:
        ids = elements
    else:  # elements are 0 .. E-1; a payload entry that names none gets an id of its own
        intern = dict(element_of)
        ids = list(range(len(elements)))
        payloads = [[intern.setdefault(_key(x), len(intern)) for x in pl] for pl in payloads]
    adds = np.zeros(len(elements), dtype=abi.SF_ADD_DTYPE)
    if len(elements):
        rows = np.array(add_rows, dtype=np.int64)
        adds["value"] = np.array(ids, dtype=np.int64)
        adds["inv_pos"], adds["ok_pos"], adds["ok_time"] = rows[:, 0], rows[:, 1], rows[:, 2]
    reads = np.zeros(len(read_rows), dtype=abi.SF_READ_DTYPE)
    if len(read_rows):
        rows = np.array(read_rows, dtype=np.int64)
        reads["inv_time"], reads["ok_time"] = rows[:, 0], rows[:, 1]
        reads["inv_pos"], reads["ok_pos"] = rows[:, 2], rows[:, 3]
        lens = np.array([len(pl) for pl in payloads], dtype=np.int64)
        reads["len"] = lens
        reads["off"] = np.cumsum(lens) - lens
    values = np.array([x for pl in payloads for x in pl], dtype=np.int64)
    return Encoded(adds, reads, values, index, elements, orphans)


def _sorted(xs):
    try:
        return sorted(xs)
    except TypeError:
        return sorted(xs, key=repr)


def latency_points(latencies):
    """jepsen's frequency-distribution: {point: nth(sorted, min(n - 1, floor(n * point)))},
    None without latencies."""
    s = sorted(latencies)
    n = len(s)
    if not n:
        return None
    return {p: s[min(n - 1, int(math.floor(n * p)))] for p in LATENCY_POINTS}


def result_map(history, enc, out, summary):
    """jepsen's set-full result map from the library's element records."""
    valid = {1: True, 0: False}.get(int(summary["valid"]), UNKNOWN)
    outcome, flags = out["outcome"], out["flags"]

    def named(mask):
        return _sorted([enc.elements[e] for e in np.nonzero(mask)[0]])

    def opt(x):
        return None if x < 0 else int(x)

    stale = np.nonzero(flags & abi.LC_SF_STALE)[0]
    worst = sorted(stale.tolist(), key=lambda e: (-int(out["stable_latency_ms"][e]), e))[:WORST_STALE]
    dup = np.nonzero(flags & abi.LC_SF_DUPLICATED)[0]
    return {
        "valid?": valid,
        "attempt-count": len(out),
        "stable-count": int(summary["n_stable"]),
        "lost-count": int(summary["n_lost"]),
        "lost": named(outcome == abi.LC_SF_LOST),
        "never-read-count": int(summary["n_never_read"]),
        "never-read": named(outcome == abi.LC_SF_NEVER_READ),
        "stale-count": int(summary["n_stale"]),
        "stale": named((flags & abi.LC_SF_STALE) != 0),
        "worst-stale": [{
            "element": enc.elements[e],
            "outcome": OUTCOMES[int(outcome[e])],
            "stable-latency": opt(out["stable_latency_ms"][e]),
            "lost-latency": opt(out["lost_latency_ms"][e]),
            "known": history[out["known_pos"][e]] if out["known_pos"][e] >= 0 else None,
            "last-absent": history[out["last_absent"][e]] if out["last_absent"][e] >= 0 else None,
        } for e in worst],
        "stable-latencies": latency_points(
            out["stable_latency_ms"][outcome == abi.LC_SF_STABLE].tolist()),
        "lost-latencies": latency_points(out["lost_latency_ms"][outcome == abi.LC_SF_LOST].tolist()),
        "duplicated-count": int(summary["n_duplicated"]),
        "duplicated": {_hashable(enc.elements[e]): int(out["dup_max"][e]) for e in dup},
        "phantom-count": int(summary["n_phantom"]),
        "orphan-read-count": enc.n_orphan_reads,
    }


def _hashable(v):
    return v if not isinstance(v, (list, dict, set)) else repr(v)


class SetFullChecker:
    """Drop-in for `(checker/set-full {:linearizable? linearizable})`.

    device=True decides on the first GPU of device_mask (lc_set_full: the
    library must have it; there is no quiet fallback); device=False uses
    lc_set_full_host and needs no GPU.  checker.check_safe works on it as on
    every checker here.
    """

    def __init__(self, linearizable=True, device_mask=0, device=True):
        self.linearizable = bool(linearizable)
        self.device_mask = device_mask
        self.device = device
        self._ctx = None
        self.last_summary = None  # the library's lc_sf_summary of the last check, as a dict

    def _context(self):
        if self._ctx is None:
            self._ctx = abi.Context(self.device_mask)
        return self._ctx

    def close(self):
        if self._ctx is not None:
            self._ctx.close()
            self._ctx = None

    def check(self, test, history, opts=None):
        history = list(history)
        enc = encode(history)
        if self.device:
            out, s = self._context().set_full(enc.adds, enc.reads, enc.values, self.linearizable)
        else:
            out, s = abi.set_full_host(enc.adds, enc.reads, enc.values, self.linearizable)
        self.last_summary = s
        return result_map(history, enc, out, s)
