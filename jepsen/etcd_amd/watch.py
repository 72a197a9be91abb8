"""The :watch workload's checker: every thread's watch log must be the same
sequence, with the logs hashed, compared and diffed on the device
(include/lincheck_watch.h).

`encode` makes lc_watch_check's flat arrays from Jepsen op maps in one pass;
`WatchChecker` stands where the reference's `watch` workload puts its
`(checker)`: `.check(test, history, opts)` returns the reference's result map
with string keys, `{"valid?", "revisions"}` and, when `valid?` is false,
`{"logs", "canonical", "deltas", "nonmonotonic-errors"}` (in the reference
`(not :unknown)` is false, so an unknown result has only the first two).
The rules re-derive the checker of watch.clj and what is known of clj-diff;
parity with them is unpinned.  Which of several equally common
(or equally long) logs is called canonical, and the order of deltas of one edit
distance, are ours: the reference leaves both to a hash map's order.  A delta's
"diff" is built from the library's edit script in clj-diff's shape, `{"+":
[[index, item, ...], ...], "-": [index, ...]}`, insertions grouped by the index
of the canonical log after which they go (-1: the front); above the cap max_d
(lc_watch_limits) a delta keeps its exact "edit-distance", its "diff" is None
and "diff-omitted" is True.

Op maps may have string or keyword (":type") keys and values.  The Clojure shim
and the EDN reader's CLI do not reach this checker yet.
"""
from collections import namedtuple

import numpy as np

from . import abi, history as H
from .append import UNKNOWN, Unsupported, _ident

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1

# threads: abi.WT_THREAD_DTYPE; values: int64, the logs back to back in the
# threads' order; nonmonotonic: the second elements of rule 8's errors;
# elements: what the ids stand for (None: the history's own integers)
Encoded = namedtuple("Encoded", "threads values nonmonotonic elements")


def _get(m, name, default=None):
    """m[name] under a string or a keyword key."""
    if name in m:
        return m[name]
    return m.get(":" + name, default)


def _is_i64(v):
    return type(v) is int and INT64_MIN <= v <= INT64_MAX


def encode(history, concurrency):
    """Rules 1 and 8 over the op maps -> Encoded.  Threads come in order of
    their first watch op."""
    logs, revs, nonmono = {}, {}, []
    for pos, op in enumerate(history):
        err = _get(op, "error")
        if isinstance(err, (list, tuple)) and err and H._kw(err[0]) == "nonmonotonic-watch":
            nonmono.append(err[1] if len(err) > 1 else None)
        if H._kw(_get(op, "type")) != "ok" or H._kw(_get(op, "f")) not in ("watch", "final-watch"):
            continue
        v = _get(op, "value")
        log = _get(v, "log") if isinstance(v, dict) else None
        if not isinstance(log, (list, tuple)):
            raise Unsupported("op %d: an :ok watch without a :log" % pos)
        t = _get(op, "process") % concurrency
        logs.setdefault(t, []).extend(log)
        rev = _get(v, "revision")
        revs[t] = max(revs.get(t, 0), 0 if rev is None else rev)
    every = [x for log in logs.values() for x in log]
    ids = None
    if not all(_is_i64(x) for x in every):
        ids = {}
        for x in every:
            ids.setdefault(_ident(x), (len(ids), x))
    threads = np.zeros(len(logs), dtype=abi.WT_THREAD_DTYPE)
    off = 0
    for i, (t, log) in enumerate(logs.items()):
        threads[i] = (off, len(log), revs[t], t)
        off += len(log)
    values = np.array(every if ids is None else [ids[_ident(x)][0] for x in every], dtype=np.int64).reshape(-1)
    return Encoded(threads, values, nonmono, None if ids is None else [x for _, x in ids.values()])


def diff_of(script):
    """An edit script (abi.WT_EDIT_DTYPE rows in path order, values already
    named) as clj-diff's map."""
    plus, minus = [], []
    for at, value, op in script:
        if op == abi.LC_WT_DELETE:
            minus.append(at)
        elif plus and plus[-1][0] == at - 1:
            plus[-1].append(value)
        else:
            plus.append([at - 1, value])
    return {"+": plus, "-": minus}


class WatchChecker:
    """check(test, history, opts) -> the reference checker's map.  test: a
    mapping with "concurrency" (or ":concurrency").  use_gpu False, or no GPU
    context given and none wanted, runs lc_watch_check_host."""

    def __init__(self, ctx=None, use_gpu=True):
        self.ctx, self.use_gpu = ctx, use_gpu
        self.last_summary = None

    def _run(self, enc):
        n = len(enc.nonmonotonic)
        if self.use_gpu and self.ctx is not None:
            return self.ctx.watch_check(enc.threads, enc.values, n)
        if self.use_gpu:
            with abi.Context(device_mask=1) as ctx:
                return ctx.watch_check(enc.threads, enc.values, n)
        return abi.watch_check_host(enc.threads, enc.values, n)

    def check(self, test, history, opts=None):
        enc = encode(history, _get(test, "concurrency"))
        out, s = self._run(enc)
        self.last_summary = s
        name = (lambda v: int(v)) if enc.elements is None else (lambda v: enc.elements[int(v)])
        log_of = lambda i: [name(v) for v in  # noqa: E731
                            enc.values[int(enc.threads[i]["off"]):int(enc.threads[i]["off"] + enc.threads[i]["len"])]]
        tid = lambda i: int(enc.threads[i]["thread"])  # noqa: E731
        valid = {1: True, 0: False, -1: UNKNOWN}[s["valid"]]
        res = {"valid?": valid, "revisions": {tid(i): int(enc.threads[i]["revision"]) for i in range(len(enc.threads))}}
        if valid is not False:
            return res
        deltas = []
        for d in out["deltas"]:
            rec = {"thread": tid(int(d["thread"])), "edit-distance": int(d["edit_distance"])}
            if d["flags"] & abi.LC_WT_NO_SCRIPT:
                rec["diff"], rec["diff-omitted"] = None, True
            else:
                sc = out["edits"][int(d["script_off"]):int(d["script_off"] + d["script_len"])]
                rec["diff"] = diff_of([(int(e["at"]), name(e["value"]), int(e["op"])) for e in sc])
            deltas.append(rec)
        res["logs"] = {tid(i): log_of(i) for i in range(len(enc.threads))}
        res["canonical"] = log_of(s["canonical"]) if s["canonical"] >= 0 else None
        res["deltas"] = deltas
        res["nonmonotonic-errors"] = list(enc.nonmonotonic)
        return res


def synth_arrays(n_threads, n_values, edits=None, seed=0):
    """n_threads logs of one random base log of n_values events; edits maps a
    thread's position to a number of scattered single edits (a deletion, an
    insertion or a replacement each, at random places) -> (threads, values)."""
    rng = np.random.default_rng(seed)
    base = rng.integers(1, 2 ** 40, size=n_values, dtype=np.int64)
    logs = []
    for t in range(n_threads):
        log = base
        k = (edits or {}).get(t, 0)
        if k:
            log = list(base)
            for _ in range(k):
                kind, at = int(rng.integers(3)), int(rng.integers(max(len(log), 1)))
                if kind == 0 and log:
                    del log[at]
                elif kind == 1 or not log:
                    log.insert(at, int(rng.integers(1, 2 ** 40)))
                else:
                    log[at] = int(rng.integers(1, 2 ** 40))
            log = np.array(log, dtype=np.int64)
        logs.append(log)
    threads = np.zeros(n_threads, dtype=abi.WT_THREAD_DTYPE)
    off = 0
    for t, log in enumerate(logs):
        threads[t] = (off, len(log), n_values, t)
        off += len(log)
    return threads, (np.concatenate(logs) if logs else np.zeros(0, dtype=np.int64))
