"""Elle's list-append checker with the graph on the device (include/lincheck_append.h).

`encode` makes lc_append_check's three flat arrays from Jepsen op maps in one
pass; `AppendChecker` stands where the reference's `:append` workload puts
`(elle.list-append/check {:consistency-models [:strict-serializable]})`:
`.check(test, history, opts)` returns an Elle-shaped result map with string
keys, `{"valid?", "anomaly-types", "anomalies", "not"}`.
The rules are a re-derivation of elle.list-append; parity with Elle itself is
unpinned.  "phantom" (a read of an element nobody appended) is
our name, not Elle's; "not" names, by the table below, the weakest model each
anomaly found rules out.

A txn op's :value is a list of mops `[f, k, v]`, f one of "append" / "r"
(with or without the keyword's colon).  The Clojure shim and the EDN reader's
CLI do not reach this checker yet.
"""
from collections import Counter, namedtuple

import numpy as np

from . import abi, history as H

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
UNKNOWN = "unknown"
TYPE_CODE = {"ok": abi.LC_AP_OK, "info": abi.LC_AP_INFO, "fail": abi.LC_AP_FAIL}
EDGE_NAMES = {abi.LC_AP_WW: "ww", abi.LC_AP_WR: "wr", abi.LC_AP_RW: "rw", abi.LC_AP_RT: "realtime"}
READ_ANOMALIES = ((abi.LC_AP_R_NONPREFIX, "incompatible-order"), (abi.LC_AP_R_DUPLICATE, "duplicate-elements"),
                  (abi.LC_AP_R_G1A, "G1a"), (abi.LC_AP_R_PHANTOM, "phantom"), (abi.LC_AP_R_G1B, "G1b"),
                  (abi.LC_AP_R_INTERNAL, "internal"))
NOT = {"incompatible-order": "read-uncommitted", "duplicate-elements": "read-uncommitted",
       "phantom": "read-uncommitted", "G0": "read-uncommitted", "G1a": "read-committed", "G1b": "read-committed",
       "G1c": "read-committed", "internal": "read-atomic", "G-single": "consistent-view",
       "G2-item": "repeatable-read", "G0-realtime": "strict-serializable", "G1c-realtime": "strict-serializable",
       "G-single-realtime": "strict-serializable", "G2-item-realtime": "strict-serializable"}


class Unsupported(ValueError):
    """The history cannot be written as lc_append_check's arrays."""


# txns / mops: abi.AP_TXN_DTYPE / AP_MOP_DTYPE arrays; values: the reads'
# payloads, int64; inv / comp: per txn, the history positions of its invoke and
# its completion (-1: none); keys / elements: what the ids stand for (None:
# the history's own integers); n_orphans: completions without an invoke (ignored)
Encoded = namedtuple("Encoded", "txns mops values inv comp keys elements n_orphans")


def _is_int(v):
    return type(v) is int and INT64_MIN < v <= INT64_MAX


def _ident(v):
    """What makes two keys or elements the same (history.Interner's equality)."""
    return (type(v).__name__, v) if not isinstance(v, (list, dict, set)) else repr(v)


def _mops_of(op, pos):
    v = op.get("value")
    if not isinstance(v, (list, tuple)):
        raise Unsupported("op %d: a txn's :value is no list of mops" % pos)
    out = []
    for mop in v:
        if not isinstance(mop, (list, tuple)) or len(mop) != 3 or H._kw(mop[0]) not in ("append", "r"):
            raise Unsupported("op %d: %r is no [f k v] with f :append or :r" % (pos, mop))
        out.append((H._kw(mop[0]), mop[1], mop[2]))
    return out


def encode(history):
    """One pass over the op maps -> Encoded.  An invoke is paired with its
    process's next completion; without one, or with an :info, the txn is INFO."""
    pending, rows, orphans = {}, [], 0   # process -> row; [inv, comp, type, mops]
    for pos, op in enumerate(history):
        if not H.is_client(op) or H._kw(op.get("f")) != "txn":
            continue
        t, p = H._kw(op.get("type")), op["process"]
        if t == "invoke":
            if p in pending:
                raise Unsupported("op %d: process %r invokes while its last txn is pending" % (pos, p))
            pending[p] = row = [pos, -1, abi.LC_AP_INFO, _mops_of(op, pos)]
            rows.append(row)
        elif t in TYPE_CODE:
            row = pending.pop(p, None)
            if row is None:
                orphans += 1
                continue
            if t == "info":
                row[1] = pos  # (kept for the result map; the arrays say -1)
                continue
            row[1], row[2] = pos, TYPE_CODE[t]
            if t == "ok":
                done = _mops_of(op, pos)
                if [(f, _ident(k)) for f, k, _ in done] != [(f, _ident(k)) for f, k, _ in row[3]] or \
                        any(f == "append" and _ident(v) != _ident(v0)
                            for (f, _, v), (_, _, v0) in zip(done, row[3])):
                    raise Unsupported("op %d: the completion's mops are not the invoke's" % pos)
                row[3] = done
    keys = [k for r in rows for _, k, _ in r[3]]
    elems = []
    for r in rows:
        for f, _, v in r[3]:
            if f == "append":
                elems.append(v)
            elif r[2] == abi.LC_AP_OK:
                if v is not None and not isinstance(v, (list, tuple)):
                    raise Unsupported("a read's value %r is no list" % (v,))
                elems.extend(v or ())
    key_ids = elem_ids = None
    if not all(_is_int(k) for k in keys):
        key_ids = {}
        for k in keys:
            key_ids.setdefault(_ident(k), (len(key_ids), k))
    if not all(_is_int(e) for e in elems):
        elem_ids = {}
        for e in elems:
            elem_ids.setdefault(_ident(e), (len(elem_ids), e))
    kid = (lambda k: k) if key_ids is None else (lambda k: key_ids[_ident(k)][0])
    eid = (lambda e: e) if elem_ids is None else (lambda e: elem_ids[_ident(e)][0])
    txns = np.zeros(len(rows), dtype=abi.AP_TXN_DTYPE)
    mops, values, seen = [], [], set()
    for i, (inv, comp, typ, ms) in enumerate(rows):
        txns[i] = (len(mops), inv, comp if typ != abi.LC_AP_INFO else -1, typ, len(ms))
        for f, k, v in ms:
            if f == "append":
                if (kid(k), eid(v)) in seen:
                    raise Unsupported("%r is appended to key %r twice" % (v, k))
                seen.add((kid(k), eid(v)))
                mops.append((kid(k), eid(v), abi.LC_AP_APPEND, 0))
            elif typ == abi.LC_AP_OK:
                mops.append((kid(k), len(values), abi.LC_AP_READ, len(v or ())))
                values.extend(eid(e) for e in (v or ()))
            else:
                mops.append((kid(k), 0, abi.LC_AP_READ, -1))
    return Encoded(txns, np.array(mops, dtype=abi.AP_MOP_DTYPE).reshape(-1), np.array(values, dtype=np.int64),
                   [r[0] for r in rows], [r[1] for r in rows],
                   None if key_ids is None else [k for _, k in key_ids.values()],
                   None if elem_ids is None else [e for _, e in elem_ids.values()], orphans)


def _sorted(xs):
    try:
        return sorted(xs)
    except TypeError:
        return sorted(xs, key=repr)


class _Names:
    """The arrays' ids back as the history's keys, elements, mops and ops."""

    def __init__(self, history, enc):
        self.history, self.enc = history, enc
        self.mop_txn = np.repeat(np.arange(len(enc.txns)), enc.txns["mop_len"])
        self.writer = {(int(m["key"]), int(m["value"])): i for i, m in enumerate(enc.mops)
                       if m["f"] == abi.LC_AP_APPEND}

    def key(self, k):
        return k if self.enc.keys is None else self.enc.keys[k]

    def elem(self, e):
        return e if self.enc.elements is None else self.enc.elements[e]

    def payload(self, m):
        mop = self.enc.mops[m]
        return [int(x) for x in self.enc.values[mop["value"]:mop["value"] + mop["len"]]]

    def mop(self, m):
        mop = self.enc.mops[m]
        if mop["f"] == abi.LC_AP_APPEND:
            return ["append", self.key(int(mop["key"])), self.elem(int(mop["value"]))]
        return ["r", self.key(int(mop["key"])), [self.elem(e) for e in self.payload(m)] if mop["len"] >= 0 else None]

    def op(self, t):
        """The txn's completion, or its invoke where it has none."""
        c = self.enc.comp[t]
        return self.history[c if c >= 0 else self.enc.inv[t]]

    def writer_txn(self, k, e):
        m = self.writer.get((k, e))
        return None if m is None else int(self.mop_txn[m])


def _read_record(nm, out, m, name, orders):
    enc = nm.enc
    t, mop = int(nm.mop_txn[m]), enc.mops[m]
    k, pl = int(mop["key"]), nm.payload(m)
    rec = {"op": nm.op(t), "mop": nm.mop(m)}
    if name == "incompatible-order":
        rec["key"], rec["longest"] = nm.key(k), [nm.elem(e) for e in orders[k]]
    elif name == "duplicate-elements":
        rec["duplicates"] = {nm.elem(e): n for e, n in Counter(pl).items() if n > 1}
    elif name == "phantom":
        rec["element"] = nm.elem(next(e for e in pl if nm.writer_txn(k, e) is None))
    elif name == "G1a":
        e = next(e for e in pl if nm.writer_txn(k, e) is not None
                 and enc.txns["type"][nm.writer_txn(k, e)] == abi.LC_AP_FAIL)
        rec["element"], rec["writer"] = nm.elem(e), nm.op(nm.writer_txn(k, e))
    elif name == "G1b":
        rec["element"], rec["writer"] = nm.elem(pl[-1]), nm.op(nm.writer_txn(k, pl[-1]))
    elif name == "internal":
        first = int(enc.txns["mop_off"][t])
        earlier = [j for j in range(first, m) if int(enc.mops[j]["key"]) == k]
        reads = [j for j in earlier if enc.mops[j]["f"] == abi.LC_AP_READ]
        since = [nm.elem(int(enc.mops[j]["value"])) for j in earlier if not reads or j > reads[-1]]
        rec["expected"] = ([nm.elem(e) for e in nm.payload(reads[-1])] if reads else ["..."]) + since
    return rec


def _step_record(nm, out, orders, ext_len, a, b, typ, k):
    if typ == abi.LC_AP_RT:
        return {"type": "realtime", "a-completed": nm.enc.comp[a], "b-invoked": nm.enc.inv[b]}
    o = orders[k]
    rec = {"type": EDGE_NAMES[typ], "key": nm.key(k)}
    if typ == abi.LC_AP_WW:
        j = next(j for j in range(len(o) - 1) if nm.writer_txn(k, o[j]) == a and nm.writer_txn(k, o[j + 1]) == b)
        rec["value"], rec["value'"] = nm.elem(o[j]), nm.elem(o[j + 1])
    elif typ == abi.LC_AP_WR:
        rec["value"] = nm.elem(o[ext_len[(b, k)] - 1])
    else:
        n = ext_len[(a, k)]
        rec["value"], rec["value'"] = (nm.elem(o[n - 1]) if n else None), nm.elem(o[n])
    return rec


def result_map(history, enc, out, summary):
    """The Elle-shaped result map from the library's arrays."""
    if summary["valid"] < 0:
        return {"valid?": UNKNOWN, "anomaly-types": ["empty-transaction-graph"],
                "anomalies": {"empty-transaction-graph": True}, "not": set()}
    nm = _Names(history, enc)
    orders = {int(k["key"]): nm.payload(int(k["longest"])) for k in out["keys"] if k["longest"] >= 0}
    anomalies = {}
    for m in np.nonzero(out["mop_flags"] & abi.LC_AP_R_ANOMALY)[0]:
        for bit, name in READ_ANOMALIES:
            if out["mop_flags"][m] & bit:
                anomalies.setdefault(name, []).append(_read_record(nm, out, int(m), name, orders))
    ext_len = {(int(nm.mop_txn[m]), int(enc.mops[m]["key"])): int(enc.mops[m]["len"])
               for m in np.nonzero(out["mop_flags"] & abi.LC_AP_R_EXTERNAL)[0]}
    steps, off = out["steps"], out["cycle_off"]
    for c in range(int(summary["n_cycles_returned"])):
        cyc = steps[off[c]:off[c + 1]]
        txs = [int(s["txn"]) for s in cyc]
        name = abi.LC_AP_CLASSES[int(out["scc_class"][txs[0]])]
        anomalies.setdefault(name, []).append({
            "cycle": [nm.op(t) for t in txs] + [nm.op(txs[0])],
            "steps": [_step_record(nm, out, orders, ext_len, txs[i], txs[(i + 1) % len(txs)], int(s["type"]),
                                   int(s["key"])) for i, s in enumerate(cyc)]})
    # (SCCs past the first LC_AP_MAX_CYCLES are named and counted, without a cycle)
    for i, n in enumerate(summary["n_class"]):
        if n:
            anomalies.setdefault(abi.LC_AP_CLASSES[i], [])
    return {"valid?": summary["valid"] == 1, "anomaly-types": _sorted(anomalies),
            "anomalies": anomalies, "not": {NOT[a] for a in anomalies}}


class AppendChecker:
    """Stands where the reference's :append workload puts Elle's list-append
    checker with `:consistency-models [:strict-serializable]`.

    device=True builds the graph on the first GPU of device_mask
    (lc_append_check: the library must have it; there is no quiet fallback);
    device=False uses lc_append_check_host and needs no GPU.

    device_scc=True uses lc_append_check_screened (include/lincheck_screen.h): the
    cycle screen runs on the device, the host's SCC pass only where it does
    not prove the graph clean, and the result map gains an "scc-screen"
    sub-map (clean, rounds, members, ms); every other key is unchanged.  With
    a library that lacks the call the unscreened one runs and the sub-map is
    absent.  Off by default.

    device_cycles=True (it implies device_scc) uses lc_append_check_restricted
    (include/lincheck_cycles.h): where the screen does not prove the graph
    clean, the host pass covers the marked txns only and asks the device which
    txn closes a G-single cycle; the result map gains a "cycle-search" sub-map
    beside "scc-screen", every other key is unchanged.  With a library that
    lacks the call it degrades to device_scc.  Off by default.
    """

    def __init__(self, device_mask=0, device=True, device_scc=False, device_cycles=False):
        self.device_mask = device_mask
        self.device = device
        self.device_scc = device_scc or device_cycles
        self.device_cycles = device_cycles
        self.last_search = None   # device_cycles: lc_cycle_search_summary of the last check, as a dict
        self.last_screen = None   # device_scc: the screen's lc_screen_summary of the last check, as a dict
        self._ctx = None
        self.last_summary = None  # the library's lc_ap_summary of the last check, as a dict
        self.last_out = None      # and its output arrays

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
            scr = srch = None
            if self.device_cycles and abi.has_restricted():
                out, s, scr, srch = self._context().append_check_restricted(enc.txns, enc.mops, enc.values)
            elif self.device_scc and abi.has_screened():
                out, s, scr = self._context().append_check_screened(enc.txns, enc.mops, enc.values)
            else:  # (a library without the screened call: the unscreened one, and no sub-map)
                out, s = self._context().append_check(enc.txns, enc.mops, enc.values)
            self.last_screen, self.last_search = scr, srch
        else:
            self.last_screen = self.last_search = None
            out, s = abi.append_check_host(enc.txns, enc.mops, enc.values)
        self.last_out, self.last_summary = out, s
        result = result_map(history, enc, out, s)
        if self.device and self.last_screen is not None:
            scr = self.last_screen
            result["scc-screen"] = {"clean": {1: True, 0: False, -1: "gave-up"}[scr["clean"]],
                                    "label-rounds": scr["label_rounds"], "trim-rounds": scr["trim_rounds"],
                                    "max-rounds": scr["max_rounds"], "rt-members": scr["n_rt_members"],
                                    "trim-survivors": scr["n_trim_survivors"], "kernel-ms": scr["kernel_ms"],
                                    "ms": scr["total_ms"]}
        if self.device and self.last_search is not None:
            srch = self.last_search
            result["cycle-search"] = {"restricted": bool(srch["restricted"]), "marked": srch["n_marked"],
                                      "device-searches": srch["n_device_searches"],
                                      "device-queries": srch["n_device_queries"],
                                      "host-fallbacks": srch["n_host_fallbacks"], "search-ms": srch["search_ms"]}
        return result


def synth_arrays(n_txns, seed=0, live_keys=3, per_key=32, max_mops=4, concurrency=10, p_info=0.03):
    """A valid history shaped like the reference's :append workload, as
    lc_append_check's arrays, with numpy alone: `live_keys` keys are live at a
    time, a key is retired after `per_key` appends, a txn has 1..max_mops mops
    (half appends, half reads), about `concurrency` txns overlap, and p_info of
    them never complete (their appends take effect).  The txns take effect in
    one serial order that real time respects.  -> (txns, mops, values)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, max_mops + 1, n_txns)
    off = np.cumsum(lens) - lens
    n_mops = int(lens.sum())
    slot = rng.integers(0, live_keys, n_mops)
    is_app = rng.random(n_mops) < 0.5
    before = np.zeros(n_mops, dtype=np.int64)   # appends to the mop's slot so far
    for s in range(live_keys):
        mine = slot == s
        a = (is_app & mine).astype(np.int64)
        before[mine] = (np.cumsum(a) - a)[mine]
    key = slot + live_keys * (before // per_key)
    at = before % per_key                        # the key's length when the mop runs
    info = rng.random(n_txns) < p_info
    t = np.arange(n_txns, dtype=np.float64)
    inv_t, comp_t = t - rng.random(n_txns) * concurrency / 2, t + rng.random(n_txns) * concurrency / 2
    times = np.concatenate([inv_t, comp_t[~info]])
    rank = np.empty(len(times), dtype=np.int64)
    rank[np.argsort(times, kind="stable")] = np.arange(len(times))
    inv_pos, comp_pos = rank[:n_txns], np.full(n_txns, -1, dtype=np.int64)
    comp_pos[~info] = rank[n_txns:]
    perm = np.argsort(inv_pos)                   # txns in invoke order, their mops with them
    new_off = np.cumsum(lens[perm]) - lens[perm]
    src = np.repeat(off[perm] - new_off, lens[perm]) + np.arange(n_mops)
    txns = np.zeros(n_txns, dtype=abi.AP_TXN_DTYPE)
    txns["mop_off"], txns["mop_len"] = new_off, lens[perm]
    txns["inv_pos"], txns["comp_pos"] = inv_pos[perm], comp_pos[perm]
    txns["type"] = np.where(info[perm], abi.LC_AP_INFO, abi.LC_AP_OK)
    mops = np.zeros(n_mops, dtype=abi.AP_MOP_DTYPE)
    mop_info = np.repeat(info, lens)
    mops["key"] = key
    mops["f"] = np.where(is_app, abi.LC_AP_APPEND, abi.LC_AP_READ)
    mops["value"] = np.where(is_app, key * per_key + at, np.where(mop_info, 0, key * per_key))
    mops["len"] = np.where(is_app, 0, np.where(mop_info, -1, at))
    values = np.arange((int(key.max()) + 1) * per_key, dtype=np.int64)  # key k's list is values[k * per_key ...]
    return txns, mops[src], values
