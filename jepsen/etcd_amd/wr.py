"""Elle's rw-register checker for the :wr workload, with the version graphs and
the dependency graph on the device (include/lincheck_wr.h).

`encode` makes lc_wr_check's two flat arrays from Jepsen op maps in one pass;
`WrChecker` stands where the reference's `:wr` workload puts
`(elle.rw-register/check {:consistency-models [:strict-serializable] ...})`:
`.check(test, history, opts)` returns an Elle-shaped result map with string
keys, `{"valid?", "anomaly-types", "anomalies", "not"}`.
The rules are a re-derivation of elle.rw-register; parity with Elle itself is
unpinned.  "phantom" (a read of a value nobody wrote) is our
name, not Elle's; "not" names, by the table below, the weakest model each
anomaly found rules out.

A txn op's :value is a list of mops `[f, k, v]`, f one of "w" / "r" (with or
without the keyword's colon); a read's v is nil (None) until an :ok completion
fills it in, and may be nil there too.  The Clojure shim and the EDN reader's
CLI do not reach this checker yet.
"""
from collections import namedtuple

import numpy as np

from . import abi, history as H
from .append import UNKNOWN, Unsupported, _ident, _is_int, _sorted

TYPE_CODE = {"ok": abi.LC_WR_OK, "info": abi.LC_WR_INFO, "fail": abi.LC_WR_FAIL}
EDGE_NAMES = {abi.LC_AP_WW: "ww", abi.LC_AP_WR: "wr", abi.LC_AP_RW: "rw", abi.LC_AP_RT: "realtime"}
READ_ANOMALIES = ((abi.LC_WR_R_INTERNAL, "internal"), (abi.LC_WR_R_PHANTOM, "phantom"), (abi.LC_WR_R_G1A, "G1a"),
                  (abi.LC_WR_R_G1B, "G1b"))
NOT = {"phantom": "read-uncommitted", "cyclic-versions": "read-uncommitted", "G0": "read-uncommitted",
       "G1a": "read-committed", "G1b": "read-committed", "G1c": "read-committed", "internal": "read-atomic",
       "lost-update": "cursor-stability", "G-single": "consistent-view", "G2-item": "repeatable-read",
       "G0-realtime": "strict-serializable", "G1c-realtime": "strict-serializable",
       "G-single-realtime": "strict-serializable", "G2-item-realtime": "strict-serializable"}

# txns / mops: abi.WR_TXN_DTYPE / WR_MOP_DTYPE arrays; inv / comp: per txn, the
# history positions of its invoke and its completion (-1: none); keys / values:
# what the ids stand for (None: the history's own integers); n_orphans:
# completions without an invoke (ignored)
Encoded = namedtuple("Encoded", "txns mops inv comp keys values n_orphans")


def _mops_of(op, pos):
    v = op.get("value")
    if not isinstance(v, (list, tuple)):
        raise Unsupported("op %d: a txn's :value is no list of mops" % pos)
    out = []
    for mop in v:
        if not isinstance(mop, (list, tuple)) or len(mop) != 3 or H._kw(mop[0]) not in ("w", "r"):
            raise Unsupported("op %d: %r is no [f k v] with f :w or :r" % (pos, mop))
        if H._kw(mop[0]) == "w" and mop[2] is None:
            raise Unsupported("op %d: %r writes nil" % (pos, mop))
        out.append((H._kw(mop[0]), mop[1], mop[2]))
    return out


def encode(history):
    """One pass over the op maps -> Encoded.  An invoke is paired with its
    process's next completion; without one, or with an :info, the txn is INFO.
    An OK txn's mops are its completion's (its reads known, nil where the
    completion says nil); every other txn's are its invoke's, reads unknown."""
    pending, rows, orphans = {}, [], 0   # process -> row; [inv, comp, type, mops]
    for pos, op in enumerate(history):
        if not H.is_client(op) or H._kw(op.get("f")) != "txn":
            continue
        t, p = H._kw(op.get("type")), op["process"]
        if t == "invoke":
            if p in pending:
                raise Unsupported("op %d: process %r invokes while its last txn is pending" % (pos, p))
            pending[p] = row = [pos, -1, abi.LC_WR_INFO, _mops_of(op, pos)]
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
                        any(f == "w" and _ident(v) != _ident(v0) for (f, _, v), (_, _, v0) in zip(done, row[3])):
                    raise Unsupported("op %d: the completion's mops are not the invoke's" % pos)
                row[3] = done
    keys = [k for r in rows for _, k, _ in r[3]]
    vals = [v for r in rows for f, _, v in r[3] if (f == "w" or r[2] == abi.LC_WR_OK) and v is not None]
    key_ids = val_ids = None
    if not all(_is_int(k) for k in keys):
        key_ids = {}
        for k in keys:
            key_ids.setdefault(_ident(k), (len(key_ids), k))
    if not all(_is_int(v) for v in vals):
        val_ids = {}
        for v in vals:
            val_ids.setdefault(_ident(v), (len(val_ids), v))
    kid = (lambda k: k) if key_ids is None else (lambda k: key_ids[_ident(k)][0])
    vid = (lambda v: v) if val_ids is None else (lambda v: val_ids[_ident(v)][0])
    txns = np.zeros(len(rows), dtype=abi.WR_TXN_DTYPE)
    mops, seen = [], set()
    for i, (inv, comp, typ, ms) in enumerate(rows):
        txns[i] = (len(mops), inv, comp if typ != abi.LC_WR_INFO else -1, typ, len(ms))
        for f, k, v in ms:
            if f == "w":
                if (kid(k), vid(v)) in seen:
                    raise Unsupported("%r is written to key %r twice" % (v, k))
                seen.add((kid(k), vid(v)))
                mops.append((kid(k), vid(v), abi.LC_WR_WRITE, 0))
            elif typ == abi.LC_WR_OK:
                mops.append((kid(k), abi.LC_WR_NIL if v is None else vid(v), abi.LC_WR_READ, 1))
            else:
                mops.append((kid(k), 0, abi.LC_WR_READ, 0))
    return Encoded(txns, np.array(mops, dtype=abi.WR_MOP_DTYPE).reshape(-1), [r[0] for r in rows],
                   [r[1] for r in rows], None if key_ids is None else [k for _, k in key_ids.values()],
                   None if val_ids is None else [v for _, v in val_ids.values()], orphans)


class _Names:
    """The arrays' ids back as the history's keys, values, mops and ops; and
    what the records need of rule 2: each txn's external read and its writes
    per key."""

    def __init__(self, history, enc, out):
        self.history, self.enc = history, enc
        self.mop_txn = np.repeat(np.arange(len(enc.txns)), enc.txns["mop_len"])
        self.writer, self.ext_read, self.writes = {}, {}, {}
        for i, m in enumerate(enc.mops):
            t, k, v = int(self.mop_txn[i]), int(m["key"]), int(m["value"])
            if m["f"] == abi.LC_WR_WRITE:
                self.writer[(k, v)] = i
                self.writes.setdefault((t, k), []).append(v)
            elif out["mop_flags"][i] & abi.LC_WR_R_EXTERNAL:
                self.ext_read[(t, k)] = v

    def key(self, k):
        return k if self.enc.keys is None else self.enc.keys[k]

    def value(self, v):
        return None if v == abi.LC_WR_NIL else v if self.enc.values is None else self.enc.values[v]

    def mop(self, m):
        mop = self.enc.mops[m]
        if mop["f"] == abi.LC_WR_WRITE:
            return ["w", self.key(int(mop["key"])), self.value(int(mop["value"]))]
        return ["r", self.key(int(mop["key"])), self.value(int(mop["value"])) if mop["known"] else None]

    def op(self, t):
        """The txn's completion, or its invoke where it has none."""
        c = self.enc.comp[t]
        return self.history[c if c >= 0 else self.enc.inv[t]]

    def writer_op(self, k, v):
        return self.op(int(self.mop_txn[self.writer[(k, v)]]))


def _read_record(nm, m, name):
    enc = nm.enc
    t, mop = int(nm.mop_txn[m]), enc.mops[m]
    k, v = int(mop["key"]), int(mop["value"])
    rec = {"op": nm.op(t), "mop": nm.mop(m)}
    if name == "internal":
        prev = max(j for j in range(int(enc.txns["mop_off"][t]), m) if int(enc.mops[j]["key"]) == k)
        rec["expected"] = nm.value(int(enc.mops[prev]["value"]))
    elif name in ("G1a", "G1b"):
        rec["writer"] = nm.writer_op(k, v)
    return rec


def _step_record(nm, wfr, a, b, typ, k, lin=False):
    if typ == abi.LC_AP_RT:
        return {"type": "realtime", "a-completed": nm.enc.comp[a], "b-invoked": nm.enc.inv[b]}
    rec = {"type": EDGE_NAMES[typ], "key": nm.key(k)}
    if lin and typ != abi.LC_AP_WR:  # a version edge of any source: which of b's values follows is not restated
        if typ == abi.LC_AP_RW:
            rec["value"] = nm.value(nm.ext_read[(a, k)])
        return rec
    if typ == abi.LC_AP_WR:
        rec["value"] = nm.value(nm.ext_read[(b, k)])
    elif typ == abi.LC_AP_WW:  # a wfr edge: b read a's value and went on to write
        rec["value"], rec["value'"] = nm.value(nm.ext_read[(b, k)]), nm.value(nm.writes[(b, k)][-1])
    else:  # b's write follows what a read: by b's own read of it, or because a read nil
        v = nm.ext_read[(a, k)]
        follows = nm.writes[(b, k)][-1] if wfr and nm.ext_read.get((b, k)) == v else nm.writes[(b, k)][0]
        rec["value"], rec["value'"] = nm.value(v), nm.value(follows)
    return rec


def version_cycle(nm, k, v0):
    """The version cycle of key k through v0, walked against rule 4's wfr
    edges (a value's parent is what its writer's txn read externally), as the
    values in their order, the first repeated at the end."""
    back, v = [v0], v0
    for _ in range(len(nm.writer) + 1):
        v = nm.ext_read[(int(nm.mop_txn[nm.writer[(k, v)]]), k)]
        back.append(v)
        if v == v0:
            break
    return [nm.value(x) for x in reversed(back)]


def lin_version_edges(nm, k, wfr):
    """Key k's version edges under include/lincheck_wrlin.h's rule 4', as a
    dict value -> set of values (ids; LC_WR_NIL is nil), derived from the
    arrays: initial, wfr (if asked) and lin, the last by walking each touch's
    later touches in invoke order while none of them has completed before the
    next is invoked."""
    enc = nm.enc
    succ = {}
    for (k2, v), m in nm.writer.items():
        if k2 == k and enc.txns["type"][nm.mop_txn[m]] != abi.LC_WR_FAIL:
            succ.setdefault(abi.LC_WR_NIL, set()).add(v)
    touches = []  # (inv, comp, first, last), ascending by inv
    for t in sorted({t for (t, k2) in list(nm.ext_read) + list(nm.writes) if k2 == k}):
        if enc.txns["type"][t] != abi.LC_WR_OK:
            continue
        r, w = nm.ext_read.get((t, k)), nm.writes.get((t, k))
        first, last = (r if r is not None else w[-1]), (w[-1] if w else r)
        if wfr and r is not None and w:
            succ.setdefault(r, set()).add(w[-1])
        touches.append((int(enc.txns["inv_pos"][t]), int(enc.txns["comp_pos"][t]), first, last))
    for i, (_, comp, _, last) in enumerate(touches):
        least = None  # the least completion among the touches invoked after comp, so far
        for inv2, comp2, first2, _ in touches[i + 1:]:
            if inv2 < comp:
                continue
            if least is not None and least < inv2:
                break
            least = comp2 if least is None else min(least, comp2)
            if last != first2:
                succ.setdefault(last, set()).add(first2)
    return succ


def lin_version_cycle(nm, k, v0, wfr):
    """A cycle of key k's version graph through v0, depth first, as the values
    in their order, the first repeated at the end."""
    succ = lin_version_edges(nm, k, wfr)
    path, stack, seen = [v0], [iter(sorted(succ.get(v0, ())))], set()
    while stack:
        v = next(stack[-1], None)
        if v is None:
            stack.pop()
            path.pop()
        elif v == v0:
            return [nm.value(x) for x in path + [v0]]
        elif v not in seen:
            seen.add(v)
            path.append(v)
            stack.append(iter(sorted(succ.get(v, ()))))
    raise AssertionError("key %r: no version cycle through %r" % (k, v0))


def result_map(history, enc, out, summary, wfr_keys=True, lin_keys=False):
    """The Elle-shaped result map from the library's arrays."""
    if summary["valid"] < 0:
        return {"valid?": UNKNOWN, "anomaly-types": ["empty-transaction-graph"],
                "anomalies": {"empty-transaction-graph": True}, "not": set()}
    nm = _Names(history, enc, out)
    anomalies = {}
    for m in np.nonzero(out["mop_flags"] & abi.LC_WR_R_ANOMALY)[0]:
        for bit, name in READ_ANOMALIES:
            if out["mop_flags"][m] & bit:
                anomalies.setdefault(name, []).append(_read_record(nm, int(m), name))
    for k in out["keys"]:
        if k["flags"] & abi.LC_WR_K_CYCLIC:
            kk, v0 = int(k["key"]), int(k["cyc_value"])
            anomalies.setdefault("cyclic-versions", []).append(
                {"key": nm.key(kk), "cycle": lin_version_cycle(nm, kk, v0, wfr_keys) if lin_keys
                 else version_cycle(nm, kk, v0)})
    if summary["n_lost_update"]:
        groups = {}  # (key, value) -> the txns that read it externally and write the key, in txn order
        for (t, k), v in sorted(nm.ext_read.items()):
            if (t, k) in nm.writes:
                groups.setdefault((k, v), []).append(t)
        anomalies["lost-update"] = [{"key": nm.key(k), "value": nm.value(v), "txns": [nm.op(t) for t in ts]}
                                    for (k, v), ts in groups.items() if len(ts) > 1]
    steps, off = out["steps"], out["cycle_off"]
    for c in range(int(summary["n_cycles_returned"])):
        cyc = steps[off[c]:off[c + 1]]
        txs = [int(s["txn"]) for s in cyc]
        name = abi.LC_AP_CLASSES[int(out["scc_class"][txs[0]])]
        anomalies.setdefault(name, []).append({
            "cycle": [nm.op(t) for t in txs] + [nm.op(txs[0])],
            "steps": [_step_record(nm, wfr_keys, txs[i], txs[(i + 1) % len(txs)], int(s["type"]), int(s["key"]),
                                   lin_keys)
                      for i, s in enumerate(cyc)]})
    # (SCCs past the first LC_AP_MAX_CYCLES are named and counted, without a cycle)
    for i, n in enumerate(summary["n_class"]):
        if n:
            anomalies.setdefault(abi.LC_AP_CLASSES[i], [])
    return {"valid?": summary["valid"] == 1, "anomaly-types": _sorted(anomalies),
            "anomalies": anomalies, "not": {NOT[a] for a in anomalies}}


class WrChecker:
    """Stands where the reference's :wr workload puts Elle's rw-register
    checker with `:consistency-models [:strict-serializable]`.

    wfr_keys: whether rule 4's wfr edges are inferred (a txn that reads a key
    and then writes it orders what it read before what it wrote).  The
    reference passes `:wfr-keys true`; Elle's option is, as far as we recall,
    `:wfr-keys?`, so that whether the reference's spelling switches the
    inference on cannot be settled here.  It defaults to on, the evident
    intent; False follows the other reading.

    device=True works on the first GPU of device_mask (lc_wr_check: the
    library must have it; there is no quiet fallback); device=False uses
    lc_wr_check_host and needs no GPU.

    device_scc=True uses lc_wr_check_screened (include/lincheck_screen.h): the
    cycle screen runs on the device, the host's SCC pass only where it does
    not prove the graph clean, and the result map gains an "scc-screen"
    sub-map (clean, rounds, members, ms); every other key is unchanged.  With
    a library that lacks the call the unscreened one runs and the sub-map is
    absent.  Off by default.

    device_cycles=True (it implies device_scc) uses lc_wr_check_restricted
    (include/lincheck_cycles.h): where the screen does not prove the graph
    clean, the host pass covers the marked txns only and asks the device which
    txn closes a G-single cycle; the result map gains a "cycle-search" sub-map
    beside "scc-screen", every other key is unchanged.  With a library that
    lacks the call it degrades to device_scc.  Off by default.

    linearizable_keys=True adds Elle's :linearizable-keys? inference
    (include/lincheck_wrlin.h; the reference comments it out as expensive):
    real time orders each key's versions, so that a stale read between blind
    writes is caught.  It uses lc_wr_check_lin (device) or
    lc_wr_check_lin_host; the library must have them.  The result map gains
    "linearizable-keys": {"touches", "pairs", "version-edges"}; a ww / rw step
    record then carries "type" and "key" (and for rw the value read) without
    "value'", and a cyclic key's "cycle" is found depth first over the key's
    version edges, which the binding derives for the cyclic keys alone.  Not
    together with device_scc / device_cycles (ValueError).  Off by default.
    """

    def __init__(self, device_mask=0, device=True, wfr_keys=True, device_scc=False, device_cycles=False,
                 linearizable_keys=False):
        if linearizable_keys and (device_scc or device_cycles):
            raise ValueError("linearizable_keys has no screened or restricted call: not with device_scc / device_cycles")
        self.linearizable_keys = linearizable_keys
        self.last_lin = None      # linearizable_keys: lc_wr_lin_summary of the last check, as a dict
        self.device_mask = device_mask
        self.device = device
        self.device_scc = device_scc or device_cycles
        self.device_cycles = device_cycles
        self.last_search = None   # device_cycles: lc_cycle_search_summary of the last check, as a dict
        self.last_screen = None   # device_scc: the screen's lc_screen_summary of the last check, as a dict
        self.wfr_keys = wfr_keys
        self._ctx = None
        self.last_summary = None  # the library's lc_wr_summary of the last check, as a dict
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
        if self.linearizable_keys:
            if not abi.has_wr_lin():
                raise RuntimeError("the loaded library has no lc_wr_check_lin")
            self.last_screen = self.last_search = None
            if self.device:
                out, s, ls = self._context().wr_check_lin(enc.txns, enc.mops, self.wfr_keys)
            else:
                out, s, ls = abi.wr_check_lin_host(enc.txns, enc.mops, self.wfr_keys)
            self.last_out, self.last_summary, self.last_lin = out, s, ls
            result = result_map(history, enc, out, s, self.wfr_keys, True)
            result["linearizable-keys"] = {"touches": ls["n_touches"], "pairs": ls["n_pairs"],
                                           "version-edges": ls["n_vedges"]}
            return result
        if self.device:
            scr = srch = None
            if self.device_cycles and abi.has_restricted():
                out, s, scr, srch = self._context().wr_check_restricted(enc.txns, enc.mops, self.wfr_keys)
            elif self.device_scc and abi.has_screened():
                out, s, scr = self._context().wr_check_screened(enc.txns, enc.mops, self.wfr_keys)
            else:  # (a library without the screened call: the unscreened one, and no sub-map)
                out, s = self._context().wr_check(enc.txns, enc.mops, self.wfr_keys)
            self.last_screen, self.last_search = scr, srch
        else:
            self.last_screen = self.last_search = None
            out, s = abi.wr_check_host(enc.txns, enc.mops, self.wfr_keys)
        self.last_out, self.last_summary = out, s
        result = result_map(history, enc, out, s, self.wfr_keys)
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
    """A valid history shaped like the reference's :wr workload, as
    lc_wr_check's arrays, with numpy alone: `live_keys` keys are live at a
    time, a key is retired after `per_key` writes, a txn has 1..max_mops mops
    (half writes, half reads), about `concurrency` txns overlap, and p_info of
    them never complete (their writes take effect).  The txns take effect in
    one serial order that real time respects.  -> (txns, mops)."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, max_mops + 1, n_txns)
    off = np.cumsum(lens) - lens
    n_mops = int(lens.sum())
    slot = rng.integers(0, live_keys, n_mops)
    is_w = rng.random(n_mops) < 0.5
    before = np.zeros(n_mops, dtype=np.int64)   # writes to the mop's slot so far
    for s in range(live_keys):
        mine = slot == s
        a = (is_w & mine).astype(np.int64)
        before[mine] = (np.cumsum(a) - a)[mine]
    key = slot + live_keys * (before // per_key)
    at = before % per_key                        # the key's writes when the mop runs
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
    txns = np.zeros(n_txns, dtype=abi.WR_TXN_DTYPE)
    txns["mop_off"], txns["mop_len"] = new_off, lens[perm]
    txns["inv_pos"], txns["comp_pos"] = inv_pos[perm], comp_pos[perm]
    txns["type"] = np.where(info[perm], abi.LC_WR_INFO, abi.LC_WR_OK)
    mops = np.zeros(n_mops, dtype=abi.WR_MOP_DTYPE)
    mop_info = np.repeat(info, lens)
    mops["key"] = key
    mops["f"] = np.where(is_w, abi.LC_WR_WRITE, abi.LC_WR_READ)
    # key k's j-th write has the value k * per_key + j (j from 1); a read sees the latest, nil before the first
    seen = np.where(at == 0, abi.LC_WR_NIL, key * per_key + at)
    mops["value"] = np.where(is_w, key * per_key + at + 1, np.where(mop_info, 0, seen))
    mops["known"] = np.where(is_w | mop_info, 0, 1)
    return txns, mops[src]
