"""An independent restatement of list-append (include/lincheck_append.h) for
the tests: plain Python over the op maps, dicts and sets, Elle's real-time
frontier walk as the prose has it (not the range formula), and cycles from a
boolean reachability closure over the UNREDUCED interval order — reduction
preserves reachability, so SCCs and classes must agree with the library's.
It shares no code with jepsen/etcd_amd/append.py or the C sources.  Small
histories only: the closure is cubic."""
from collections import Counter

import numpy as np

CLASSES = ("G0", "G1c", "G-single", "G2-item", "G0-realtime", "G1c-realtime", "G-single-realtime",
           "G2-item-realtime")
READ_NAMES = ("incompatible-order", "duplicate-elements", "G1a", "phantom", "G1b", "internal")
NOT = {"incompatible-order": "read-uncommitted", "duplicate-elements": "read-uncommitted",
       "phantom": "read-uncommitted", "G0": "read-uncommitted", "G1a": "read-committed", "G1b": "read-committed",
       "G1c": "read-committed", "internal": "read-atomic", "G-single": "consistent-view",
       "G2-item": "repeatable-read"}
NOT.update({c: "strict-serializable" for c in CLASSES[4:]})


def _kw(x):
    return x[1:] if isinstance(x, str) and x.startswith(":") else x


def transactions(history):
    """-> the txns in invoke order: {"inv", "comp", "type", "mops", "op"};
    mops are (f, k, v) from the completion when it is :ok, else from the invoke,
    and a read's v is None unless the txn is ok."""
    txns, pending = [], {}
    for pos, op in enumerate(history):
        p = op.get("process")
        if not isinstance(p, int) or isinstance(p, bool) or _kw(op.get("f")) != "txn":
            continue
        t = _kw(op["type"])
        if t == "invoke":
            pending[p] = x = {"inv": pos, "comp": None, "type": "info", "op": op,
                              "mops": [(_kw(f), k, None if _kw(f) == "r" else v) for f, k, v in op["value"]]}
            txns.append(x)
        elif p in pending:
            x = pending.pop(p)
            x["op"] = op
            if t != "info":
                x["comp"], x["type"] = pos, t
            if t == "ok":
                x["mops"] = [(_kw(f), k, list(v or ()) if _kw(f) == "r" else v) for f, k, v in op["value"]]
    return txns


def _closure(a):
    """Transitive closure of a boolean adjacency matrix (paths of length >= 1)."""
    r = a.copy()
    while True:
        n = r | ((r.astype(np.uint8) @ r.astype(np.uint8)) > 0)
        if (n == r).all():
            return r
        r = n


def check(history):
    txns = transactions(history)
    n = len(txns)
    ok = [x["type"] == "ok" for x in txns]
    node = [x["type"] != "fail" for x in txns]
    # rule 1
    writer, appends = {}, {}
    for t, x in enumerate(txns):
        for i, (f, k, v) in enumerate(x["mops"]):
            if f == "append":
                assert (k, v) not in writer, "two appends of one (key, element)"
                writer[(k, v)] = t
                appends.setdefault((t, k), []).append(v)
    # rule 2
    all_keys = sorted({k for x in txns for _, k, _ in x["mops"]})
    reads = [(t, i, k, v) for t, x in enumerate(txns) if ok[t] for i, (f, k, v) in enumerate(x["mops"]) if f == "r"]
    keys = {}
    for k in all_keys:
        mine = [r for r in reads if r[2] == k]
        rec = {"longest": None, "order": [], "incompatible": False, "first_dup": -1, "first_failed": -1,
               "first_phantom": -1}
        if mine:
            best = max(len(r[3]) for r in mine)
            t, i, _, order = next(r for r in mine if len(r[3]) == best)
            rec["longest"], rec["order"] = (t, i), order
            for j, e in enumerate(order):
                if e in order[:j] and rec["first_dup"] < 0:
                    rec["first_dup"] = j
                if (k, e) not in writer and rec["first_phantom"] < 0:
                    rec["first_phantom"] = j
                if (k, e) in writer and txns[writer[(k, e)]]["type"] == "fail" and rec["first_failed"] < 0:
                    rec["first_failed"] = j
        keys[k] = rec
    read_flags = {}
    for t, i, k, v in reads:
        fl = set()
        if v != keys[k]["order"][:len(v)]:
            fl.add("incompatible-order")
            keys[k]["incompatible"] = True
        # rule 3
        if max(Counter(v).values(), default=0) > 1:
            fl.add("duplicate-elements")
        if any((k, e) in writer and txns[writer[(k, e)]]["type"] == "fail" for e in v):
            fl.add("G1a")
        if any((k, e) not in writer for e in v):
            fl.add("phantom")
        if v and (k, v[-1]) in writer:
            w = writer[(k, v[-1])]
            if w != t and appends[(w, k)][-1] != v[-1]:
                fl.add("G1b")
        # rule 4
        before = [(f, v2) for f, k2, v2 in txns[t]["mops"][:i] if k2 == k]
        last_read = max((j for j, (f, _) in enumerate(before) if f == "r"), default=None)
        if last_read is not None:
            if v != before[last_read][1] + [a for _, a in before[last_read + 1:]]:
                fl.add("internal")
        elif before:
            own = [a for _, a in before]
            if v[len(v) - len(own):] != own or len(v) < len(own):
                fl.add("internal")
        else:
            fl.add("external")
        read_flags[(t, i)] = fl
    for rec in keys.values():
        rec["no_order"] = rec["incompatible"] or rec["first_dup"] >= 0 or rec["first_phantom"] >= 0
    # rule 5
    edges = set()

    def edge(a, b, typ, k):
        if a != b and node[a] and node[b]:
            edges.add((a, b, typ, k))

    for k, rec in keys.items():
        if rec["no_order"]:
            continue
        o = rec["order"]
        for a, b in zip(o, o[1:]):
            edge(writer[(k, a)], writer[(k, b)], "ww", k)
        for t, i, k2, v in reads:
            if k2 == k and "external" in read_flags[(t, i)]:
                if v:
                    edge(writer[(k, o[len(v) - 1])], t, "wr", k)
                if len(v) < len(o):
                    edge(t, writer[(k, o[len(v)])], "rw", k)
    # rule 6: Elle's frontier walk over the history
    by_inv = {x["inv"]: t for t, x in enumerate(txns)}
    by_comp = {x["comp"]: t for t, x in enumerate(txns) if ok[t]}
    frontier, seen, rt_pred = set(), {}, {t: set() for t in range(n)}
    for pos in range(len(history)):
        if pos in by_inv:
            t = by_inv[pos]
            seen[t] = set(frontier)
            if node[t]:
                rt_pred[t] = set(frontier)
        if pos in by_comp:
            t = by_comp[pos]
            frontier = (frontier - seen[t]) | {t}
    # rule 7: closures; real time unreduced
    def matrix(types, rt):
        a = np.zeros((n, n), dtype=bool)
        for x, y, typ, _ in edges:
            if typ in types:
                a[x, y] = True
        if rt:
            for x in range(n):
                for y in range(n):
                    if ok[x] and node[y] and txns[x]["comp"] < txns[y]["inv"]:
                        a[x, y] = True
        return a

    sccs, classes = [], []
    if n:
        full = _closure(matrix({"ww", "wr", "rw"}, True))
        reach = {(types, rt): _closure(matrix(set(types), rt))
                 for rt in (False, True) for types in (("ww",), ("ww", "wr"), ("ww", "wr", "rw"))}
        done = set()
        for t in range(n):
            if t in done or not full[t, t]:
                continue
            s = frozenset(u for u in range(n) if full[t, u] and full[u, t])
            done |= s
            sccs.append(s)
            cls = None
            for rt in (False, True):
                inside = [(x, y, typ) for x, y, typ, _ in edges if x in s and y in s]
                tests = (any(reach[(("ww",), rt)][u, u] for u in s),
                         any(typ == "wr" and reach[(("ww", "wr"), rt)][y, x] for x, y, typ in inside),
                         any(typ == "rw" and reach[(("ww", "wr"), rt)][y, x] for x, y, typ in inside),
                         any(reach[(("ww", "wr", "rw"), rt)][u, u] for u in s))
                if cls is None and any(tests):
                    cls = CLASSES[tests.index(True) + (4 if rt else 0)]
            classes.append(cls)
    # rule 8 and the result map
    counts = {name: sum(name in fl for fl in read_flags.values()) for name in READ_NAMES}
    counts["incompatible-keys"] = sum(rec["incompatible"] for rec in keys.values())
    for c in CLASSES:
        counts[c] = classes.count(c)
    txn_flags = {t: set() for t in range(n)}
    for (t, i), fl in read_flags.items():
        txn_flags[t] |= fl - {"external"}
    if not any(ok):
        valid = "unknown"
        result = {"valid?": "unknown", "anomaly-types": ["empty-transaction-graph"],
                  "anomalies": {"empty-transaction-graph": True}, "not": set()}
    else:
        names = sorted({name for fl in read_flags.values() for name in fl - {"external"}} | set(classes))
        valid = not names
        anomalies = {}
        for (t, i), fl in sorted(read_flags.items()):
            f, k, v = txns[t]["mops"][i]
            for name in READ_NAMES:
                if name not in fl:
                    continue
                rec = {"op": txns[t]["op"], "mop": ["r", k, v]}
                if name == "incompatible-order":
                    rec["key"], rec["longest"] = k, keys[k]["order"]
                elif name == "duplicate-elements":
                    rec["duplicates"] = {e: c for e, c in Counter(v).items() if c > 1}
                elif name == "phantom":
                    rec["element"] = [e for e in v if (k, e) not in writer][0]
                elif name == "G1a":
                    e = [e for e in v if (k, e) in writer and txns[writer[(k, e)]]["type"] == "fail"][0]
                    rec["element"], rec["writer"] = e, txns[writer[(k, e)]]["op"]
                elif name == "G1b":
                    rec["element"], rec["writer"] = v[-1], txns[writer[(k, v[-1])]]["op"]
                else:
                    before = [(f2, v2) for f2, k2, v2 in txns[t]["mops"][:i] if k2 == k]
                    lr = max((j for j, (f2, _) in enumerate(before) if f2 == "r"), default=None)
                    rec["expected"] = (["..."] + [a for _, a in before]) if lr is None else \
                        before[lr][1] + [a for _, a in before[lr + 1:]]
                anomalies.setdefault(name, []).append(rec)
        for c in classes:
            anomalies.setdefault(c, None)  # cycles are certified by the tests, not restated here
        result = {"valid?": valid, "anomaly-types": names, "anomalies": anomalies, "not": {NOT[a] for a in names}}
    return {"txns": txns, "read_flags": read_flags, "txn_flags": txn_flags, "keys": keys, "edges": edges,
            "rt_pred": rt_pred, "sccs": sccs, "classes": classes, "counts": counts, "valid": valid,
            "result": result}
