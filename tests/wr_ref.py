"""An independent restatement of rw-register (include/lincheck_wr.h) for the
tests: plain Python over the op maps, dicts and sets; each key's version graph
an explicit edge set searched depth first (no parent pointers, no pointer
jumping); Elle's real-time frontier walk as the prose has it (not the range
formula); and cycles from a boolean reachability closure over the UNREDUCED
interval order — reduction preserves reachability, so SCCs and classes must
agree with the library's.  It shares no code with jepsen/etcd_amd/wr.py or the
C sources.  Small histories only: the closure is cubic."""
import numpy as np

CLASSES = ("G0", "G1c", "G-single", "G2-item", "G0-realtime", "G1c-realtime", "G-single-realtime",
           "G2-item-realtime")
READ_NAMES = ("internal", "phantom", "G1a", "G1b")
KEY_NAMES = ("cyclic-versions", "lost-update")
NOT = {"phantom": "read-uncommitted", "cyclic-versions": "read-uncommitted", "G0": "read-uncommitted",
       "G1a": "read-committed", "G1b": "read-committed", "G1c": "read-committed", "internal": "read-atomic",
       "lost-update": "cursor-stability", "G-single": "consistent-view", "G2-item": "repeatable-read"}
NOT.update({c: "strict-serializable" for c in CLASSES[4:]})
NIL = None


def _kw(x):
    return x[1:] if isinstance(x, str) and x.startswith(":") else x


def transactions(history):
    """-> the txns in invoke order: {"inv", "comp", "type", "mops", "op"};
    mops are (f, k, v, known) from the completion when it is :ok, else from the
    invoke with every read unknown."""
    txns, pending = [], {}
    for pos, op in enumerate(history):
        p = op.get("process")
        if not isinstance(p, int) or isinstance(p, bool) or _kw(op.get("f")) != "txn":
            continue
        t = _kw(op["type"])
        if t == "invoke":
            pending[p] = x = {"inv": pos, "comp": None, "type": "info", "op": op,
                              "mops": [(_kw(f), k, v if _kw(f) == "w" else None, False) for f, k, v in op["value"]]}
            txns.append(x)
        elif p in pending:
            x = pending.pop(p)
            x["op"] = op
            if t != "info":
                x["comp"], x["type"] = pos, t
            if t == "ok":
                x["mops"] = [(_kw(f), k, v, _kw(f) == "r") for f, k, v in op["value"]]
    return txns


def _closure(a):
    """Transitive closure of a boolean adjacency matrix (paths of length >= 1)."""
    r = a.copy()
    while True:
        n = r | ((r.astype(np.uint8) @ r.astype(np.uint8)) > 0)
        if (n == r).all():
            return r
        r = n


def _on_cycles(vedges):
    """The versions lying on a cycle of the edge set: v reaches itself, depth first."""
    succ = {}
    for a, b in vedges:
        succ.setdefault(a, []).append(b)
    on = set()
    for v0 in succ:
        stack, seen = list(succ[v0]), set()
        while stack:
            v = stack.pop()
            if v == v0:
                on.add(v0)
                break
            if v not in seen:
                seen.add(v)
                stack.extend(succ.get(v, ()))
    return on


def check(history, wfr_keys=True):
    txns = transactions(history)
    n = len(txns)
    ok = [x["type"] == "ok" for x in txns]
    node = [x["type"] != "fail" for x in txns]
    # rule 1
    writer, writes = {}, {}
    for t, x in enumerate(txns):
        for f, k, v, _ in x["mops"]:
            if f == "w":
                assert (k, v) not in writer, "two writes of one (key, value)"
                writer[(k, v)] = t
                writes.setdefault((t, k), []).append(v)
    all_keys = sorted({k for x in txns for _, k, _, _ in x["mops"]})
    # rules 2 and 3
    read_flags, ext_read = {}, {}
    for t, x in enumerate(txns):
        if not ok[t]:
            continue
        latest = {}
        for i, (f, k, v, known) in enumerate(x["mops"]):
            if f == "r":
                fl = set()
                if k in latest:
                    if latest[k] != v:
                        fl.add("internal")
                else:
                    fl.add("external")
                    ext_read[(t, k)] = v
                if v is not NIL:
                    if (k, v) not in writer:
                        fl.add("phantom")
                    else:
                        w = writer[(k, v)]
                        if txns[w]["type"] == "fail":
                            fl.add("G1a")
                        if w != t and writes[(w, k)][-1] != v:
                            fl.add("G1b")
                read_flags[(t, i)] = fl
            latest[k] = v
    # rules 4 to 6
    keys = {}
    vedges = {k: set() for k in all_keys}      # rule 4, self-loops left out
    wfr_edges = {k: set() for k in all_keys}   # the wfr edges, self-loops included
    for k in all_keys:
        versions = {NIL} | {v for (k2, v) in writer if k2 == k} | \
            {x["mops"][i][2] for (t, i), fl in read_flags.items() for x in [txns[t]] if x["mops"][i][1] == k}
        for (k2, v), w in writer.items():
            if k2 == k and node[w]:
                vedges[k].add((NIL, v))
        readers_writers = {}
        for (t, k2), a in ext_read.items():
            if k2 == k and (t, k) in writes:
                readers_writers.setdefault(a, []).append(t)
                if wfr_keys:
                    wfr_edges[k].add((a, writes[(t, k)][-1]))
        vedges[k] |= {(a, b) for a, b in wfr_edges[k] if a != b}
        on = _on_cycles(wfr_edges[k])
        keys[k] = {"cyclic": bool(on), "cyc_value": min(on) if on else None,
                   "lost": any(len(ts) > 1 for ts in readers_writers.values()),
                   "lost_versions": sorted((a is not NIL, a) for a, ts in readers_writers.items() if len(ts) > 1),
                   "n_writes": sum(1 for x in txns for f, k2, _, _ in x["mops"] if f == "w" and k2 == k),
                   "n_versions": len(versions),
                   "n_ext_reads": sum(1 for (t, k2) in ext_read if k2 == k)}
    # rule 7
    edges = set()

    def edge(a, b, typ, k):
        if a != b and node[a] and node[b]:
            edges.add((a, b, typ, k))

    for (t, k), v in ext_read.items():
        if v is not NIL and (k, v) in writer:
            edge(writer[(k, v)], t, "wr", k)
    for k in all_keys:
        if keys[k]["cyclic"]:
            continue
        for a, b in vedges[k]:
            w = writer[(k, b)]
            if (k, a) in writer:
                edge(writer[(k, a)], w, "ww", k)
            for (t, k2), v in ext_read.items():
                if k2 == k and v == a:
                    edge(t, w, "rw", k)
    # rule 8: Elle's frontier walk over the history
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

    # rule 9: closures; real time unreduced
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
    # rule 10 and the result map
    counts = {name: sum(name in fl for fl in read_flags.values()) for name in READ_NAMES}
    counts["cyclic-versions"] = sum(rec["cyclic"] for rec in keys.values())
    counts["lost-update"] = sum(len(rec["lost_versions"]) for rec in keys.values())
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
        names = sorted({name for fl in read_flags.values() for name in fl - {"external"}} | set(classes) |
                       {name for name in KEY_NAMES if counts[name]})
        valid = not names
        anomalies = {}
        for (t, i), fl in sorted(read_flags.items()):
            f, k, v, _ = txns[t]["mops"][i]
            for name in READ_NAMES:
                if name not in fl:
                    continue
                rec = {"op": txns[t]["op"], "mop": ["r", k, v]}
                if name == "internal":
                    rec["expected"] = [m[2] for m in txns[t]["mops"][:i] if m[1] == k][-1]
                elif name in ("G1a", "G1b"):
                    rec["writer"] = txns[writer[(k, v)]]["op"]
                anomalies.setdefault(name, []).append(rec)
        for k in all_keys:
            if keys[k]["cyclic"]:
                pred = {}
                for a, b in wfr_edges[k]:
                    assert b not in pred  # one incoming wfr edge at most
                    pred[b] = a
                back = [keys[k]["cyc_value"]]
                while len(back) == 1 or back[-1] != back[0]:
                    back.append(pred[back[-1]])
                anomalies.setdefault("cyclic-versions", []).append({"key": k, "cycle": back[::-1]})
        groups = {}
        for t in range(n):
            for k in all_keys:
                if (t, k) in ext_read and (t, k) in writes:
                    groups.setdefault((k, ext_read[(t, k)]), []).append(t)
        lost = [{"key": k, "value": v, "txns": [txns[t]["op"] for t in ts]}
                for (k, v), ts in groups.items() if len(ts) > 1]
        if lost:
            anomalies["lost-update"] = lost
        for c in classes:
            anomalies.setdefault(c, None)  # cycles are certified by the tests, not restated here
        result = {"valid?": valid, "anomaly-types": names, "anomalies": anomalies, "not": {NOT[a] for a in names}}
    for rec in keys.values():
        del rec["lost_versions"]
    return {"txns": txns, "read_flags": read_flags, "txn_flags": txn_flags, "keys": keys, "edges": edges,
            "rt_pred": rt_pred, "sccs": sccs, "classes": classes, "counts": counts, "valid": valid,
            "result": result}
