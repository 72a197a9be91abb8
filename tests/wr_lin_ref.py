"""An independent restatement of rw-register with the :linearizable-keys?
inference (include/lincheck_wrlin.h) for the tests: plain Python over the op
maps.  Rules 1-3, 5 and 8 are wr_ref.py's (its check() is called for them);
rule 4''s key-successor relation comes straight from its definition — all pairs
with the "no T3 between" test, no sorting, no ranges; each key's version graph
is an explicit edge set searched depth first (wr_ref._on_cycles); rule 9 is a
boolean closure over the unreduced interval order, as in wr_ref.py.  It shares
no code with jepsen/etcd_amd/wr.py or the C sources.  Small histories only."""
import numpy as np

import wr_ref as REF

NIL = REF.NIL


def key_successors(members, txns):
    """Rule 4' by its definition: the (t1, t2) with comp(t1) < inv(t2) and no
    member t3 with comp(t1) < inv(t3) and comp(t3) < inv(t2)."""
    return [(a, b) for a in members for b in members
            if txns[a]["comp"] < txns[b]["inv"] and
            not any(txns[a]["comp"] < txns[c]["inv"] and txns[c]["comp"] < txns[b]["inv"] for c in members)]


def check(history, wfr_keys=True, lin_keys=True):
    base = REF.check(history, wfr_keys)
    txns, n = base["txns"], len(base["txns"])
    all_keys = sorted(base["keys"])
    if not lin_keys:
        base["lin"] = {k: {"n_pairs": 0, "n_touches": 0, "n_vedges": 0} for k in all_keys}
        base["lin_totals"] = {"touches": 0, "pairs": 0, "version-edges": 0}
        return base
    ok = [x["type"] == "ok" for x in txns]
    node = [x["type"] != "fail" for x in txns]
    writer, writes, ext_read = {}, {}, {}
    for t, x in enumerate(txns):
        for i, (f, k, v, _) in enumerate(x["mops"]):
            if f == "w":
                writer[(k, v)] = t
                writes.setdefault((t, k), []).append(v)
            elif "external" in base["read_flags"].get((t, i), ()):
                ext_read[(t, k)] = v
    # rules 4' and 6'
    keys, lin, vedges = {}, {}, {}
    for k in all_keys:
        e = {(NIL, v) for (k2, v), w in writer.items() if k2 == k and node[w]}
        members = [t for t in range(n) if ok[t] and ((t, k) in ext_read or (t, k) in writes)]
        if wfr_keys:
            e |= {(ext_read[(t, k)], writes[(t, k)][-1]) for t in members if (t, k) in ext_read and (t, k) in writes}
        first = {t: ext_read[(t, k)] if (t, k) in ext_read else writes[(t, k)][-1] for t in members}
        last = {t: writes[(t, k)][-1] if (t, k) in writes else ext_read[(t, k)] for t in members}
        pairs = key_successors(members, txns)
        e |= {(last[a], first[b]) for a, b in pairs if last[a] != first[b]}
        vedges[k] = e
        on = REF._on_cycles(e)
        assert not on or on - {NIL}  # every cycle holds a non-nil value
        keys[k] = dict(base["keys"][k], cyclic=bool(on), cyc_value=min(on - {NIL}) if on else None)
        lin[k] = {"n_pairs": len(pairs), "n_touches": len(members), "n_vedges": len(e)}
    # rule 7'
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
            if (k, b) not in writer:  # nil or a phantom at the head
                continue
            w = writer[(k, b)]
            if (k, a) in writer:
                edge(writer[(k, a)], w, "ww", k)
            for (t, k2), v in ext_read.items():
                if k2 == k and v == a:
                    edge(t, w, "rw", k)
    # rule 9, as wr_ref.check has it
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
        full = REF._closure(matrix({"ww", "wr", "rw"}, True))
        reach = {(types, rt): REF._closure(matrix(set(types), rt))
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
                    cls = REF.CLASSES[tests.index(True) + (4 if rt else 0)]
            classes.append(cls)
    # rule 10 and the result map
    counts = dict(base["counts"])
    counts["cyclic-versions"] = sum(rec["cyclic"] for rec in keys.values())
    for c in REF.CLASSES:
        counts[c] = classes.count(c)
    totals = {"touches": sum(r["n_touches"] for r in lin.values()), "pairs": sum(r["n_pairs"] for r in lin.values()),
              "version-edges": sum(r["n_vedges"] for r in lin.values())}
    if not any(ok):
        valid, result = "unknown", dict(base["result"])
    else:
        keep = set(REF.READ_NAMES) | {"lost-update"}
        anomalies = {a: v for a, v in base["result"]["anomalies"].items() if a in keep}
        for k in all_keys:
            if keys[k]["cyclic"]:  # (the cycle is certified by the tests, not restated here)
                anomalies.setdefault("cyclic-versions", []).append({"key": k, "cycle": None})
        for c in classes:
            anomalies.setdefault(c, None)
        names = sorted(anomalies)
        valid = not names
        result = {"valid?": valid, "anomaly-types": names, "anomalies": anomalies, "not": {REF.NOT[a] for a in names}}
    result["linearizable-keys"] = totals
    return {"txns": txns, "read_flags": base["read_flags"], "txn_flags": base["txn_flags"], "keys": keys,
            "edges": edges, "rt_pred": base["rt_pred"], "sccs": sccs, "classes": classes, "counts": counts,
            "valid": valid, "result": result, "lin": lin, "lin_totals": totals, "vedges": vedges}
