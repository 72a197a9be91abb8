"""An independent restatement of the cycle screen (include/lincheck_screen.h)
for the tests, over op-level data: the txns as append_ref.transactions /
wr_ref.transactions give them ({"inv", "comp", "type"}) and the data edges as
a set of (from, to, type, key).  One boolean reachability closure over the data
edges plus the UNREDUCED interval order, as append_ref.py / wr_ref.py take it;
the two labels read straight off the closure; SCCs from mutual reachability;
the trim simulated on sets.  No rounds, no scans, no ranges, and no code shared
with jepsen/etcd_amd or the C sources.  Small graphs only: the closure is
cubic."""
import numpy as np

NO_COMP, NO_INV = 2 ** 31 - 1, -1
RT, TRIM = 1, 2


def _closure(a):
    """Transitive closure of a boolean adjacency matrix (paths of length >= 1)."""
    r = a.copy()
    while True:
        n = r | ((r.astype(np.uint8) @ r.astype(np.uint8)) > 0)
        if (n == r).all():
            return r
        r = n


def screen(txns, edges):
    """-> {"reach_lo", "reach_hi", "mark": lists per txn; "sccs": the nontrivial
    SCCs as frozensets, by least txn; "rt_sccs": those with a real-time edge
    inside; "survivors": what the trim leaves; "clean"}."""
    n = len(txns)
    ok = np.array([x["type"] == "ok" for x in txns], dtype=bool)
    node = np.array([x["type"] != "fail" for x in txns], dtype=bool)
    inv = np.array([x["inv"] for x in txns], dtype=np.int64)
    comp = np.array([x["comp"] if x["type"] == "ok" else NO_COMP for x in txns], dtype=np.int64)
    data = {(a, b) for a, b, _, _ in edges}
    assert all(node[a] and node[b] and a != b for a, b in data)
    # real time, unreduced: an OK txn before every node invoked after its completion
    rt = ok[:, None] & node[None, :] & (comp[:, None] < inv[None, :])
    adj = rt.copy()
    for a, b in data:
        adj[a, b] = True
    reach = _closure(adj) if n else adj
    at_most = reach | np.eye(n, dtype=bool)  # paths of >= 0 edges
    lo = np.where(at_most & ok[None, :], comp[None, :], NO_COMP).min(axis=1, initial=NO_COMP)
    hi = np.where(at_most & node[:, None], inv[:, None], NO_INV).max(axis=0, initial=NO_INV)
    lo = [int(lo[u]) if node[u] else NO_COMP for u in range(n)]
    hi = [int(hi[u]) if node[u] else NO_INV for u in range(n)]
    sccs, seen = [], set()
    for t in range(n):
        if t not in seen and reach[t, t]:
            s = frozenset(np.nonzero(reach[t, :] & reach[:, t])[0].tolist())
            seen |= s
            sccs.append(s)
    rt_sccs = [s for s in sccs if rt[np.ix_(sorted(s), sorted(s))].any()]
    flagged = {u for u in range(n) if node[u] and lo[u] < hi[u]}
    alive = {u for u in range(n) if node[u]} - flagged
    inside = {(a, b) for a, b in data if a in alive and b in alive and (lo[a], hi[a]) == (lo[b], hi[b])}
    while True:
        live = {(a, b) for a, b in inside if a in alive and b in alive}
        keep = {a for a, _ in live} & {b for _, b in live}
        if keep == alive:
            break
        alive = keep
    mark = [(RT if u in flagged else 0) | (TRIM if u in alive else 0) for u in range(n)]
    return {"reach_lo": lo, "reach_hi": hi, "mark": mark, "sccs": sccs, "rt_sccs": rt_sccs, "survivors": alive,
            "flagged": flagged, "clean": not sccs}


def category(ref):
    """Which of the batch's kinds a history is: (clean, rt-SCC only, data-only
    SCC only, both kinds, a trim survivor outside every SCC)."""
    in_scc = set().union(*ref["sccs"]) if ref["sccs"] else set()
    n_rt = len(ref["rt_sccs"])
    n_data = len(ref["sccs"]) - n_rt
    return {"clean": not ref["sccs"], "rt-only": n_rt > 0 and n_data == 0, "data-only": n_data > 0 and n_rt == 0,
            "both": n_rt > 0 and n_data > 0, "stray-survivor": bool(ref["survivors"] - in_scc)}
