"""Histories for the rw-register tests: a simulated register store with
linearization points and injected faults, scripted schedules for the rare
classes, and small hand-made shapes.  Op maps are Jepsen's with string keys:
{"type", "f": "txn", "value": [[f, k, v] ...], "process", "index"}; f is "w"
or "r"."""
import collections
import random

import numpy as np

from jepsen.etcd_amd import abi

FAULTS = ("stale", "split", "leak", "garble", "double")
SCRIPTED = ("behind", "skew", "g0", "g0rt", "loop")


class MarkedCall(abi._WrCall):
    """A call whose output arrays and summary are filled with a marker byte
    first, so that a call that must write nothing can be seen to have written
    nothing.  run(ctx=None) makes the call and returns its code."""
    MARK = -77

    def __init__(self, txns, mops, wfr_keys=True, edge_cap=None):
        super().__init__(txns, mops, wfr_keys, edge_cap)
        for a in self.arrays.values():
            a.view(np.int8)[...] = self.MARK
        self.summary.valid = self.MARK

    def run(self, ctx=None):
        if ctx is None:
            return abi.lib().lc_wr_check_host(*self.args())
        return abi.lib().lc_wr_check(ctx._h, *self.args())

    def arrays_untouched(self):
        return all((a.view(np.int8) == np.int8(self.MARK)).all() for a in self.arrays.values())

    def untouched(self):
        return self.summary.valid == self.MARK and self.arrays_untouched()


def op(typ, process, value, index):
    return {"type": typ, "f": "txn", "value": value, "process": process, "index": index}


def script(name, rng, ka, kb, fresh):
    """One scripted schedule on two keys of its own as [(type, process slot, mops)];
    fresh() gives values nobody else uses.
      behind  T2 = [r ka a][w ka b][w kb c] is pending while T3 reads c from kb and
              completes; then T1 starts, writes a to ka and completes; then T2
              completes, having read T1's a: T1 -wr-> T2 -wr-> T3 -rt-> T1 (G1c-realtime)
      skew    T0 reads ka as nil and kb as b over the whole schedule; B writes b
              and completes after T1, which reads kb as nil and started after A,
              the writer of ka, completed: T0 -rw-> A -rt-> T1 -rw-> B -wr-> T0
              (G2-item-realtime)
      g0      concurrent T1 = [r ka x2][w ka x1][w kb y1] and T2 = [r kb y1][w kb y2]
              [w ka x2]: ww both ways once wfr is inferred (G0), wr both ways (G1c)
      g0rt    T1 reads 2 from ka, writes 1 and completes; then T2 writes 2: ww
              (or wr) T2 -> T1 against real time (G0-realtime / G1c-realtime)
      loop    a version cycle of length 1, 2 or 3 on ka (txn i reads value i and
              writes value i + 1, the last one the first), half of the time with a
              txn below it that reads a cycle's value and writes a smaller one"""
    if name == "behind":
        a, b, c = fresh(), fresh(), fresh()
        t2 = [["r", ka, a], ["w", ka, b], ["w", kb, c]]
        return [("invoke", 0, t2), ("invoke", 1, [["r", kb, None]]), ("ok", 1, [["r", kb, c]]),
                ("invoke", 2, [["w", ka, a]]), ("ok", 2, [["w", ka, a]]), ("ok", 0, t2)]
    if name == "skew":
        a, b = fresh(), fresh()
        return [("invoke", 0, [["r", ka, None], ["r", kb, None]]), ("invoke", 1, [["w", kb, b]]),
                ("invoke", 2, [["w", ka, a]]), ("ok", 2, [["w", ka, a]]),
                ("invoke", 3, [["r", kb, None]]), ("ok", 3, [["r", kb, None]]),
                ("ok", 1, [["w", kb, b]]), ("ok", 0, [["r", ka, None], ["r", kb, b]])]
    if name == "g0":
        x1, x2, y1, y2 = fresh(), fresh(), fresh(), fresh()
        t1 = [["r", ka, x2], ["w", ka, x1], ["w", kb, y1]]
        t2 = [["r", kb, y1], ["w", kb, y2], ["w", ka, x2]]
        return [("invoke", 0, t1), ("invoke", 1, t2), ("ok", 0, t1), ("ok", 1, t2)]
    if name == "g0rt":
        v1, v2 = fresh(), fresh()
        t1 = [["r", ka, v2], ["w", ka, v1]]
        return [("invoke", 0, t1), ("ok", 0, t1), ("invoke", 1, [["w", ka, v2]]), ("ok", 1, [["w", ka, v2]])]
    assert name == "loop"
    below = fresh() if rng.random() < 0.5 else None
    n = rng.randint(1, 3)
    vals = [fresh() for _ in range(n)]
    txs = [[["r", ka, vals[i]], ["w", ka, vals[(i + 1) % n]]] for i in range(n)]
    if below is not None:
        txs.append([["r", ka, rng.choice(vals)], ["w", ka, below]])
    return [("invoke", i, t) for i, t in enumerate(txs)] + [("ok", i, t) for i, t in enumerate(txs)]


def random_history(seed, n_txns=12, n_keys=3, conc=4, faults=None, p_fault=0.45, p_info=0.08, p_fail=0.08,
                   sliding=False):
    """A register store serving `conc` processes.  Every txn takes effect at
    one point between its invoke and its completion unless a fault says
    otherwise:
      stale   a read answers with an earlier value of its key
      split   a txn's mops take effect one by one, other txns in between
      leak    a failed txn's writes take effect
      garble  a read answers with a value nobody wrote, or with an earlier value
              of its key although the txn itself has touched the key since
      double  a txn that reads a key and goes on to write it is admitted on the
              version the last such txn read
    and the schedules of script(), played on two keys of their own while no txn
    runs (once in a history of at most 16 txns), by processes drawn at random.
    faults: which of them may strike (None: a random choice per history).
    sliding: the n_keys live keys move on by one every four txns, as the
    reference's workload retires its keys."""
    rng = random.Random(seed)
    if faults is None:  # some histories have none, the others one or two
        faults = [] if rng.random() < 0.15 else rng.sample(FAULTS, rng.randint(1, 2))
        if rng.random() < 0.3:
            faults.append(rng.choice(SCRIPTED))
    faults = set(faults)
    runners = set(rng.sample(range(conc), 2)) if rng.random() < 0.34 else set()

    def strikes(f):
        return f in faults and rng.random() < p_fault

    store = {}
    past = collections.defaultdict(lambda: [None])  # earlier values of each key
    admitted = {}                                   # key -> what the last read-then-write txn read
    next_val = [1]
    history, procs, started = [], {}, 0             # process -> its running txn
    free = list(range(conc))
    next_proc = conc

    def fresh():
        next_val[0] += 1
        return next_val[0] - 1

    def apply_mop(x, i):
        f, k, v = x["mops"][i]
        mine = [j for j in range(i) if x["mops"][j][1] == k]
        if f == "w":
            store[k] = v
            past[k].append(v)
            return
        if mine:  # the txn's own latest view of the key
            got = x["mops"][mine[-1]][2] if x["mops"][mine[-1]][0] == "w" else x["result"][mine[-1]]
            if x["split"]:
                got = store.get(k)
        else:
            got = rng.choice(past[k]) if strikes("stale") else store.get(k)
            writes_later = any(m[0] == "w" and m[1] == k for m in x["mops"][i + 1:])
            if writes_later:
                if k in admitted and strikes("double"):
                    got = admitted[k]
                admitted[k] = got
        if strikes("garble"):
            got = 1000000 + fresh() if rng.random() < 0.5 else rng.choice(past[k])
        x["result"][i] = got

    def play_scripted():
        nonlocal started
        ka, kb = 1000000 + 2 * started, 1000001 + 2 * started
        ps = rng.sample(free, 4)
        for typ, p, mops in script(rng.choice(sorted(faults & set(SCRIPTED))), rng, ka, kb, fresh):
            history.append(op(typ, ps[p], [list(m) for m in mops], len(history)))
            started += typ == "invoke"

    scripted_left = 1 if n_txns <= 16 else n_txns
    while started < n_txns or procs:
        if not procs and len(free) >= 4 and n_txns - started >= 4 and scripted_left and faults & set(SCRIPTED) \
                and rng.random() < (1.0 if n_txns <= 16 else 0.5):
            scripted_left -= 1
            play_scripted()
            continue
        can_start = started < n_txns and free
        if can_start and (not procs or rng.random() < 0.45):
            p = free.pop(rng.randrange(len(free)))
            mops = []
            for _ in range(rng.randint(1, 4)):
                k = rng.randrange(n_keys) + (started // 4 if sliding else 0)
                mops.append(["w", k, fresh()] if rng.random() < 0.5 else ["r", k, None])
            r = rng.random()
            fate = "info" if r < p_info else "fail" if r < p_info + p_fail else "ok"
            x = {"mops": mops, "fate": fate, "at": 0, "result": {}, "process": p,
                 "lazy": 0.97 if p in runners else 0.85 if rng.random() < 0.35 else 0.4,  # how it lingers
                 "split": strikes("split"),
                 "effect": fate == "ok" or (fate == "info" and rng.random() < 0.6) or
                 (fate == "fail" and strikes("leak"))}
            procs[p] = x
            history.append(op("invoke", p, [list(m) for m in mops], len(history)))
            started += 1
            continue
        p = rng.choice(sorted(procs))
        x = procs[p]
        if x["at"] < len(x["mops"]) and (x["effect"] or x["fate"] == "ok"):
            for i in range(x["at"], x["at"] + 1 if x["split"] else len(x["mops"])):
                apply_mop(x, i)
                x["at"] = i + 1
            if x["at"] < len(x["mops"]):
                continue
        if rng.random() < x["lazy"]:
            continue
        del procs[p]
        if x["fate"] == "ok":
            value = [[f, k, x["result"].get(i, v)] for i, (f, k, v) in enumerate(x["mops"])]
            history.append(op("ok", p, value, len(history)))
            free.append(p)
        elif x["fate"] == "fail":
            history.append(op("fail", p, [list(m) for m in x["mops"]], len(history)))
            free.append(p)
        else:  # the process is gone; half of the time it says so
            if rng.random() < 0.5:
                history.append(op("info", p, [list(m) for m in x["mops"]], len(history)))
            free.append(next_proc)
            next_proc += 1
    return history


def sequential(n, n_keys=1):
    """n txns one after the other, each reading key i % n_keys and writing it."""
    h, cur = [], {}
    for i in range(n):
        k = i % n_keys
        h.append(op("invoke", 0, [["r", k, None], ["w", k, i + 1]], len(h)))
        h.append(op("ok", 0, [["r", k, cur.get(k)], ["w", k, i + 1]], len(h)))
        cur[k] = i + 1
    return h


def concurrent(n, n_keys=1):
    """n txns all invoked before any completes; they take effect in order."""
    h, cur, done = [], {}, []
    for i in range(n):
        h.append(op("invoke", i, [["r", i % n_keys, None], ["w", i % n_keys, i + 1]], len(h)))
    for i in range(n):
        k = i % n_keys
        done.append(op("ok", i, [["r", k, cur.get(k)], ["w", k, i + 1]], len(h) + i))
        cur[k] = i + 1
    return h + done
