"""Histories for the list-append tests: a simulated list store with
linearization points and injected faults, and small hand-made shapes.  Op maps
are Jepsen's with string keys: {"type", "f": "txn", "value": [[f, k, v] ...],
"process", "index"}; f is "append" or "r"."""
import collections
import random

import numpy as np

from jepsen.etcd_amd import abi

FAULTS = ("stale", "split", "insert", "drop", "garble", "leak")
SCRIPTED = ("behind", "skew")


class MarkedCall(abi._AppendCall):
    """A call whose output arrays and summary are filled with a marker byte
    first, so that a call that must write nothing can be seen to have written
    nothing.  run(ctx=None) makes the call and returns its code."""
    MARK = -77

    def __init__(self, txns, mops, values):
        super().__init__(txns, mops, values)
        for a in self.arrays.values():
            a.view(np.int8)[...] = self.MARK
        self.summary.valid = self.MARK

    def run(self, ctx=None):
        if ctx is None:
            return abi.lib().lc_append_check_host(*self.args())
        return abi.lib().lc_append_check(ctx._h, *self.args())

    def untouched(self):
        return self.summary.valid == self.MARK and \
            all((a.view(np.int8) == np.int8(self.MARK)).all() for a in self.arrays.values())


def op(typ, process, value, index):
    return {"type": typ, "f": "txn", "value": value, "process": process, "index": index}


def random_history(seed, n_txns=12, n_keys=3, conc=4, faults=None, p_fault=0.45, p_info=0.08, p_fail=0.08,
                   sliding=False):
    """A list store serving `conc` processes.  Every txn takes effect at one
    point between its invoke and its completion unless a fault says otherwise:
      stale   a read answers from an earlier state of its key
      split   a txn's mops take effect one by one, other txns in between
      insert  an append lands inside the list, not at its end
      drop    an acknowledged append is lost
      garble  a read answers with two entries swapped, one repeated, or one nobody wrote
      leak    a failed txn's appends take effect
    and two faults that are a schedule, played on two keys of their own while
    no txn runs (once in a history of at most 16 txns), by four processes
    drawn at random, the keys holding up to two earlier elements each:
      behind  a long txn's appends show before it completes; a txn that starts
              after a reader of them has completed is ordered before them
      skew    a long txn reads one key before and another key after two
              short writers, one of which a third reader misses
    faults: which of them may strike (None: a random choice per history).
    sliding: the n_keys live keys move on by one every four txns, as the
    reference's workload retires its keys."""
    rng = random.Random(seed)
    if faults is None:  # some histories have none, the others one or two
        faults = [] if rng.random() < 0.15 else rng.sample(FAULTS, rng.randint(1, 2))
        if rng.random() < 0.08:
            faults.append(rng.choice(SCRIPTED))
    faults = set(faults)
    # in a third of the histories the txns of two processes complete very late:
    # long txns that many short ones overlap
    runners = set(rng.sample(range(conc), 2)) if rng.random() < 0.34 else set()

    def strikes(f):
        return f in faults and rng.random() < p_fault

    store = collections.defaultdict(list)
    past = collections.defaultdict(lambda: [[]])  # earlier states of each key
    next_elem = [1]
    pending_elems = set()                     # appended by txns that have not completed
    history, procs, started = [], {}, 0       # process -> its running txn
    free = list(range(conc))
    next_proc = conc

    def apply_mop(x, i):
        f, k, v = x["mops"][i]
        if f == "append":
            if strikes("drop"):
                return
            at = len(store[k])
            if strikes("insert"):  # anywhere; half of the time before the first entry of a txn still running
                at = rng.randrange(len(store[k]) + 1)
                running = [j for j, e in enumerate(store[k]) if e in pending_elems]
                if running and rng.random() < 0.5:
                    at = running[0]
            pending_elems.add(v)
            store[k] = store[k][:at] + [v] + store[k][at:]
            past[k].append(list(store[k]))
        else:
            got = list(rng.choice(past[k]) if strikes("stale") else store[k])
            if strikes("garble"):
                kind = rng.randrange(3)
                if kind == 0 and len(got) >= 2:
                    a, b = rng.sample(range(len(got)), 2)
                    got[a], got[b] = got[b], got[a]
                elif kind == 1 and got:
                    got.insert(rng.randrange(len(got) + 1), rng.choice(got))
                else:
                    got.insert(rng.randrange(len(got) + 1), 1000000 + next_elem[0])
                    next_elem[0] += 1
            x["result"][i] = got

    def play_scripted():
        """One of the scripted faults, on two keys nobody else uses, while no txn runs."""
        nonlocal started
        ka, kb = 1000000 + 2 * started, 1000001 + 2 * started
        a, b, c = range(next_elem[0], next_elem[0] + 3)
        next_elem[0] += 3
        p0, p1, p2, p3 = rng.sample(free, 4)
        # what the two keys hold beforehand: up to two elements each, from one earlier txn
        xs = list(range(next_elem[0], next_elem[0] + rng.randrange(3)))
        ys = list(range(next_elem[0] + 2, next_elem[0] + 2 + rng.randrange(3)))
        next_elem[0] += 4
        script = []
        if xs or ys:
            first = [["append", ka, x] for x in xs] + [["append", kb, y] for y in ys]
            script += [("invoke", p3, first), ("ok", p3, first)]
        if rng.choice(sorted(faults & set(SCRIPTED))) == "behind":
            script += [("invoke", p0, [["append", ka, b], ["append", kb, c]]), ("invoke", p1, [["r", kb, None]]),
                       ("ok", p1, [["r", kb, ys + [c]]]), ("invoke", p2, [["append", ka, a]]),
                       ("ok", p2, [["append", ka, a]]), ("ok", p0, [["append", ka, b], ["append", kb, c]]),
                       ("invoke", p3, [["r", ka, None]]), ("ok", p3, [["r", ka, xs + [a, b]]])]
        else:
            script += [("invoke", p0, [["r", ka, None], ["r", kb, None]]), ("invoke", p1, [["append", kb, b]]),
                       ("invoke", p2, [["append", ka, a]]), ("ok", p2, [["append", ka, a]]),
                       ("invoke", p3, [["r", kb, None]]), ("ok", p3, [["r", kb, list(ys)]]),
                       ("ok", p1, [["append", kb, b]]), ("ok", p0, [["r", ka, list(xs)], ["r", kb, ys + [b]]]),
                       ("invoke", p2, [["r", ka, None], ["r", kb, None]]),
                       ("ok", p2, [["r", ka, xs + [a]], ["r", kb, ys + [b]]])]
        for typ, p, mops in script:
            history.append(op(typ, p, mops, len(history)))
            started += typ == "invoke"

    scripted_left = 1 if n_txns <= 16 else n_txns
    while started < n_txns or procs:
        if not procs and len(free) >= 4 and n_txns - started >= 6 and scripted_left and faults & set(SCRIPTED) \
                and rng.random() < (1.0 if n_txns <= 16 else p_fault / 2):
            scripted_left -= 1
            play_scripted()
            continue
        can_start = started < n_txns and free
        if can_start and (not procs or rng.random() < 0.45):
            p = free.pop(rng.randrange(len(free)))
            mops = []
            for _ in range(rng.randint(1, 4)):
                k = rng.randrange(n_keys) + (started // 4 if sliding else 0)
                if rng.random() < 0.5:
                    mops.append(["append", k, next_elem[0]])
                    next_elem[0] += 1
                else:
                    mops.append(["r", k, None])
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
        if x["effect"] and x["at"] < len(x["mops"]):
            for i in range(x["at"], x["at"] + 1 if x["split"] else len(x["mops"])):
                apply_mop(x, i)
                x["at"] = i + 1
            if x["at"] < len(x["mops"]):
                continue
        if rng.random() < x["lazy"]:
            continue
        del procs[p]
        pending_elems.difference_update(v for f, _, v in x["mops"] if f == "append")
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
    """n txns one after the other, each appending to key i % n_keys and reading it back."""
    h, lists = [], {k: [] for k in range(n_keys)}
    for i in range(n):
        k = i % n_keys
        h.append(op("invoke", 0, [["append", k, i + 1], ["r", k, None]], len(h)))
        lists[k] = lists[k] + [i + 1]
        h.append(op("ok", 0, [["append", k, i + 1], ["r", k, list(lists[k])]], len(h)))
    return h


def concurrent(n, n_keys=1):
    """n txns all invoked before any completes."""
    h, lists, done = [], {k: [] for k in range(n_keys)}, []
    for i in range(n):
        h.append(op("invoke", i, [["append", i % n_keys, i + 1], ["r", i % n_keys, None]], len(h)))
    for i in range(n):
        k = i % n_keys
        lists[k] = lists[k] + [i + 1]
        done.append(op("ok", i, [["append", k, i + 1], ["r", k, list(lists[k])]], len(h) + i))
    return h + done
