"""An independent restatement of set-full (include/lincheck_setfull.h) for the
tests: jepsen's reduce as written.  It walks the op maps with a dict of element
states and updates EVERY element at each :ok read; no flat arrays, no table,
no bitmap.  `check` returns (element records in add order, the result map);
`random_history` makes the tiny histories the CPU tests compare on.
"""
import random
from collections import Counter

UNKNOWN = "unknown"


class Unsupported(ValueError):
    pass


def _kw(x):
    return x[1:] if isinstance(x, str) and x.startswith(":") else x


def _key(v):
    return (type(v).__name__, v) if not isinstance(v, (list, dict, set)) else repr(v)


def _client(op):
    p = op.get("process")
    return isinstance(p, int) and not isinstance(p, bool)


def _quantiles(xs):
    s = sorted(xs)
    n = len(s)
    if not n:
        return None
    # floor(n * p) with p as a fraction: 0, 1/2, 19/20, 99/100, 1
    return {p: s[min(n - 1, n * num // den)]
            for p, num, den in ((0, 0, 1), (0.5, 1, 2), (0.95, 19, 20), (0.99, 99, 100), (1, 1, 1))}


def _sorted(xs):
    try:
        return sorted(xs)
    except TypeError:
        return sorted(xs, key=repr)


def check(history, linearizable=True):
    elements = {}   # key -> state, in add order
    pending = {}    # process -> (position, op) of its pending read invoke
    phantoms = orphans = 0
    for pos, op in enumerate(history):
        if not _client(op):
            continue
        f, t = _kw(op.get("f")), _kw(op.get("type"))
        if f not in ("add", "read") or t not in ("invoke", "ok", "fail", "info"):
            continue
        if f == "add":
            k = _key(op.get("value"))
            if t == "invoke":
                if "time" not in op:
                    raise Unsupported(pos)
                if k in elements:
                    raise Unsupported(pos)
                elements[k] = {"element": op.get("value"), "known": None, "add-ok": False,
                               "last-present": None, "last-absent": None, "dup": 0}
            elif t == "ok" and k in elements and not elements[k]["add-ok"]:
                if "time" not in op:
                    raise Unsupported(pos)
                st = elements[k]
                st["add-ok"] = True
                if st["known"] is None:
                    st["known"] = (pos, op)
        else:
            p = op["process"]
            if t == "invoke":
                if "time" not in op:
                    raise Unsupported(pos)
                pending[p] = (pos, op)
            elif t == "fail":
                pending.pop(p, None)
            elif t == "ok":
                if p not in pending:
                    orphans += 1
                    continue
                if "time" not in op:
                    raise Unsupported(pos)
                inv = pending[p]
                seen = Counter(_key(x) for x in (op.get("value") or ()))
                for k, n in seen.items():
                    if k not in elements:  # names no element, or one added after this completion
                        phantoms += n
                    elif n > 1:
                        elements[k]["dup"] = max(elements[k]["dup"], n)
                for k, st in elements.items():
                    if k in seen:
                        if st["known"] is None:
                            st["known"] = (pos, op)
                        if st["last-present"] is None or inv[0] >= st["last-present"][0]:
                            st["last-present"] = inv
                    elif st["last-absent"] is None or inv[0] >= st["last-absent"][0]:
                        st["last-absent"] = inv
    records = []
    for st in elements.values():
        known, lp, la = st["known"], st["last-present"], st["last-absent"]
        kp = known[0] if known else -1
        lpp = lp[0] if lp else -1
        lap = la[0] if la else -1
        outcome = "never-read"
        if lp and lap < lpp:
            outcome = "stable"
        elif known and la and lpp < lap and kp < lap:
            outcome = "lost"
        stable_time = la[1]["time"] + 1 if la else 0
        lost_time = lp[1]["time"] + 1 if lp else 0
        kt = known[1]["time"] if known else 0
        sl = max(0, stable_time - kt) // 1000000 if outcome == "stable" else -1
        ll = max(0, lost_time - kt) // 1000000 if outcome == "lost" else -1
        records.append({"element": st["element"], "outcome": outcome, "stale": sl > 0,
                        "known_pos": kp, "last_present": lpp, "last_absent": lap,
                        "dup_max": st["dup"], "stable_latency_ms": sl, "lost_latency_ms": ll,
                        "known": known[1] if known else None, "last-absent": la[1] if la else None})
    by = lambda o: [r for r in records if r["outcome"] == o]  # noqa: E731
    stale = [r for r in records if r["stale"]]
    dups = [r for r in records if r["dup_max"]]
    if dups or by("lost"):
        valid = False
    elif not by("stable"):
        valid = UNKNOWN
    elif linearizable and stale:
        valid = False
    else:
        valid = True
    order = {id(r): i for i, r in enumerate(records)}
    worst = sorted(stale, key=lambda r: (-r["stable_latency_ms"], order[id(r)]))[:8]
    result = {
        "valid?": valid,
        "attempt-count": len(records),
        "stable-count": len(by("stable")),
        "lost-count": len(by("lost")),
        "lost": _sorted([r["element"] for r in by("lost")]),
        "never-read-count": len(by("never-read")),
        "never-read": _sorted([r["element"] for r in by("never-read")]),
        "stale-count": len(stale),
        "stale": _sorted([r["element"] for r in stale]),
        "worst-stale": [{"element": r["element"], "outcome": r["outcome"],
                         "stable-latency": r["stable_latency_ms"], "lost-latency": None,
                         "known": r["known"], "last-absent": r["last-absent"]} for r in worst],
        "stable-latencies": _quantiles([r["stable_latency_ms"] for r in by("stable")]),
        "lost-latencies": _quantiles([r["lost_latency_ms"] for r in by("lost")]),
        "duplicated-count": len(dups),
        "duplicated": {r["element"]: r["dup_max"] for r in dups},
        "phantom-count": phantoms,
        "orphan-read-count": orphans,
    }
    return records, result


FIELDS = ("known_pos", "last_present", "last_absent", "dup_max", "stable_latency_ms",
          "lost_latency_ms")
OUTCOME_CODE = {"never-read": 0, "stable": 1, "lost": 2}


def same_elements(records, out):
    """The reference's records against an lc_sf_element array: None, or the
    first difference."""
    if len(records) != len(out):
        return ("count", len(records), len(out))
    for e, r in enumerate(records):
        o = out[e]
        want = (OUTCOME_CODE[r["outcome"]], (1 if r["stale"] else 0) | (2 if r["dup_max"] else 0)) + \
            tuple(r[f] for f in FIELDS)
        got = (int(o["outcome"]), int(o["flags"])) + tuple(int(o[f]) for f in FIELDS)
        if want != got:
            return (e, r["element"], want, got)
    return None


def random_history(seed, max_elements=12, max_reads=16, max_procs=6, n_procs=None, full=False):
    """A tiny set history with everything the rules speak of: crashed and
    failed adds and reads, elements that are dropped and come back, late
    visibility (stale), phantoms, duplicates, nemesis ops, an :ok read without
    an invoke, two :ok of one read invoke.  full: max_elements adds and
    max_reads reads, not a draw of up to as many."""
    rng = random.Random(seed)
    n_procs = n_procs or rng.randint(1, max_procs)
    n_elements = rng.randint(0, max_elements)
    n_reads = rng.randint(0, max_reads)
    if full:
        n_elements, n_reads = max_elements, max_reads
    p_drop = rng.choice((0.0, 0.0, 0.15, 0.4))
    p_late = rng.choice((0.0, 0.3, 0.6))
    history, t = [], 0
    visible, late, dropped = set(), [], []
    busy = {}       # process -> its pending invoke
    next_element, adds_left, reads_left = 0, n_elements, n_reads

    def emit(**op):
        nonlocal t
        t += rng.choice((1, 50_000, 400_000, 1_100_000, 2_500_000))
        op["time"] = t
        history.append(op)

    steps = 0
    while (adds_left or reads_left or busy) and steps < 50 * (max_elements + max_reads + 4):
        steps += 1
        if rng.random() < 0.06:
            emit(process="nemesis", type="info", f=rng.choice(("kill", "start")), value=None)
        if late and rng.random() < 0.35:
            visible.add(late.pop(0))
        if visible and rng.random() < p_drop:
            x = rng.choice(sorted(visible))
            visible.discard(x)
            dropped.append(x)
        if dropped and rng.random() < 0.2:
            visible.add(dropped.pop(0))
        p = rng.randrange(n_procs)
        op = busy.get(p)
        if op is None:
            if adds_left and (not reads_left or rng.random() < 0.45):
                adds_left -= 1
                op = {"process": p, "f": "add", "value": next_element}
                next_element += 1
            elif reads_left:
                reads_left -= 1
                op = {"process": p, "f": "read", "value": None}
            else:
                continue
            busy[p] = op
            emit(type="invoke", **op)
            if op["f"] == "add" and rng.random() < 0.25:  # visible before it completes
                visible.add(op["value"])
            continue
        del busy[p]
        how = rng.choices(("ok", "fail", "info", "none"), (0.7, 0.1, 0.12, 0.08))[0]
        if op["f"] == "add":
            x = op["value"]
            if how in ("ok", "info") or (how == "none" and rng.random() < 0.5):
                if x not in visible:
                    (late.append if rng.random() < p_late else visible.add)(x)
            if how != "none":
                emit(process=p, f="add", value=x, type=how)
        else:
            if how == "ok":
                payload = sorted(visible)
                if rng.random() < 0.2:   # phantoms: an unknown value, an element not yet added
                    payload.append(rng.choice((1000 + rng.randrange(5), next_element + rng.randrange(3))))
                if payload and rng.random() < 0.15:  # duplicates
                    payload += [rng.choice(payload)] * rng.randint(1, 2)
                rng.shuffle(payload)
                emit(process=p, f="read", value=payload, type="ok")
                if rng.random() < 0.08:  # a second :ok of the same invoke
                    emit(process=p, f="read", value=sorted(visible), type="ok")
            elif how != "none":
                emit(process=p, f="read", value=None, type=how)
        if rng.random() < 0.02:  # an :ok read of a process that may have no pending invoke
            emit(process=rng.randrange(n_procs), f="read", value=sorted(visible), type="ok")
    return history
