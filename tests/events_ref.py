"""Shared pieces of the event tests (test_events.py, test_gpu_events.py): the
canonical renaming of value ids, random op-map histories, and builders of
event streams with every edge the device path has."""
import random

import numpy as np

from jepsen.etcd_amd import abi, events as E, history as H
from jepsen.etcd_amd.history import Tuple

INV, OK, FAIL, INFO = E.LC_EV_INVOKE, E.LC_EV_OK, E.LC_EV_FAIL, E.LC_EV_INFO
R, W, CAS = abi.LC_F_READ, abi.LC_F_WRITE, abi.LC_F_CAS


def tf(type_, fkw, bad=0):
    return type_ | fkw << 8 | bad << 16


def rename_ids(ops32, key_off, pinned=()):
    """Each key's value / expected ids renamed by first appearance in record
    order, a CAS's new value before its old one: history.pack's own interning
    order, so two packs of one history that differ only in how ids were
    handed out become equal.  `pinned` ids keep their number."""
    out = np.array(ops32, dtype=np.int32).reshape(-1, 6).copy()
    for k in range(len(key_off) - 1):
        ids = {i: i for i in pinned}
        for r in range(int(key_off[k]), int(key_off[k + 1])):
            for col in (1, 2):  # value, then expected
                v = int(out[r, col])
                if v < 0:
                    continue
                if v not in ids:
                    n = len(ids)
                    while n in ids.values():
                        n += 1
                    ids[v] = n
                out[r, col] = ids[v]
    return out


def host_pack_of_history(history, model="versioned-register", independent=True, init_value=None):
    """(keys, ops32, key_off, key_base, completion index or -1) of H.pack, as
    24-byte records."""
    keys, ops, key_off, done = H.pack(history, model=model, independent=independent,
                                      init_value=init_value)
    ops32, base = abi.pack32(ops, key_off)
    comp = np.array([d["completion"]["index"] if d["completion"] is not None else -1
                     for dk in done for d in dk], dtype=np.int64)
    return keys, ops32, key_off, base, comp


_BAD_VALUES = (5, [1, 2, 3], ["x", 1], [1, 7, 7], "oops")


def _value(rng, model, fk, type_):
    """A value of the model's shape for an op map of :f fk (or not: now and
    then a bad-shape one, or a version no state reaches)."""
    if model == "mutex":
        return None
    if rng.random() < 0.08:
        return rng.choice(_BAD_VALUES)
    v = rng.choice((None, 0, 1, 2, "a"))
    body = [rng.choice((0, 1, 2)), v] if fk == "cas" else v
    if model != "versioned-register":
        return body
    if type_ == "ok":
        ver = rng.choice((0, 1, 2, 3, 2 ** 40)) if rng.random() < 0.9 else None
    else:
        ver = None
    return [ver, body]


def random_history(rng, model, independent=True, max_events=14, n_procs=3, n_keys=2):
    """A tiny history with types drawn freely: orphan, repeated and missing
    completions and double invokes all occur; nemesis ops and bad-shape
    values are present.  A completion carries the :f of its process's open
    invoke on that key when there is one (Jepsen's own rule; the one case the
    event rules decide differently is tested by hand)."""
    fs = ("acquire", "release", "bogus") if model == "mutex" else ("read", "write", "cas", "bogus")
    hist, open_f = [], {}
    for _ in range(rng.randint(0, max_events)):
        if rng.random() < 0.12:
            hist.append({"type": "info", "f": "start-partition", "process": "nemesis",
                         "value": None})
            continue
        t = rng.choice(("invoke", "invoke", "ok", "ok", "fail", "info"))
        p, k = rng.randrange(n_procs), rng.randrange(n_keys)
        slot = (k if independent else 0, p)
        fk = rng.choice(fs)
        if t == "invoke":
            open_f[slot] = fk
        else:
            fk = open_f.pop(slot, fk)
        v = _value(rng, model, fk, t)
        hist.append({"type": t, "f": fk, "process": p, "value": Tuple(k, v) if independent else v})
    return hist


class Stream:
    """An event array under construction: rows (key, process, tf, value,
    expected, version)."""

    def __init__(self):
        self.rows = []

    def add(self, key, process=0, type_=INV, fkw=W, value=-1, expected=-1, version=-1, bad=0):
        self.rows.append((key, process, tf(type_, fkw, bad), value, expected, version))
        return len(self.rows) - 1

    def skip(self):
        self.rows.append((E.LC_EV_SKIP, 0, 0, 0, 0, 0))

    def array(self):
        return np.array(self.rows, dtype=np.int64).astype(np.int32).reshape(-1, 6)


def key_subhistory(n, key=0, straddler=7):
    """n events of one key (rows, to be placed by the caller): process
    `straddler` invokes at the last event of every 64-event chunk of the
    subhistory and completes at the first event of the next; the rest are
    write pairs by three other processes, each :ok carrying the next version,
    so the key is valid and the version-order tier decides it."""
    rows, version, filler = [], 0, 0
    open_fill = None
    for j in range(n):
        if j % 64 == 63:
            rows.append((key, straddler, tf(INV, W), 4, -1, -1))
        elif j % 64 == 0 and j > 0:
            version += 1
            rows.append((key, straddler, tf(OK, W), 4, -1, version))
        elif open_fill is None:
            open_fill = 10 + filler % 3
            filler += 1
            rows.append((key, open_fill, tf(INV, W), filler % 5, -1, -1))
        else:
            version += 1
            rows.append((key, open_fill, tf(OK, W), filler % 5, -1, version))
            open_fill = None
    return rows


def interleave(parts, seed=1):
    """One stream from several keys' row lists, each kept in its own order,
    merged at random."""
    rng = random.Random(seed)
    at = [0] * len(parts)
    left = [i for i, p in enumerate(parts) for _ in p]
    rng.shuffle(left)
    rows = []
    for i in left:
        rows.append(parts[i][at[i]])
        at[i] += 1
    return np.array(rows, dtype=np.int64).astype(np.int32).reshape(-1, 6)


def pairs_key(key, n_events, proc_base=0, n_procs=3):
    """n_events events of one key: write invoke / :ok pairs with rising
    versions by rotating processes (an odd last event is a pending invoke)."""
    rows, version = [], 0
    for j in range(n_events):
        p = proc_base + (j // 2) % n_procs
        if j % 2 == 0:
            rows.append((key, p, tf(INV, W), (j // 2) % 5, -1, -1))
        else:
            version += 1
            rows.append((key, p, tf(OK, W), (j // 2) % 5, -1, version))
    return rows
