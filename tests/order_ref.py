"""Test-side certifier of LC_WITNESS_ORDER_FULL / LC_WITNESS_ORDER_PREFIX
witnesses (include/lincheck.h, lc_aux), and an exhaustive search for an order.

TEST INFRASTRUCTURE ONLY.  Written from the definition over oracle.brute.step
and the real-time rule; it shares no code with jepsen/etcd_amd/witness.py (the
product-side check), and the tests compare the two with each other.

An order of one key's records at event `cut` (None: the whole history):
  * ranks 0 .. L-1, each used once; -1 = left out;
  * a record called after `cut` is left out, a record returned by `cut` is in
    (without a cut: every :ok record is in);
  * stepping the model in rank order never becomes inconsistent;
  * real time: every op returns after the call of every op ranked before it.
"""
import numpy as np

from oracle import brute

INF = (1 << 63) - 1


def certify(records, witness, cut=None, init=(0, -1)):
    recs = np.asarray(records, dtype=np.int64).reshape(-1, 6)
    w = np.asarray(witness, dtype=np.int64).reshape(-1)
    if len(w) != len(recs):
        return False
    if cut is None:
        cut = INF - 1
    inside = w >= 0
    if (inside & (recs[:, 4] > cut)).any() or (~inside & (recs[:, 5] <= cut)).any():
        return False
    L = int(inside.sum())
    if sorted(w[inside].tolist()) != list(range(L)):
        return False
    seq = np.nonzero(inside)[0][np.argsort(w[inside])]
    calls, rets = recs[seq, 4], recs[seq, 5]
    # real time, all pairs at once: op j against the latest call before it
    if L > 1 and (rets[1:] <= np.maximum.accumulate(calls)[:-1]).any():
        return False
    state = init
    for r in seq:
        op = tuple(int(x) for x in recs[r])
        if op[0] not in (brute.READ, brute.WRITE, brute.CAS):
            return False
        state = brute.step(state, op)
        if state is None:
            return False
    return True


def find_order(records, cut=None, init=(0, -1)):
    """Some witness of the records at `cut` (None: whole history), or None when
    there is none: every order is tried (plain backtracking over the
    definition, no memo, no reductions) — for keys of at most ~8 ops."""
    recs = [tuple(int(x) for x in r) for r in records]
    n = len(recs)
    if cut is None:
        cut = INF - 1
    need = [i for i in range(n) if recs[i][5] <= cut]
    may = [i for i in range(n) if recs[i][4] <= cut]
    order = []

    def go(state, used, latest):
        if all(i in used for i in need):
            return True
        for i in may:
            if i in used or (order and recs[i][5] <= latest):
                continue
            nxt = brute.step(state, recs[i])
            if nxt is None:
                continue
            order.append(i)
            if go(nxt, used | {i}, max(latest, recs[i][4])):
                return True
            order.pop()
        return False

    if not go(init, frozenset(), -1):
        return None
    w = [-1] * n
    for rank, i in enumerate(order):
        w[i] = rank
    return w
