"""Linearization orders from the witness search (LC_FLAG_SEARCH_WITNESS).

A key a search tier decided carries, with the flag, witness kind
LC_WITNESS_ORDER_FULL (valid) or LC_WITNESS_ORDER_PREFIX (invalid):
witness[r] is the rank of record r in a total order, -1 when r is left out
(include/lincheck.h, lc_aux).  `certify` is the product-side check of such an
order against the definition, from the records alone: one pass that steps the
model (register.clj:60-96) and keeps the largest call seen.  It shares
nothing with the device search that found the order.
"""
import numpy as np

LC_WITNESS_ORDER_FULL, LC_WITNESS_ORDER_PREFIX = 3, 4
_READ, _WRITE, _CAS = 0, 1, 2
_NIL = -1
_INF = (1 << 63) - 1


def order(records, witness):
    """The record indices of one key in rank order (ranked records only)."""
    w = np.asarray(witness, dtype=np.int64)
    if len(w) != len(records):
        raise ValueError("witness has %d entries for %d records" % (len(w), len(records)))
    idx = np.nonzero(w >= 0)[0]
    return idx[np.argsort(w[idx], kind="stable")].tolist()


def certify(records, witness, kind, cut=None, init=(0, _NIL)):
    """Is `witness` a linearization of one key's `records` ((n, 6): f, value,
    expected, version, call, ret)?  kind ORDER_FULL: of the whole history;
    ORDER_PREFIX: of the prefix at event `cut` (fail_prefix_end - 1) — records
    called after it must be absent, records returned by it present.  True only
    when the ranks are 0 .. L-1, each once, every required record is ranked,
    every step is legal from `init`, and every op returns after the largest
    call among the ops ranked before it."""
    if kind == LC_WITNESS_ORDER_FULL:
        cut = _INF - 1
    elif kind != LC_WITNESS_ORDER_PREFIX or cut is None:
        return False
    recs = [tuple(int(x) for x in r) for r in np.asarray(records, dtype=np.int64).reshape(-1, 6)]
    w = [int(x) for x in np.asarray(witness).reshape(-1)]
    if len(w) != len(recs):
        return False
    at = {}
    for r, rank in enumerate(w):
        f, _, _, _, call, ret = recs[r]
        if rank < 0:
            if ret <= cut:  # (ret == LC_INF is above every cut)
                return False
            continue
        if call > cut or rank in at:
            return False
        at[rank] = r
    if sorted(at) != list(range(len(at))):
        return False
    ver, val = init
    latest_call = None
    for rank in range(len(at)):
        f, value, expected, version, call, ret = recs[at[rank]]
        if latest_call is not None and ret <= latest_call:
            return False
        if f == _READ:
            if version != _NIL and version != ver:
                return False
            if value != _NIL and value != val:
                return False
        elif f == _WRITE or f == _CAS:
            if version != _NIL and version != ver + 1:
                return False
            if f == _CAS and expected != val:
                return False
            ver, val = ver + 1, value
        else:
            return False
        latest_call = call if latest_call is None else max(latest_call, call)
    return True
