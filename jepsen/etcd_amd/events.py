"""Jepsen op maps -> lc_event records (include/lincheck_events.h).

One pass over the history, one 24-byte record per op map, no per-key state:
the per-key split and the history completion that history.py does with dict
loops then run on the device (lc_check_events).  The encoder applies
history.py's client filter, tuple recognition and per-model field rules to
each op map on its own:

* a nemesis op (no integer :process), or a client op whose :type is none of
  invoke / ok / fail / info, is LC_EV_SKIP: it keeps its position;
* under `independent` a client op's value must be an independent tuple [k v];
  its key number is k's rank by first appearance (history.history_keys's
  order).  A non-tuple client op belongs to every key, which an event cannot
  say: `Unsupported` is raised and the caller takes the host path;
* fkw is the model's code for the op map's own :f (3: no step), the bad-shape
  bit says that its own value does not have the model's shape, and value /
  expected / version are its own value's fields, interned by ONE interner for
  the whole history (the init value first, so it is id 0; the mutex's ids are
  fixed).  A version outside [-1, 2^31-2] becomes 2^31-2, as lc_pack32 does.

One deliberate difference from history.pack: when an :ok completion's :f
differs from its invoke's, the record's f is 3 (history.py would take the
invoke's :f with the completion's value).  Jepsen writes no such history.
"""
import numpy as np

from . import history as H
from .abi import LC_NIL

LC_EV_SKIP = -1
LC_EV_INVOKE, LC_EV_OK, LC_EV_FAIL, LC_EV_INFO = 0, 1, 2, 3
TYPES = {"invoke": LC_EV_INVOKE, "ok": LC_EV_OK, "fail": LC_EV_FAIL, "info": LC_EV_INFO}
VERSION_NEVER = 0x7FFFFFFE  # lc_pack32: a version no state reaches


class Unsupported(ValueError):
    """The history cannot be written as events (a client op without an
    independent tuple under `independent`, a :process beyond int32)."""


def encode(history, model="versioned-register", independent=True, init_value=None):
    """history -> (events (n, 6) int32: key, process, tf, value, expected,
    version; keys in first-appearance order; the value table id -> value;
    index int64: op["index"] where present, else the position)."""
    if model not in H.MODELS:
        raise ValueError("unknown model %r (one of %s)" % (model, ", ".join(H.MODELS)))
    n = len(history)
    ev = np.zeros((n, 6), dtype=np.int32)
    ev[:, 0] = LC_EV_SKIP
    index = np.arange(n, dtype=np.int64)
    intern = H.Interner()
    if init_value is not None and model != "mutex":
        intern(init_value)
    key_ids = {}
    keys = [] if independent else [None]
    for pos, op in enumerate(history):
        if "index" in op:
            index[pos] = op["index"]
        value = op.get("value")
        k = 0
        if independent and isinstance(value, H.Tuple):
            k = key_ids.get(value.key)
            if k is None:
                k = key_ids[value.key] = len(keys)
                keys.append(value.key)
            value = value.value
            tupled = True
        else:
            tupled = False
        if not H.is_client(op):
            continue
        if independent and not tupled:
            raise Unsupported("client op %d has no independent tuple: it belongs to every key" % pos)
        t = TYPES.get(H._kw(op.get("type")))
        if t is None:
            continue
        p = op["process"]
        if not -2 ** 31 <= p < 2 ** 31:
            raise Unsupported("process %d of op %d does not fit 32 bits" % (p, pos))
        fk = H._kw(op.get("f"))
        if model == "mutex":
            fkw = H.LC_F_CAS if fk in ("acquire", "release") else H.F_UNKNOWN
        else:
            fkw = H.F_CODES.get(fk, H.F_UNKNOWN)
            if model == "register" and fkw == H.LC_F_CAS:
                fkw = H.F_UNKNOWN
        bad = 0
        v = e = ver = LC_NIL
        if fkw != H.F_UNKNOWN:
            f, v, e, ver = H._record(model, fk, value, intern)
            if f == H.F_UNKNOWN:
                bad = 1
            elif not -1 <= ver <= VERSION_NEVER:
                ver = VERSION_NEVER
        ev[pos] = (k, p, t | fkw << 8 | bad << 16, v, e, ver)
    return ev, keys, intern.values, index
