"""lc_check_events without a GPU: the event record, the encoder
(jepsen/etcd_amd/events.py) and the rules on the host (lc_events_pack_host)
against history.pack."""
import ctypes
import errno
import random

import numpy as np
import pytest

import events_ref as ER
from jepsen.etcd_amd import abi, events as E, history as H, synth
from jepsen.etcd_amd.history import Tuple


def test_struct_and_symbols():
    assert ctypes.sizeof(abi.LcEvent) == 24 and abi.as_events(np.zeros((3, 6))).strides == (24, 4)
    lib = ctypes.CDLL(abi.LIB_PATH)
    for name in ("lc_events_pack_host", "lc_events_pack", "lc_check_events", "lc_last_events_stats",
                 "lc_events_limits"):
        assert hasattr(lib, name), name
    assert abi.lib().lc_abi_version() == 5
    lim = abi.events_limits()
    assert lim["max_lds_events"] >= 64 and lim["lds_process_capacity"] >= 64
    assert ctypes.sizeof(abi.LcEventsOut) == 48 and ctypes.sizeof(abi.LcEventsStats) == 80


def _same_as_history_pack(hist, model, independent=True, init_value=None):
    ev, keys, _values, index = E.encode(hist, model, independent, init_value)
    ops32, key_off, key_base, completion = abi.pack_events_host(ev, len(keys))
    rkeys, rops32, rkey_off, rbase, rcomp = ER.host_pack_of_history(hist, model, independent,
                                                                    init_value)
    assert keys == rkeys
    assert (key_off == rkey_off).all() and (key_base == rbase).all()
    if model == "mutex":  # fixed ids: nothing to rename
        assert (ops32 == rops32).all()
    else:
        pinned = (0,) if init_value is not None else ()
        assert (ER.rename_ids(ops32, key_off, pinned) == ER.rename_ids(rops32, rkey_off, pinned)).all()
    assert (completion == rcomp).all()
    assert (index == np.arange(len(hist))).all()
    return len(ops32)


@pytest.mark.parametrize("model", H.MODELS)
def test_host_pack_matches_history_pack_on_jepsen_history(model):
    hist, _ = synth.jepsen_history(40, 150, p_info=0.05, p_anomaly=0.3, seed=77)
    if model != "versioned-register":
        # the same op maps with the other models' value shapes: [version x] -> x
        fmap = {"read": "release", "write": "acquire", "cas": "acquire"}
        new = []
        for op in hist:
            op = dict(op)
            if isinstance(op.get("value"), Tuple):
                k, v = op["value"]
                op["value"] = Tuple(k, None if model == "mutex" else v[1])
                if model == "mutex":
                    op["f"] = fmap[op["f"]]
            new.append(op)
        hist = new
    assert _same_as_history_pack(hist, model) > 1000


def test_host_pack_matches_history_pack_with_init_value():
    hist, _ = synth.jepsen_history(10, 100, p_info=0.05, seed=78)
    assert _same_as_history_pack(hist, "versioned-register", init_value=3) > 100


def test_host_pack_matches_history_pack_not_independent():
    hist, _ = synth.jepsen_history(1, 300, p_info=0.05, seed=79)
    flat = []
    for op in hist:
        op = dict(op)
        if isinstance(op.get("value"), Tuple):
            op["value"] = op["value"].value
        flat.append(op)
    assert _same_as_history_pack(flat, "versioned-register", independent=False) > 100


@pytest.mark.parametrize("model", H.MODELS)
def test_host_pack_matches_history_pack_on_random_tiny_histories(model):
    rng = random.Random(1234)
    n_ops = 0
    for i in range(2000):
        independent = i % 4 != 3
        n_ops += _same_as_history_pack(ER.random_history(rng, model, independent), model, independent)
    assert n_ops > 2000  # the histories are not degenerate


def test_completion_f_differs_from_invoke_gives_unknown_f():
    """Rule 4's deliberate difference from history.pack."""
    hist = [{"type": "invoke", "f": "write", "process": 0, "value": Tuple("k", [None, 3])},
            {"type": "ok", "f": "read", "process": 0, "value": Tuple("k", [1, 3])},
            {"type": "invoke", "f": "read", "process": 0, "value": Tuple("k", [None, None])},
            {"type": "ok", "f": "read", "process": 0, "value": Tuple("k", [1, 3])}]
    ev, keys, _, _ = E.encode(hist)
    ops32, key_off, key_base, completion = abi.pack_events_host(ev, len(keys))
    assert ops32.tolist() == [[3, -1, -1, -1, 0, 1], [abi.LC_F_READ, 0, -1, 1, 2, 3]]
    assert key_off.tolist() == [0, 2] and key_base.tolist() == [0] and completion.tolist() == [1, 3]
    # history.pack keeps the invoke's :f with the completion's value
    assert H.pack(hist)[1][0].tolist()[:4] == [abi.LC_F_WRITE, 0, -1, 1]


def test_encode_unsupported_and_index():
    hist = [{"type": "invoke", "f": "read", "process": 0, "value": Tuple(5, [None, None])},
            {"type": "info", "f": "start", "process": "nemesis", "value": None},
            {"type": "ok", "f": "read", "process": 0, "value": Tuple(5, [0, None])}]
    hist = [dict(op, index=3 * i + 7) for i, op in enumerate(hist)]
    ev, keys, values, index = E.encode(hist)
    assert keys == [5] and index.tolist() == [7, 10, 13]
    assert ev[:, 0].tolist() == [0, E.LC_EV_SKIP, 0]
    with pytest.raises(E.Unsupported):
        E.encode(hist + [{"type": "invoke", "f": "read", "process": 1, "value": [None, None]}])
    # without jepsen.independent the same op is fine
    ev, keys, _, _ = E.encode([{"type": "invoke", "f": "read", "process": 1, "value": [None, None]}],
                              independent=False)
    assert keys == [None] and ev[0, 0] == 0


def test_host_pack_arguments():
    s = ER.Stream()
    s.add(0, 1, ER.INV)
    s.add(0, 1, ER.OK, version=1)
    good = s.array()
    assert len(abi.pack_events_host(good, 1)[0]) == 1
    for col, val in ((0, 1), (0, -2), (2, 4), (2, ER.tf(ER.INV, ER.W) | 0x80)):
        bad = good.copy()
        bad[1, col] = val
        with pytest.raises(abi.LcError) as e:
            abi.pack_events_host(bad, 1)
        assert e.value.code == -errno.EINVAL
    # nothing at all, and keys without events
    ops32, key_off, key_base, completion = abi.pack_events_host(np.zeros((0, 6), np.int32), 0)
    assert len(ops32) == 0 and key_off.tolist() == [0] and len(key_base) == 0
    ops32, key_off, key_base, completion = abi.pack_events_host(np.zeros((0, 6), np.int32), 3)
    assert len(ops32) == 0 and key_off.tolist() == [0, 0, 0, 0] and key_base.tolist() == [0, 0, 0]
    # a key whose only pair failed is an empty key
    s = ER.Stream()
    s.add(1, 1, ER.INV, ER.CAS, 1, 2)
    s.skip()
    s.add(1, 1, ER.FAIL, ER.CAS, 1, 2)
    ops32, key_off, key_base, completion = abi.pack_events_host(s.array(), 2)
    assert len(ops32) == 0 and key_off.tolist() == [0, 0, 0]
