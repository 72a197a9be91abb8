"""set-full on the host: lc_set_full_host and SetFullChecker(device=False)
against the independent reference (setfull_ref.py) on hand-derived histories
and on random tiny ones; the encoder's rules; every -EINVAL case."""
import errno
import json
import os

import numpy as np
import pytest

import setfull_ref as REF
from jepsen.etcd_amd import abi, checker, setfull as SF

KATS = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "setfull_kat.json")))
N_RANDOM, SEED = 2000, 0x5E7F0000


def _host(history, linearizable=True):
    enc = SF.encode(history)
    out, s = abi.set_full_host(enc.adds, enc.reads, enc.values, linearizable)
    return enc, out, s


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(kat):
    lin = kat["linearizable"]
    want = [dict(e, stale=bool(e["flags"] & 1)) for e in kat["elements"]]
    # the reference against the hand derivation
    records, result = REF.check(kat["history"], lin)
    for r, w in zip(records, want):
        assert {k: r[k] for k in w if k != "flags"} == {k: w[k] for k in w if k != "flags"}, kat["name"]
    assert len(records) == len(want)
    assert result["valid?"] == kat["valid"] and result["phantom-count"] == kat["n_phantom"]
    # the library against both
    enc, out, s = _host(kat["history"], lin)
    assert REF.same_elements(records, out) is None
    assert [int(f) for f in out["flags"]] == [e["flags"] for e in kat["elements"]]
    assert {1: True, 0: False, -1: "unknown"}[s["valid"]] == kat["valid"]
    assert s["n_phantom"] == kat["n_phantom"] and s["n_tiles"] == 0
    assert SF.SetFullChecker(linearizable=lin, device=False).check({}, kat["history"], {}) == result


@pytest.fixture(scope="module")
def batch():
    hs = [REF.random_history(SEED + i) for i in range(N_RANDOM)]
    return [(h, i % 5 != 0, REF.check(h, i % 5 != 0)) for i, h in enumerate(hs)]


def test_random_batch_has_every_case(batch):
    """From the reference alone: the batch is worth comparing on."""
    n = dict.fromkeys(("stable", "lost", "never-read", "stale", "duplicated", "phantom"), 0)
    for _, _, (records, result) in batch:
        for r in records:
            n[r["outcome"]] += 1
            n["stale"] += r["stale"]
            n["duplicated"] += r["dup_max"] > 0
        n["phantom"] += result["phantom-count"]
    assert all(v >= 50 for v in n.values()), n
    valids = {str(result["valid?"]) for _, _, (_, result) in batch}
    assert valids == {"True", "False", "unknown"}
    assert sum(result["orphan-read-count"] for _, _, (_, result) in batch) >= 20


def test_random_host_against_reference(batch):
    for i, (h, lin, (records, result)) in enumerate(batch):
        enc, out, s = _host(h, lin)
        assert REF.same_elements(records, out) is None, (i, REF.same_elements(records, out))
        assert s["n_phantom"] == result["phantom-count"], i
        assert (s["n_elements"], s["n_stable"], s["n_lost"], s["n_never_read"], s["n_stale"],
                s["n_duplicated"]) == (
            len(records), result["stable-count"], result["lost-count"], result["never-read-count"],
            result["stale-count"], result["duplicated-count"]), i
        assert s["linearizable"] == int(lin)


def test_random_checker_against_reference(batch):
    for i, (h, lin, (_, result)) in enumerate(batch):
        got = SF.SetFullChecker(linearizable=lin, device=False).check({}, h, {})
        assert got == result, (i, {k: (got[k], result[k]) for k in result if got[k] != result[k]})


def _op(p, t, f, v, time=0, **kw):
    return dict({"process": p, "type": t, "f": f, "value": v, "time": time}, **kw)


def test_encoder_rule_2():
    h = [
        _op(0, "invoke", "add", 7, 1),       # 0
        _op(1, "ok", "read", [7], 2),        # 1  no pending invoke: ignored and counted
        _op(1, "invoke", "read", None, 3),   # 2
        _op(1, "invoke", "read", None, 4),   # 3  the latest invoke is the pending one
        _op(1, "info", "read", None, 5),     # 4  :info leaves it pending
        _op(1, "ok", "read", [7], 6),        # 5  paired with 3
        _op(1, "ok", "read", [], 7),         # 6  an :ok does not clear it: paired with 3 again
        _op(1, "fail", "read", None, 8),     # 7  clears it
        _op(1, "ok", "read", [7], 9),        # 8  ignored and counted
        _op("nemesis", "info", "read", [7], 10),  # 9  not a client op
        _op(2, "invoke", "read", None, 11),  # 10
        _op(2, "fail", "read", None, 12),    # 11
        _op(2, "invoke", "read", None, 13),  # 12
        _op(2, "ok", "read", [7, 8], 14),    # 13 paired with 12
        _op(0, "ok", "add", 7, 15),          # 14
        _op(0, "ok", "add", 8, 16),          # 15 no add invoke of 8: ignored
    ]
    enc = SF.encode(h)
    assert enc.n_orphan_reads == 2 and enc.elements == [7]
    assert enc.adds.tolist() == [(7, 15, 0, 14)]
    assert [(r["inv_pos"], r["ok_pos"], r["inv_time"], r["ok_time"], r["off"], r["len"])
            for r in enc.reads] == [(3, 5, 4, 6, 0, 1), (3, 6, 4, 7, 1, 0), (12, 13, 13, 14, 1, 2)]
    assert enc.values.tolist() == [7, 7, 8]
    records, result = REF.check(h)
    assert REF.same_elements(records, _host(h)[1]) is None
    assert result["orphan-read-count"] == 2 and result["phantom-count"] == 1
    # the element is seen by 5, missed by 6 (the same invoke) and seen by 13
    assert (records[0]["last_present"], records[0]["last_absent"], records[0]["known_pos"]) == (12, 3, 5)


def test_encoder_rule_9():
    two = [_op(0, "invoke", "add", 1, 1), _op(0, "fail", "add", 1, 2), _op(0, "invoke", "add", 1, 3)]
    with pytest.raises(SF.Unsupported):
        SF.encode(two)
    with pytest.raises(REF.Unsupported):
        REF.check(two)
    for bad in ([{"process": 0, "type": "invoke", "f": "add", "value": 1}],
                [{"process": 0, "type": "invoke", "f": "read", "value": None}],
                [_op(0, "invoke", "read", None, 1), {"process": 0, "type": "ok", "f": "read", "value": []}],
                [_op(0, "invoke", "add", 1, 1), {"process": 0, "type": "ok", "f": "add", "value": 1}]):
        with pytest.raises(SF.Unsupported):
            SF.encode(bad)
        with pytest.raises(REF.Unsupported):
            REF.check(bad)
    # check_safe turns it into jepsen's {:valid? :unknown}
    r = checker.check_safe(SF.SetFullChecker(device=False), {}, two)
    assert r["valid?"] == "unknown" and "Unsupported" in r["error"]
    # keyword spellings, :index and a nemesis op do not matter
    h = [{"process": 0, "type": ":invoke", "f": ":add", "value": 1, "time": 1, "index": 10},
         {"process": "nemesis", "type": "info", "f": "kill"},
         {"process": 0, "type": ":ok", "f": ":add", "value": 1, "time": 2, "index": 12}]
    enc = SF.encode(h)
    assert enc.adds.tolist() == [(1, 2, 0, 2)] and enc.index.tolist() == [10, 1, 12]


def test_encoder_non_integer_elements():
    def h(a, b, ghost):
        return [_op(0, "invoke", "add", a, 1), _op(0, "ok", "add", a, 2),
                _op(0, "invoke", "add", b, 3), _op(0, "ok", "add", b, 4),
                _op(1, "invoke", "read", None, 5), _op(1, "ok", "read", [b, ghost, a, b], 6)]
    ints = SF.encode(h(5, -9, 77))
    assert ints.adds["value"].tolist() == [5, -9] and ints.values.tolist() == [-9, 77, 5, -9]
    for a, b, ghost in (("x", "y", "z"), (5, "5", 6), (1, True, 2), (1.5, 2, 3), ((1, 2), (1, 3), 4),
                        (2 ** 63, 1, 2), (-2 ** 63, 1, 2), (1, 2, -2 ** 63)):
        hist = h(a, b, ghost)
        enc = SF.encode(hist)
        assert enc.elements == [a, b]
        assert enc.adds["value"].tolist() == [0, 1] and enc.values.tolist() == [1, 2, 0, 1]
        records, result = REF.check(hist)
        assert SF.SetFullChecker(device=False).check({}, hist, {}) == result
        assert result["duplicated"] == {b: 2} and result["phantom-count"] == 1


def _arrays(adds, reads, values):
    return (np.array(adds, dtype=abi.SF_ADD_DTYPE), np.array(reads, dtype=abi.SF_READ_DTYPE),
            np.array(values, dtype=np.int64))


# (value, ok_time, inv_pos, ok_pos) / (inv_time, ok_time, off, inv_pos, ok_pos, len, pad)
GOOD = ([(1, 0, 0, 1), (2, 0, 2, -1)], [(0, 0, 0, 3, 4, 2, 0), (0, 0, 1, 5, 6, 1, 0)], [1, 2])
EINVAL_CASES = {
    "adds-not-ascending": ([(1, 0, 2, 3), (2, 0, 2, -1)], GOOD[1], GOOD[2]),
    "adds-descending": ([(1, 0, 2, 3), (2, 0, 1, -1)], GOOD[1], GOOD[2]),
    "two-adds-of-one-value": ([(1, 0, 0, 1), (1, 0, 2, -1)], GOOD[1], GOOD[2]),
    "add-value-reserved": ([(-2 ** 63, 0, 0, 1)], GOOD[1], GOOD[2]),
    "add-ok-before-invoke": ([(1, 0, 5, 5)], GOOD[1], GOOD[2]),
    "add-position-negative": ([(1, 0, -1, 1)], GOOD[1], GOOD[2]),
    "add-position-too-large": ([(1, 0, 2 ** 31 - 1, -1)], GOOD[1], GOOD[2]),
    "add-ok-position-too-large": ([(1, 0, 0, 2 ** 31 - 1)], GOOD[1], GOOD[2]),
    "reads-not-ascending": (GOOD[0], [(0, 0, 0, 3, 4, 2, 0), (0, 0, 1, 2, 4, 1, 0)], GOOD[2]),
    "read-invoke-not-before-ok": (GOOD[0], [(0, 0, 0, 4, 4, 2, 0)], GOOD[2]),
    "read-position-negative": (GOOD[0], [(0, 0, 0, -1, 4, 2, 0)], GOOD[2]),
    "read-position-too-large": (GOOD[0], [(0, 0, 0, 1, 2 ** 31 - 1, 2, 0)], GOOD[2]),
    "read-off-negative": (GOOD[0], [(0, 0, -1, 3, 4, 2, 0)], GOOD[2]),
    "read-len-negative": (GOOD[0], [(0, 0, 0, 3, 4, -1, 0)], GOOD[2]),
    "read-range-past-the-end": (GOOD[0], [(0, 0, 1, 3, 4, 2, 0)], GOOD[2]),
    "read-off-past-the-end": (GOOD[0], [(0, 0, 3, 3, 4, 0, 0)], GOOD[2]),
}


@pytest.mark.parametrize("name", sorted(EINVAL_CASES))
def test_host_einval(name):
    with pytest.raises(abi.LcError) as e:
        abi.set_full_host(*_arrays(*EINVAL_CASES[name]))
    assert e.value.code == -errno.EINVAL


def test_host_good_and_empty():
    out, s = abi.set_full_host(*_arrays(*GOOD))
    # element 1 is seen by the first read and missed by the second; element 2
    # has no completion and is seen by both: known = the first read's ok
    assert out["outcome"].tolist() == [abi.LC_SF_LOST, abi.LC_SF_STABLE] and s["valid"] == 0
    assert out["known_pos"].tolist() == [1, 4] and out["last_absent"].tolist() == [5, -1]
    assert out["last_present"].tolist() == [3, 5]
    for adds, reads, values in (([], GOOD[1], GOOD[2]), (GOOD[0], [], []), ([], [], [])):
        out, s = abi.set_full_host(*_arrays(adds, reads, values))
        assert (out["outcome"] == abi.LC_SF_NEVER_READ).all() and s["valid"] == -1
        assert s["n_phantom"] == (3 if reads else 0) and s["n_never_read"] == len(adds)
    lim = abi.set_full_limits()
    assert lim["tile_bytes"] == lim["default_tile_bytes"] == 1 << 30
    assert lim["max_position"] == 2 ** 31 - 1 and lim["value_bytes"] == 8
