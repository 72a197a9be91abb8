"""lc_append_check_host and AppendChecker(device=False) against the
independent restatement (append_ref.py), on hand-derived histories
(golden/append_kat.json) and 2,000 random tiny ones; the witness cycles
certified; the encoder's rules; every -EINVAL with nothing written."""
import errno
import json
import os

import numpy as np
import pytest

import append_cases as C
import append_ref as REF
from jepsen.etcd_amd import abi, append as AP

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "append_kat.json")))["cases"]
EDGE = {abi.LC_AP_WW: "ww", abi.LC_AP_WR: "wr", abi.LC_AP_RW: "rw"}
BITS = ((abi.LC_AP_R_NONPREFIX, "incompatible-order"), (abi.LC_AP_R_DUPLICATE, "duplicate-elements"),
        (abi.LC_AP_R_G1A, "G1a"), (abi.LC_AP_R_PHANTOM, "phantom"), (abi.LC_AP_R_G1B, "G1b"),
        (abi.LC_AP_R_INTERNAL, "internal"), (abi.LC_AP_R_EXTERNAL, "external"))
COUNT_OF = {"incompatible-order": "n_nonprefix", "duplicate-elements": "n_duplicate", "G1a": "n_g1a",
            "phantom": "n_phantom", "G1b": "n_g1b", "internal": "n_internal",
            "incompatible-keys": "n_incompatible_order"}
# the edge types a class's witness may use, and (type, at least) it must hold
ALLOWED = {"G0": {0}, "G1c": {0, 1}, "G-single": {0, 1, 2}, "G2-item": {0, 1, 2}}
NEEDS = {"G0": [(0, 1)], "G1c": [(1, 1)], "G-single": [(2, 1)], "G2-item": [(2, 2)]}


def names_of(flags):
    return {name for bit, name in BITS if flags & bit}


def lib_view(enc, out, s):
    """The library's arrays in append_ref.check's shapes (integer keys and elements)."""
    txns, mops = enc.txns, enc.mops
    mop_txn = np.repeat(np.arange(len(txns)), txns["mop_len"])
    read_flags, keys = {}, {}
    for m in np.nonzero((mops["f"] == abi.LC_AP_READ) & (mops["len"] >= 0))[0]:
        t = int(mop_txn[m])
        read_flags[(t, int(m - txns["mop_off"][t]))] = names_of(int(out["mop_flags"][m]))
    assert not out["mop_flags"][(mops["f"] != abi.LC_AP_READ) | (mops["len"] < 0)].any()
    for k in out["keys"]:
        lg = int(k["longest"])
        keys[int(k["key"])] = {
            "longest": None if lg < 0 else (int(mop_txn[lg]), int(lg - txns["mop_off"][mop_txn[lg]])),
            "order": [] if lg < 0 else enc.values[mops["value"][lg]:mops["value"][lg] + mops["len"][lg]].tolist(),
            "incompatible": bool(k["flags"] & abi.LC_AP_K_INCOMPATIBLE),
            "first_dup": int(k["first_dup"]), "first_failed": int(k["first_failed"]),
            "first_phantom": int(k["first_phantom"]), "no_order": bool(k["flags"] & abi.LC_AP_K_NO_ORDER)}
        assert lg < 0 or k["len"] == mops["len"][lg]
    assert (np.diff(out["keys"]["key"]) > 0).all()
    e = out["edges"]
    edges = {(int(x["from"]), int(x["to"]), EDGE[int(x["type"])], int(x["key"])) for x in e}
    as_rows = [(int(x["from"]), int(x["to"]), int(x["type"]), int(x["key"])) for x in e]
    assert as_rows == sorted(set(as_rows)), "edges not sorted and unique"
    rt_pred = {t: set(out["byc"][out["rt_lo"][t]:out["rt_hi"][t]].tolist()) for t in range(len(txns))}
    n_scc = int(s["n_scc"])
    sccs = [frozenset(np.nonzero(out["scc"] == c)[0].tolist()) for c in range(n_scc)]
    classes = [abi.LC_AP_CLASSES[int(out["scc_class"][min(m)])] for m in sccs]
    for c, m in enumerate(sccs):
        assert len(m) >= 2 and len({int(out["scc_class"][t]) for t in m}) == 1
        assert c == 0 or min(sccs[c - 1]) < min(m)
    counts = {name: int(s[f]) for name, f in COUNT_OF.items()}
    for i, c in enumerate(abi.LC_AP_CLASSES):
        counts[c] = int(s["n_class"][i])
    txn_flags = {t: names_of(int(f)) for t, f in enumerate(out["txn_flags"])}
    return {"read_flags": read_flags, "txn_flags": txn_flags, "keys": keys, "edges": edges, "rt_pred": rt_pred,
            "sccs": sccs, "classes": classes, "counts": counts,
            "valid": {1: True, 0: False, -1: "unknown"}[int(s["valid"])]}


def certify_cycles(enc, out, s):
    """Every returned cycle: each step an edge of the stated type and key in
    the returned edges or real-time ranges, closed, inside its SCC, its edge
    types fitting the SCC's class."""
    edges = {(int(x["from"]), int(x["to"]), int(x["type"]), int(x["key"])) for x in out["edges"]}
    n = int(s["n_cycles_returned"])
    assert n == min(int(s["n_scc"]), abi.LC_AP_MAX_CYCLES) and out["cycle_off"][0] == 0
    for c in range(n):
        cyc = out["steps"][out["cycle_off"][c]:out["cycle_off"][c + 1]]
        assert len(cyc) >= 2 and int(out["cycle_scc"][c]) == c
        txs = [int(x["txn"]) for x in cyc]
        assert len(set(txs)) == len(txs) and all(out["scc"][t] == c for t in txs)
        for i, x in enumerate(cyc):
            a, b, typ = txs[i], txs[(i + 1) % len(txs)], int(x["type"])
            if typ == abi.LC_AP_RT:
                assert a in out["byc"][out["rt_lo"][b]:out["rt_hi"][b]].tolist(), (c, i)
            else:
                assert (a, b, typ, int(x["key"])) in edges, (c, i)
        cls = abi.LC_AP_CLASSES[int(out["scc_class"][txs[0]])]
        types = [int(x["type"]) for x in cyc]
        base = cls.replace("-realtime", "")
        allowed = ALLOWED[base] | ({abi.LC_AP_RT} if cls.endswith("-realtime") else set())
        assert set(types) <= allowed, (cls, types)
        for typ, least in NEEDS[base]:
            assert types.count(typ) >= least, (cls, types)
        if base == "G-single":
            assert types.count(abi.LC_AP_RW) == 1, (cls, types)
        if cls.endswith("-realtime"):
            assert abi.LC_AP_RT in types, (cls, types)


def strip_cycles(result):
    """A result map with the cycle records taken out (they are certified, not compared)."""
    if not isinstance(result["anomalies"], dict):
        return result
    r = dict(result)
    r["anomalies"] = {k: (None if k in abi.LC_AP_CLASSES else v) for k, v in result["anomalies"].items()}
    return r


def agree_with_ref(history, ref=None, checker=None):
    ref = ref or REF.check(history)
    enc = AP.encode(history)
    out, s = abi.append_check_host(enc.txns, enc.mops, enc.values)
    got = lib_view(enc, out, s)
    for field in ("valid", "counts", "read_flags", "txn_flags", "keys", "edges", "rt_pred", "sccs", "classes"):
        assert got[field] == ref[field], (field, got[field], ref[field])
    assert (s["n_ok"], s["n_nodes"]) == (sum(x["type"] == "ok" for x in ref["txns"]),
                                         sum(x["type"] != "fail" for x in ref["txns"]))
    certify_cycles(enc, out, s)
    checker = checker or AP.AppendChecker(device=False)
    result = checker.check({}, history, {})
    assert strip_cycles(result) == ref["result"], (strip_cycles(result), ref["result"])
    for name, recs in result["anomalies"].items() if isinstance(result["anomalies"], dict) else ():
        if name in abi.LC_AP_CLASSES:
            for rec in recs:
                assert rec["cycle"][0] is rec["cycle"][-1] and len(rec["steps"]) == len(rec["cycle"]) - 1
    return ref, s


# ---------------------------------------------------------------- KATs

@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(kat):
    ref, s = agree_with_ref(kat["history"])
    assert ref["valid"] == kat["valid"], kat["why"]
    assert ref["result"]["anomaly-types"] == sorted(kat["anomaly-types"]), kat["why"]
    if "edges" in kat:
        assert sorted(ref["edges"]) == sorted(tuple(e) for e in kat["edges"]), kat["why"]


def test_kats_cover_what_they_should():
    seen = {a for k in KATS for a in k["anomaly-types"]}
    assert set(REF.READ_NAMES) | set(REF.CLASSES) | {"empty-transaction-graph"} <= seen
    assert any(k["valid"] is True for k in KATS)


# ---------------------------------------------------------------- random tiny histories

N_RANDOM, AT_LEAST = 2000, 20
_refs = {}


def random_refs():
    if not _refs:
        for seed in range(N_RANDOM):
            h = C.random_history(seed)
            _refs[seed] = (h, REF.check(h))
    return _refs


def test_random_histories_reach_every_anomaly():
    """From the reference alone: each anomaly of rules 2-4 and each class of
    rule 7 occurs in at least 20 of the 2,000 histories."""
    seen = {}
    for h, ref in random_refs().values():
        for name in ref["result"]["anomaly-types"]:
            seen[name] = seen.get(name, 0) + 1
    short = {n: seen.get(n, 0) for n in REF.READ_NAMES + REF.CLASSES if seen.get(n, 0) < AT_LEAST}
    assert not short, (short, seen)
    assert sum(ref["valid"] is True for _, ref in random_refs().values()) >= AT_LEAST


def test_random_histories_agree():
    checker = AP.AppendChecker(device=False)
    for seed, (h, ref) in random_refs().items():
        try:
            agree_with_ref(h, ref, checker)
        except AssertionError as e:
            raise AssertionError("seed %d: %s" % (seed, e)) from e


# ---------------------------------------------------------------- the encoder

def test_encode_pairs_by_process_and_takes_ok_mops_from_the_completion():
    h = [C.op("invoke", 0, [["append", 5, 1], ["r", 5, None]], 0),
         C.op("invoke", 1, [["r", 5, None]], 1),
         {"type": "info", "f": "start", "process": "nemesis", "value": None},
         C.op("ok", 1, [["r", 5, [1]]], 3),
         C.op("ok", 0, [["append", 5, 1], ["r", 5, [1]]], 4),
         C.op("invoke", 2, [["append", 5, 2], ["r", 5, None]], 5),
         C.op("fail", 2, [["append", 5, 2], ["r", 5, None]], 6),
         C.op("invoke", 3, [[":append", 5, 3], [":r", 5, None]], 7),
         C.op("info", 3, [[":append", 5, 3], [":r", 5, None]], 8),
         C.op("invoke", 4, [["r", 5, None]], 9),
         C.op("ok", 9, [["r", 5, []]], 10)]
    enc = AP.encode(h)
    assert enc.txns["inv_pos"].tolist() == [0, 1, 5, 7, 9] and enc.txns["comp_pos"].tolist() == [4, 3, 6, -1, -1]
    assert enc.txns["type"].tolist() == [abi.LC_AP_OK, abi.LC_AP_OK, abi.LC_AP_FAIL, abi.LC_AP_INFO, abi.LC_AP_INFO]
    assert enc.txns["mop_off"].tolist() == [0, 2, 3, 5, 7] and enc.n_orphans == 1
    assert enc.mops["len"].tolist() == [0, 1, 1, 0, -1, 0, -1, -1]
    assert enc.mops["f"].tolist() == [0, 1, 1, 0, 1, 0, 1, 1] and enc.values.tolist() == [1, 1]
    assert enc.comp == [4, 3, 6, 8, -1] and enc.keys is None and enc.elements is None


def test_encode_interns_what_is_no_int64():
    h = [C.op("invoke", 0, [["append", "x", "a"], ["append", "y", 2 ** 63]], 0),
         C.op("ok", 0, [["append", "x", "a"], ["append", "y", 2 ** 63]], 1),
         C.op("invoke", 0, [["r", "x", None], ["r", "y", None]], 2),
         C.op("ok", 0, [["r", "x", ["a"]], ["r", "y", [2 ** 63]]], 3)]
    enc = AP.encode(h)
    assert enc.keys == ["x", "y"] and enc.elements == ["a", 2 ** 63]
    assert enc.mops["key"].tolist() == [0, 1, 0, 1] and enc.values.tolist() == [0, 1]
    r = AP.AppendChecker(device=False).check({}, h, {})
    assert r == {"valid?": True, "anomaly-types": [], "anomalies": {}, "not": set()}


@pytest.mark.parametrize("bad", [
    [C.op("invoke", 0, [["append", 1, 1]], 0), C.op("invoke", 0, [["append", 1, 2]], 1)],
    [C.op("invoke", 0, [["write", 1, 1]], 0)],
    [C.op("invoke", 0, "nope", 0)],
    [C.op("invoke", 0, [["append", 1, 1]], 0), C.op("ok", 0, [["append", 1, 2]], 1)],
    [C.op("invoke", 0, [["append", 1, 1]], 0), C.op("ok", 0, [["append", 1, 1], ["r", 1, [1]]], 1)],
    [C.op("invoke", 0, [["r", 1, None]], 0), C.op("ok", 0, [["r", 1, 7]], 1)],
    [C.op("invoke", 0, [["append", 1, 1], ["append", 1, 1]], 0)],
], ids=["pending-invoke", "unknown-f", "no-mop-list", "other-element", "other-mops", "read-no-list",
        "element-twice"])
def test_encode_refuses(bad):
    with pytest.raises(AP.Unsupported):
        AP.encode(bad)


# ---------------------------------------------------------------- -EINVAL

def _good():
    enc = AP.encode(C.sequential(3) + [C.op("invoke", 1, [["append", 0, 9]], 6)])
    return enc.txns.copy(), enc.mops.copy(), enc.values.copy()


def _break(what):
    t, m, v = _good()
    if what == "inv-order":
        t["inv_pos"][1] = t["inv_pos"][0]
    elif what == "comp-below-inv":
        t["comp_pos"][0] = t["inv_pos"][0]
    elif what == "info-with-comp":
        t["comp_pos"][3] = 99
    elif what == "type":
        t["type"][0] = 3
    elif what == "position":
        t["inv_pos"][3] = 2 ** 31 - 1
    elif what == "mop-gap":
        t["mop_off"][1] += 1
    elif what == "mop-short":
        t["mop_len"][3] = 0
    elif what == "mop-f":
        m["f"][0] = 2
    elif what == "key-reserved":
        m["key"][0] = -2 ** 63
    elif what == "element-reserved":
        m["value"][0] = -2 ** 63
    elif what == "read-leaves-values":
        m["len"][5] = 4
    elif what == "read-negative":
        m["value"][1] = -1
    elif what == "ok-read-ignored":
        m["len"][1] = -1
    elif what == "info-read-with-len":
        t["type"][2], t["comp_pos"][2] = abi.LC_AP_INFO, -1
    elif what == "pair-twice":
        m["value"][6] = m["value"][0]
    return t, m, v


EINVAL_CASES = ("inv-order", "comp-below-inv", "info-with-comp", "type", "position", "mop-gap", "mop-short",
                "mop-f", "key-reserved", "element-reserved", "read-leaves-values", "read-negative",
                "ok-read-ignored", "info-read-with-len", "pair-twice")


@pytest.mark.parametrize("what", EINVAL_CASES)
def test_einval_writes_nothing(what):
    abi.append_check_host(*_good())
    call = C.MarkedCall(*_break(what))
    assert call.run() == -errno.EINVAL and call.untouched()
    with pytest.raises(abi.LcError) as e:
        abi.append_check_host(*_break(what))
    assert e.value.code == -errno.EINVAL


def test_null_out_is_einval():
    call = C.MarkedCall(*_good())
    call.out.edges = None
    assert call.run() == -errno.EINVAL and call.untouched()


def test_no_txns_is_unknown():
    out, s = abi.append_check_host(np.zeros(0, abi.AP_TXN_DTYPE), np.zeros(0, abi.AP_MOP_DTYPE), [])
    assert s["valid"] == -1 and s["n_keys"] == s["n_edges"] == s["n_scc"] == 0
    assert AP.AppendChecker(device=False).check({}, [], {})["valid?"] == "unknown"


def test_limits():
    lim = abi.append_limits()
    assert lim["max_payload"] == lim["default_max_payload"] == 1 << 30 and lim["max_position"] == 2 ** 31 - 1
    assert lim["max_mops"] == 1 << 29  # twice that many key-table slots still have int32 indices
