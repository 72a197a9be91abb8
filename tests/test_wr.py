"""lc_wr_check_host and WrChecker(device=False) against the independent
restatement (wr_ref.py), with the wfr inference on and off, on hand-derived
histories (golden/wr_kat.json) and 2,000 random tiny ones; the witness cycles
certified; the encoder's rules; every -EINVAL with nothing written; -ENOSPC
with n_edges set."""
import errno
import json
import os

import numpy as np
import pytest

import wr_cases as C
import wr_ref as REF
from jepsen.etcd_amd import abi, wr as WR

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "wr_kat.json")))["cases"]
EDGE = {abi.LC_AP_WW: "ww", abi.LC_AP_WR: "wr", abi.LC_AP_RW: "rw"}
BITS = ((abi.LC_WR_R_INTERNAL, "internal"), (abi.LC_WR_R_PHANTOM, "phantom"), (abi.LC_WR_R_G1A, "G1a"),
        (abi.LC_WR_R_G1B, "G1b"), (abi.LC_WR_R_EXTERNAL, "external"))
COUNT_OF = {"internal": "n_internal", "phantom": "n_phantom", "G1a": "n_g1a", "G1b": "n_g1b",
            "cyclic-versions": "n_cyclic_keys", "lost-update": "n_lost_update"}
# the edge types a class's witness may use, and (type, at least) it must hold
ALLOWED = {"G0": {0}, "G1c": {0, 1}, "G-single": {0, 1, 2}, "G2-item": {0, 1, 2}}
NEEDS = {"G0": [(0, 1)], "G1c": [(1, 1)], "G-single": [(2, 1)], "G2-item": [(2, 2)]}
# what cannot occur without the wfr inference: it alone makes version cycles and ww edges
WFR_ONLY = {"cyclic-versions", "G0", "G0-realtime"}


def names_of(flags):
    return {name for bit, name in BITS if flags & bit}


def lib_view(enc, out, s):
    """The library's arrays in wr_ref.check's shapes (integer keys and values)."""
    txns, mops = enc.txns, enc.mops
    mop_txn = np.repeat(np.arange(len(txns)), txns["mop_len"])
    read_flags, keys = {}, {}
    known = (mops["f"] == abi.LC_WR_READ) & (mops["known"] == 1)
    for m in np.nonzero(known)[0]:
        t = int(mop_txn[m])
        read_flags[(t, int(m - txns["mop_off"][t]))] = names_of(int(out["mop_flags"][m]))
    assert not out["mop_flags"][~known].any()
    for k in out["keys"]:
        cyclic = bool(k["flags"] & abi.LC_WR_K_CYCLIC)
        assert cyclic or k["cyc_value"] == abi.LC_WR_NIL
        keys[int(k["key"])] = {"cyclic": cyclic, "cyc_value": int(k["cyc_value"]) if cyclic else None,
                               "lost": bool(k["flags"] & abi.LC_WR_K_LOST_UPDATE), "n_writes": int(k["n_writes"]),
                               "n_versions": int(k["n_versions"]), "n_ext_reads": int(k["n_ext_reads"])}
    assert (np.diff(out["keys"]["key"]) > 0).all()
    assert s["n_versions"] == int(out["keys"]["n_versions"].sum()) and s["n_edges_raw"] >= s["n_edges"]
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


def certify_cycles(out, s):
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


def agree_with_ref(history, wfr, ref=None, checker=None):
    ref = ref or REF.check(history, wfr)
    enc = WR.encode(history)
    out, s = abi.wr_check_host(enc.txns, enc.mops, wfr)
    got = lib_view(enc, out, s)
    for field in ("valid", "counts", "read_flags", "txn_flags", "keys", "edges", "rt_pred", "sccs", "classes"):
        assert got[field] == ref[field], (field, got[field], ref[field])
    assert (s["n_ok"], s["n_nodes"]) == (sum(x["type"] == "ok" for x in ref["txns"]),
                                         sum(x["type"] != "fail" for x in ref["txns"]))
    certify_cycles(out, s)
    checker = checker or WR.WrChecker(device=False, wfr_keys=wfr)
    result = checker.check({}, history, {})
    assert strip_cycles(result) == ref["result"], (strip_cycles(result), ref["result"])
    for name, recs in result["anomalies"].items() if isinstance(result["anomalies"], dict) else ():
        if name in abi.LC_AP_CLASSES:
            for rec in recs:
                assert rec["cycle"][0] is rec["cycle"][-1] and len(rec["steps"]) == len(rec["cycle"]) - 1
    return ref, s


# ---------------------------------------------------------------- KATs

@pytest.mark.parametrize("wfr", (True, False), ids=("wfr", "no-wfr"))
@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(kat, wfr):
    ref, s = agree_with_ref(kat["history"], wfr)
    off = "" if wfr else "-off"
    assert ref["valid"] == kat["valid" + off], kat["why"]
    assert ref["result"]["anomaly-types"] == sorted(kat["anomaly-types" + off]), kat["why"]
    want = kat.get("edges")
    if not wfr and "edges-off" in kat:
        want = kat["edges-off"]
    elif not wfr and want is not None and any(e[2] == "ww" for e in want):
        want = None  # (ww edges come from the wfr inference alone)
    if want is not None:
        assert sorted(ref["edges"]) == sorted(tuple(e) for e in want), kat["why"]
    cyc = {int(k): v for k, v in kat.get("cyc", {}).items()} if wfr else {}
    assert {k: r["cyc_value"] for k, r in ref["keys"].items() if r["cyclic"]} == cyc, kat["why"]


def test_kats_cover_what_they_should():
    seen = {a for k in KATS for a in k["anomaly-types"]}
    assert set(REF.READ_NAMES) | set(REF.KEY_NAMES) | set(REF.CLASSES) | {"empty-transaction-graph"} <= seen
    assert any(k["valid"] is True for k in KATS)
    lost = next(k for k in KATS if k["name"] == "lost-update")
    assert lost["anomaly-types-off"] == ["lost-update"]  # invalid by rule 5 alone, with no SCC


def test_lost_update_without_wfr_has_no_scc():
    lost = next(k for k in KATS if k["name"] == "lost-update")
    enc = WR.encode(lost["history"])
    out, s = abi.wr_check_host(enc.txns, enc.mops, False)
    assert s["valid"] == 0 and s["n_scc"] == 0 and s["n_lost_update"] == 1
    out, s = abi.wr_check_host(enc.txns, enc.mops, True)
    assert s["valid"] == 0 and s["n_scc"] == 1 and s["n_lost_update"] == 1


# ---------------------------------------------------------------- random tiny histories

N_RANDOM, AT_LEAST = 2000, 20
_refs = {}


def random_refs():
    if not _refs:
        for seed in range(N_RANDOM):
            h = C.random_history(seed)
            _refs[seed] = (h, REF.check(h, True), REF.check(h, False))
    return _refs


@pytest.mark.parametrize("wfr", (True, False), ids=("wfr", "no-wfr"))
def test_random_histories_reach_every_anomaly(wfr):
    """From the reference alone: each anomaly of rules 2-6 and each class of
    rule 9 occurs in at least 20 of the 2,000 histories — without the wfr
    inference, each of those that can occur at all."""
    seen = {}
    for refs in random_refs().values():
        for name in refs[1 if wfr else 2]["result"]["anomaly-types"]:
            seen[name] = seen.get(name, 0) + 1
    names = set(REF.READ_NAMES + REF.KEY_NAMES + REF.CLASSES) - (set() if wfr else WFR_ONLY)
    short = {n: seen.get(n, 0) for n in names if seen.get(n, 0) < AT_LEAST}
    assert not short, (short, seen)
    assert wfr or not WFR_ONLY & set(seen)
    assert sum(refs[1 if wfr else 2]["valid"] is True for refs in random_refs().values()) >= AT_LEAST


@pytest.mark.parametrize("wfr", (True, False), ids=("wfr", "no-wfr"))
def test_random_histories_agree(wfr):
    checker = WR.WrChecker(device=False, wfr_keys=wfr)
    for seed, refs in random_refs().items():
        try:
            agree_with_ref(refs[0], wfr, refs[1 if wfr else 2], checker)
        except AssertionError as e:
            raise AssertionError("seed %d: %s" % (seed, e)) from e


# ---------------------------------------------------------------- the encoder

def test_encode_pairs_by_process_and_takes_ok_mops_from_the_completion():
    h = [C.op("invoke", 0, [["w", 5, 1], ["r", 5, None]], 0),
         C.op("invoke", 1, [["r", 5, None]], 1),
         {"type": "info", "f": "start", "process": "nemesis", "value": None},
         C.op("ok", 1, [["r", 5, None]], 3),
         C.op("ok", 0, [["w", 5, 1], ["r", 5, 1]], 4),
         C.op("invoke", 2, [["w", 5, 2], ["r", 5, None]], 5),
         C.op("fail", 2, [["w", 5, 2], ["r", 5, None]], 6),
         C.op("invoke", 3, [[":w", 5, 3], [":r", 5, None]], 7),
         C.op("info", 3, [[":w", 5, 3], [":r", 5, None]], 8),
         C.op("invoke", 4, [["r", 5, None]], 9),
         C.op("ok", 9, [["r", 5, 1]], 10)]
    enc = WR.encode(h)
    assert enc.txns["inv_pos"].tolist() == [0, 1, 5, 7, 9] and enc.txns["comp_pos"].tolist() == [4, 3, 6, -1, -1]
    assert enc.txns["type"].tolist() == [abi.LC_WR_OK, abi.LC_WR_OK, abi.LC_WR_FAIL, abi.LC_WR_INFO, abi.LC_WR_INFO]
    assert enc.txns["mop_off"].tolist() == [0, 2, 3, 5, 7] and enc.n_orphans == 1
    assert enc.mops["known"].tolist() == [0, 1, 1, 0, 0, 0, 0, 0]
    assert enc.mops["f"].tolist() == [0, 1, 1, 0, 1, 0, 1, 1]
    assert enc.mops["value"].tolist() == [1, 1, abi.LC_WR_NIL, 2, 0, 3, 0, 0]  # an :ok [:r k nil] is a nil read
    assert enc.comp == [4, 3, 6, 8, -1] and enc.keys is None and enc.values is None


def test_encode_interns_what_is_no_int64():
    h = [C.op("invoke", 0, [["w", "x", "a"], ["w", "y", 2 ** 63]], 0),
         C.op("ok", 0, [["w", "x", "a"], ["w", "y", 2 ** 63]], 1),
         C.op("invoke", 0, [["r", "x", None], ["r", "y", None], ["r", "z", None]], 2),
         C.op("ok", 0, [["r", "x", "a"], ["r", "y", 2 ** 63], ["r", "z", None]], 3)]
    enc = WR.encode(h)
    assert enc.keys == ["x", "y", "z"] and enc.values == ["a", 2 ** 63]
    assert enc.mops["key"].tolist() == [0, 1, 0, 1, 2] and enc.mops["value"].tolist() == [0, 1, 0, 1, abi.LC_WR_NIL]
    r = WR.WrChecker(device=False).check({}, h, {})
    assert r == {"valid?": True, "anomaly-types": [], "anomalies": {}, "not": set()}


def test_result_map_names_interned_values():
    h = [C.op("invoke", 0, [["r", "x", None], ["w", "x", "b"]], 0), C.op("invoke", 1, [["r", "x", None], ["w", "x", "a"]], 1),
         C.op("ok", 0, [["r", "x", "a"], ["w", "x", "b"]], 2), C.op("ok", 1, [["r", "x", "b"], ["w", "x", "a"]], 3)]
    r = WR.WrChecker(device=False).check({}, h, {})
    assert r["anomalies"]["cyclic-versions"] == [{"key": "x", "cycle": ["a", "b", "a"]}]  # "a" was interned first, so it is the least
    assert r["valid?"] is False and "G1c" in r["anomaly-types"]
    assert WR.WrChecker(device=False, wfr_keys=False).check({}, h, {})["anomaly-types"] == ["G1c"]


@pytest.mark.parametrize("bad", [
    [C.op("invoke", 0, [["w", 1, 1]], 0), C.op("invoke", 0, [["w", 1, 2]], 1)],
    [C.op("invoke", 0, [["append", 1, 1]], 0)],
    [C.op("invoke", 0, "nope", 0)],
    [C.op("invoke", 0, [["w", 1, 1]], 0), C.op("ok", 0, [["w", 1, 2]], 1)],
    [C.op("invoke", 0, [["w", 1, 1]], 0), C.op("ok", 0, [["w", 1, 1], ["r", 1, 1]], 1)],
    [C.op("invoke", 0, [["w", 1, None]], 0)],
    [C.op("invoke", 0, [["w", 1, 1], ["w", 1, 1]], 0)],
], ids=["pending-invoke", "unknown-f", "no-mop-list", "other-value", "other-mops", "write-of-nil", "value-twice"])
def test_encode_refuses(bad):
    with pytest.raises(WR.Unsupported):
        WR.encode(bad)


# ---------------------------------------------------------------- -EINVAL, -ENOSPC

def _good():
    enc = WR.encode(C.sequential(3) + [C.op("invoke", 1, [["w", 0, 9]], 6)])
    return enc.txns.copy(), enc.mops.copy()


def _break(what):
    t, m = _good()
    kw = {}
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
    elif what == "write-of-nil":
        m["value"][1] = -2 ** 63
    elif what == "ok-read-unknown":
        m["known"][0] = 0
    elif what == "known-not-0-or-1":
        m["known"][0] = 2
    elif what == "write-known":
        m["known"][1] = 1
    elif what == "info-read-known":
        t["type"][2], t["comp_pos"][2] = abi.LC_WR_INFO, -1
    elif what == "pair-twice":
        m["value"][6] = m["value"][1]
    elif what == "negative-edge-cap":
        kw["edge_cap"] = -1
    return t, m, kw


EINVAL_CASES = ("inv-order", "comp-below-inv", "info-with-comp", "type", "position", "mop-gap", "mop-short",
                "mop-f", "key-reserved", "write-of-nil", "ok-read-unknown", "known-not-0-or-1", "write-known",
                "info-read-known", "pair-twice", "negative-edge-cap")


def marked(what, wfr=True):
    t, m, kw = _break(what)
    call = C.MarkedCall(t, m, wfr, **kw)
    if "edge_cap" in kw:
        call.out.edge_cap = kw["edge_cap"]
    return call


@pytest.mark.parametrize("what", EINVAL_CASES)
def test_einval_writes_nothing(what):
    abi.wr_check_host(*_good())
    call = marked(what)
    assert call.run() == -errno.EINVAL and call.untouched()
    if what != "negative-edge-cap":
        with pytest.raises(abi.LcError) as e:
            abi.wr_check_host(*_break(what)[:2])
        assert e.value.code == -errno.EINVAL


def test_unknown_flag_is_einval():
    call = C.MarkedCall(*_good())
    call.flags = 2
    assert call.run() == -errno.EINVAL and call.untouched()
    call.flags = abi.LC_WR_WFR_KEYS | 4
    assert call.run() == -errno.EINVAL and call.untouched()


def test_null_out_is_einval():
    call = C.MarkedCall(*_good())
    call.out.edges = None
    assert call.run() == -errno.EINVAL and call.untouched()


def test_enospc_sets_n_edges_and_writes_no_array():
    lost = next(k for k in KATS if k["name"] == "lost-update")
    enc = WR.encode(lost["history"])
    want, ws = abi.wr_check_host(enc.txns, enc.mops)
    assert ws["n_edges"] == 6
    call = C.MarkedCall(enc.txns, enc.mops, True, edge_cap=5)
    assert call.run() == -errno.ENOSPC and call.arrays_untouched()
    assert call.summary.n_edges == 6 and call.summary.n_edges_raw == ws["n_edges_raw"] and call.summary.valid == 0
    with pytest.raises(abi.LcError) as e:
        abi.wr_check_host(enc.txns, enc.mops, edge_cap=5)
    assert e.value.code == -errno.ENOSPC
    call = C.MarkedCall(enc.txns, enc.mops, True, edge_cap=6)
    assert call.run() == 0 and call.summary.n_edges == 6
    # the binding comes again with room when the default does not hold the edges: 20 nil readers x 20 writers
    txs = [[["r", 1, None]] for _ in range(20)] + [[["w", 1, v + 1]] for v in range(20)]
    h = [C.op(typ, i, [list(m) for m in t], 0) for typ in ("invoke", "ok") for i, t in enumerate(txs)]
    enc = WR.encode(h)
    out, s = abi.wr_check_host(enc.txns, enc.mops)
    assert s["n_edges"] == s["n_edges_raw"] == 400 > 2 * len(enc.mops) + 16 and s["valid"] == 1


def test_no_txns_is_unknown():
    out, s = abi.wr_check_host(np.zeros(0, abi.WR_TXN_DTYPE), np.zeros(0, abi.WR_MOP_DTYPE))
    assert s["valid"] == -1 and s["n_keys"] == s["n_edges"] == s["n_scc"] == 0
    assert WR.WrChecker(device=False).check({}, [], {})["valid?"] == "unknown"


def test_limits(monkeypatch):
    lim = abi.wr_limits()
    assert lim["max_edges"] == lim["default_max_edges"] == 1 << 27 and lim["max_position"] == 2 ** 31 - 1
    assert lim["max_mops"] == 1 << 29
    monkeypatch.setenv("LC_WR_MAX_EDGES", "1000")
    assert abi.wr_limits()["max_edges"] == 1000 and abi.wr_limits()["default_max_edges"] == 1 << 27


def test_synth_arrays_is_valid_and_shaped_like_the_workload():
    txns, mops = WR.synth_arrays(3000, seed=5)
    out, s = abi.wr_check_host(txns, mops)
    assert s["valid"] == 1 and s["n_nodes"] == 3000 and 0.01 < 1 - s["n_ok"] / 3000 < 0.06
    assert txns["mop_len"].max() == 4 and out["keys"]["n_writes"].max() == 32
    out, s = abi.wr_check_host(txns, mops, wfr_keys=False)
    assert s["valid"] == 1
