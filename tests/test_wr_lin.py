"""lc_wr_check_lin_host and WrChecker(device=False, linearizable_keys=True)
against the independent restatement (wr_lin_ref.py) under all four flag
combinations, on hand-derived histories (golden/wr_lin_kat.json) and 2,000
random tiny ones; witness and version cycles certified; flag-off equality
with lc_wr_check_host; every -EINVAL with nothing written; -ENOSPC; the
limits; a synthetic valid history."""
import ctypes
import errno
import json
import os

import numpy as np
import pytest

import test_wr as TW
import wr_cases as C
import wr_lin_ref as REF
from jepsen.etcd_amd import abi, wr as WR

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "wr_lin_kat.json")))["cases"]
COMBOS = ((False, False), (True, False), (False, True), (True, True))  # (wfr, lin)
COMBO_IDS = ("", "wfr", "lin", "wfr+lin")
LIN_FIELDS = ("n_pairs", "n_touches", "n_vedges")


def lin_view(out):
    return {int(k["key"]): {f: int(r[f]) for f in LIN_FIELDS} for k, r in zip(out["keys"], out["lin_keys"])}


def certify_version_cycles(result, ref):
    """Each cyclic key's cycle: closed, through cyc_value first, every step a
    version edge of the reference's graph."""
    recs = result["anomalies"].get("cyclic-versions", []) if isinstance(result["anomalies"], dict) else []
    assert sorted(r["key"] for r in recs) == sorted(k for k, rec in ref["keys"].items() if rec["cyclic"])
    for r in recs:
        cyc = r["cycle"]
        assert len(cyc) >= 2 and cyc[0] == cyc[-1] == ref["keys"][r["key"]]["cyc_value"], r
        assert all((a, b) in ref["vedges"][r["key"]] for a, b in zip(cyc, cyc[1:])), r


def strip(result):
    """A result map without the witness cycles and the version cycles (certified, not compared)."""
    r = TW.strip_cycles(result)
    if isinstance(r["anomalies"], dict) and "cyclic-versions" in r["anomalies"]:
        r["anomalies"]["cyclic-versions"] = [dict(rec, cycle=None) for rec in r["anomalies"]["cyclic-versions"]]
    return r


def agree_with_ref(history, wfr, lin, ref=None, checker=None):
    ref = ref or REF.check(history, wfr, lin)
    enc = WR.encode(history)
    out, s, ls = abi.wr_check_lin_host(enc.txns, enc.mops, wfr, lin)
    got = TW.lib_view(enc, out, s)
    for field in ("valid", "counts", "read_flags", "txn_flags", "keys", "edges", "rt_pred", "sccs", "classes"):
        assert got[field] == ref[field], (field, got[field], ref[field])
    assert lin_view(out) == ref["lin"], (lin_view(out), ref["lin"])
    assert {"touches": ls["n_touches"], "pairs": ls["n_pairs"], "version-edges": ls["n_vedges"]} == ref["lin_totals"]
    TW.certify_cycles(out, s)
    if not lin:  # lc_wr_check_host itself
        out0, s0 = abi.wr_check_host(enc.txns, enc.mops, wfr)
        same_outputs(out, s, out0, s0)
        assert ls["max_key_versions"] == 0
        return ref, s
    checker = checker or WR.WrChecker(device=False, wfr_keys=wfr, linearizable_keys=True)
    result = checker.check({}, history, {})
    assert strip(result) == ref["result"], (strip(result), ref["result"])
    if lin and ref["valid"] != "unknown":
        certify_version_cycles(result, ref)
    for name, recs in result["anomalies"].items() if isinstance(result["anomalies"], dict) else ():
        if name in abi.LC_AP_CLASSES:
            for rec in recs:
                assert rec["cycle"][0] is rec["cycle"][-1] and len(rec["steps"]) == len(rec["cycle"]) - 1
                assert all("value'" not in st for st in rec["steps"])
    return ref, s


def same_outputs(out, s, out0, s0):
    """Every array and every count of two calls (times apart)."""
    for name, a in out0.items():
        assert np.array_equal(out[name], a), name
    for f, v in s0.items():
        assert f.endswith("_ms") or s[f] == v, f


# ---------------------------------------------------------------- KATs

@pytest.mark.parametrize("combo", range(4), ids=COMBO_IDS)
@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(kat, combo):
    wfr, lin = COMBOS[combo]
    ref, s = agree_with_ref(kat["history"], wfr, lin)
    want = kat["expect"][COMBO_IDS[combo]]
    assert ref["valid"] == want["valid"], kat["why"]
    assert ref["result"]["anomaly-types"] == sorted(want["anomaly-types"]), kat["why"]
    assert {str(k): r["cyc_value"] for k, r in ref["keys"].items() if r["cyclic"]} == want["cyc"], kat["why"]
    if lin:
        for name, field in (("touches", "n_touches"), ("pairs", "n_pairs"), ("vedges", "n_vedges")):
            assert {str(k): r[field] for k, r in ref["lin"].items()} == want[name], (name, kat["why"])


def test_kats_cover_what_the_issue_names():
    names = {k["name"] for k in KATS}
    assert len(KATS) == 12 and len(names) == 12
    stale = next(k for k in KATS if k["name"] == "stale-read-across-blind-writes")
    assert stale["expect"]["wfr"]["valid"] is True and stale["expect"]["wfr+lin"]["valid"] is False


# ---------------------------------------------------------------- random tiny histories

N_RANDOM, AT_LEAST = 2000, 20
_refs = {}


def random_refs():
    """Seeds 0..1999 of wr_cases.random_history with the reference's four answers, computed once."""
    if not _refs:
        for seed in range(N_RANDOM):
            h = C.random_history(seed)
            _refs[seed] = (h, [REF.check(h, wfr, lin) for wfr, lin in COMBOS])
    return _refs


def kinds_of(refs):
    """Which of the issue's kinds a history is, from the reference alone."""
    wfr_only, both = refs[1], refs[3]
    cyc0 = {k for k, r in wfr_only["keys"].items() if r["cyclic"]}
    cyc1 = {k for k, r in both["keys"].items() if r["cyclic"]}
    kinds = set()
    if wfr_only["valid"] is True:
        kinds.add("valid-under-wfr")
        if cyc1:
            kinds.add("valid-to-cyclic")
    if cyc1 - cyc0:
        kinds.add("cyclic-only-with-lin")
    if any(REF.NIL in REF.REF._on_cycles(e) for e in both["vedges"].values()):
        kinds.add("cycle-through-nil")
    if not cyc1 and any((a, b) not in _base_edges(both, k) for k, e in both["vedges"].items() for a, b in e):
        kinds.add("lin-edges-no-cycle")
    return kinds


def _base_edges(ref, k):
    """Key k's initial and wfr edges, from the reference's txns."""
    out = set()
    for t, x in enumerate(ref["txns"]):
        first = None
        for i, (f, k2, v, _) in enumerate(x["mops"]):
            if k2 != k:
                continue
            if f == "w" and x["type"] != "fail":
                out.add((REF.NIL, v))
            if first is None:
                first = (f, v)
        if x["type"] == "ok" and first and first[0] == "r":
            ws = [v for f, k2, v, _ in x["mops"] if k2 == k and f == "w"]
            if ws:
                out.add((first[1], ws[-1]))
    return out


def test_random_histories_reach_every_kind():
    """From the reference alone, before anything is compared: at least 20
    histories of each kind, and at least 20 key instances with a lin edge into
    a value without a writer.  (Seeds 0-1999 give: valid under wfr alone 708,
    of which a key becomes cyclic with lin 22; a key cyclic only with lin 563;
    a cycle through nil 355; lin edges added and no key cyclic 1,325.)"""
    seen, writerless = {}, 0
    for h, refs in random_refs().values():
        for kind in kinds_of(refs):
            seen[kind] = seen.get(kind, 0) + 1
        written = {(k, m[2]) for x in refs[3]["txns"] for m in x["mops"] for k in [m[1]] if m[0] == "w"}
        writerless += sum(any((k, b) not in written and (a, b) not in _base_edges(refs[3], k) for a, b in e)
                          for k, e in refs[3]["vedges"].items())
    print("kinds:", seen, "keys with a lin edge into a writerless value:", writerless)
    for kind in ("valid-under-wfr", "valid-to-cyclic", "cyclic-only-with-lin", "cycle-through-nil", "lin-edges-no-cycle"):
        assert seen.get(kind, 0) >= AT_LEAST, (kind, seen)
    assert writerless >= AT_LEAST


@pytest.mark.parametrize("combo", range(4), ids=COMBO_IDS)
def test_random_histories_agree(combo):
    wfr, lin = COMBOS[combo]
    checker = WR.WrChecker(device=False, wfr_keys=wfr, linearizable_keys=True) if lin else None
    for i, (h, refs) in random_refs().items():
        try:
            agree_with_ref(h, wfr, lin, refs[combo], checker)
        except AssertionError as e:
            raise AssertionError("history %d: %s" % (i, e)) from e


# ---------------------------------------------------------------- the contract

class MarkedLinCall(abi._WrLinCall):
    """C.MarkedCall for the lin calls: every output filled with a marker first."""
    MARK = -77

    def __init__(self, txns, mops, flags, edge_cap=None):
        super().__init__(txns, mops, bool(flags & 1), bool(flags & 2), edge_cap)
        self.flags = flags
        for a in list(self.arrays.values()) + [self.lin_keys]:
            a.view(np.int8)[...] = self.MARK
        self.summary.valid = self.MARK
        self.lin_summary.n_touches = self.MARK

    def run(self, ctx=None):
        if ctx is None:
            return abi.lib().lc_wr_check_lin_host(*self.args())
        return abi.lib().lc_wr_check_lin(ctx._h, *self.args())

    def arrays_untouched(self):
        return all((a.view(np.int8) == np.int8(self.MARK)).all() for a in list(self.arrays.values()) + [self.lin_keys])

    def untouched(self):
        return self.summary.valid == self.MARK and self.lin_summary.n_touches == self.MARK and self.arrays_untouched()


def bad_inputs():
    """(name, txns, mops, flags) that the contract refuses."""
    enc = WR.encode(C.sequential(4))
    t, m = enc.txns, enc.mops
    out = [("flags-%d" % f, t, m, f) for f in (4, 8, 5, 16, 2 ** 31)]

    def with_(arr, i, field, v):
        a = arr.copy()
        a[field][i] = v
        return a
    out += [("inv-order", with_(t, 1, "inv_pos", 0), m, 3), ("comp-below-inv", with_(t, 0, "comp_pos", 0), m, 3),
            ("info-with-comp", with_(t, 0, "type", abi.LC_WR_INFO), m, 3), ("type", with_(t, 0, "type", 7), m, 3),
            ("tiling", with_(t, 1, "mop_off", 3), m, 3), ("key-reserved", t, with_(m, 0, "key", abi.LC_WR_NIL), 3),
            ("write-nil", t, with_(m, 1, "value", abi.LC_WR_NIL), 3), ("write-known", t, with_(m, 1, "known", 1), 3),
            ("read-unknown", t, with_(m, 0, "known", 0), 3), ("f", t, with_(m, 0, "f", 2), 3),
            ("two-writes", t, with_(m, 3, "value", 1), 3)]
    return out


@pytest.mark.parametrize("case", bad_inputs(), ids=[c[0] for c in bad_inputs()])
def test_einval_writes_nothing(case):
    _, txns, mops, flags = case
    call = MarkedLinCall(txns, mops, flags)
    assert call.run() == -errno.EINVAL and call.untouched()


def test_null_lin_keys_and_negative_cap_are_einval():
    enc = WR.encode(C.sequential(4))
    call = MarkedLinCall(enc.txns, enc.mops, 3)
    args = list(call.args())
    args[7] = None
    assert abi.lib().lc_wr_check_lin_host(*args) == -errno.EINVAL and call.untouched()
    call = MarkedLinCall(enc.txns, enc.mops, 3)
    call.out.edge_cap = -1
    assert call.run() == -errno.EINVAL and call.untouched()


def test_enospc_names_the_room_and_writes_no_array():
    enc = WR.encode(C.sequential(6))
    out, s, _ = abi.wr_check_lin_host(enc.txns, enc.mops, True, True)
    assert s["n_edges"] > 2
    call = MarkedLinCall(enc.txns, enc.mops, 3, edge_cap=int(s["n_edges"]) - 1)
    assert call.run() == -errno.ENOSPC and call.arrays_untouched()
    assert call.lin_summary.n_touches == call.MARK
    assert (call.summary.n_edges, call.summary.n_edges_raw, call.summary.valid) == (s["n_edges"], s["n_edges_raw"], 0)
    call = MarkedLinCall(enc.txns, enc.mops, 3, edge_cap=int(s["n_edges"]))
    assert call.run() == 0


def test_flag_off_equals_lc_wr_check_host_and_zero_records():
    for seed in range(50):
        enc = WR.encode(C.random_history(seed, n_txns=30))
        for wfr in (True, False):
            out, s, ls = abi.wr_check_lin_host(enc.txns, enc.mops, wfr, False)
            out0, s0 = abi.wr_check_host(enc.txns, enc.mops, wfr)
            same_outputs(out, s, out0, s0)
            assert not out["lin_keys"].view(np.int8).any() and not any(ls.values())


def test_limits_and_symbols():
    assert abi.has_wr_lin() and abi.LC_WR_LINEARIZABLE_KEYS == 2
    assert abi.wr_lin_limits() == {"max_key_versions": 512, "wave_key_versions": 64}
    assert abi.lib().lc_wr_lin_limits(None) == -errno.EINVAL
    assert ctypes.sizeof(abi.LcWrLinSummary) == 40


def test_checker_refuses_the_screened_and_restricted_forms():
    for kw in ({"device_scc": True}, {"device_cycles": True}):
        with pytest.raises(ValueError):
            WR.WrChecker(device=False, linearizable_keys=True, **kw)


def test_no_txns_is_unknown():
    out, s, ls = abi.wr_check_lin_host(np.zeros(0, abi.WR_TXN_DTYPE), np.zeros(0, abi.WR_MOP_DTYPE), True, True)
    assert s["valid"] == -1 and s["n_keys"] == 0 and not any(ls.values())


@pytest.mark.parametrize("seed", range(4))
def test_synth_is_valid_under_the_inference(seed):
    txns, mops = WR.synth_arrays(3000, seed=seed)
    out, s, ls = abi.wr_check_lin_host(txns, mops, True, True)
    assert s["valid"] == 1 and s["n_cyclic_keys"] == 0 and s["n_scc"] == 0
    assert ls["n_touches"] > 0 and 2.0 < ls["n_pairs"] / ls["n_touches"] < 4.0
    assert ls["n_vedges"] == int(out["lin_keys"]["n_vedges"].sum()) and ls["max_key_versions"] <= 33
