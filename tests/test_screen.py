"""lc_cycle_screen_host and screen.cycle_screen(device=False) against
tests/screen_ref.py (a reachability closure, no rounds): the hand-derived KATs
of tests/golden/screen_kat.json, the graphs of the two Elle checkers' KATs, and
2,000 random histories of tests/append_cases.py and tests/wr_cases.py (plus
composed ones for the one kind those never produce); every refusal."""
import errno
import json
import os
import random

import numpy as np
import pytest

import append_cases as AC
import append_ref as AREF
import screen_ref as REF
import wr_cases as WC
import wr_ref as WREF
from jepsen.etcd_amd import abi, append as AP, screen as SC, wr as WR

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "screen_kat.json")))["cases"]
AP_KATS = json.load(open(os.path.join(HERE, "golden", "append_kat.json")))["cases"]
WR_KATS = json.load(open(os.path.join(HERE, "golden", "wr_kat.json")))["cases"]
TYPE = {"ok": abi.LC_AP_OK, "info": abi.LC_AP_INFO, "fail": abi.LC_AP_FAIL}
EDGE = {"ww": abi.LC_AP_WW, "wr": abi.LC_AP_WR, "rw": abi.LC_AP_RW}
COUNTS = ("clean", "n_rt_members", "n_trim_survivors", "label_rounds", "trim_rounds", "max_rounds")


def arrays(txns, edges):
    """[(type name, inv_pos, comp_pos or None)], [(from, to, type, key)] -> the call's two arrays."""
    t = np.zeros(len(txns), dtype=abi.AP_TXN_DTYPE)
    for i, (typ, inv, comp) in enumerate(txns):
        t[i] = (0, inv, -1 if comp is None else comp, TYPE[typ], 0)
    e = np.zeros(len(edges), dtype=abi.AP_EDGE_DTYPE)
    for i, (a, b, typ, key) in enumerate(sorted(tuple(x) for x in edges)):
        e[i] = (a, b, typ, 0, key)
    return t, e


def ref_of(txns, edges):
    """The same spec as screen_ref.screen takes it."""
    return REF.screen([{"type": typ, "inv": inv, "comp": comp} for typ, inv, comp in txns],
                      {tuple(x) for x in edges})


def agree(ref, txns, edges, what=""):
    """Both host entry points against the reference's result; -> the summary."""
    for fn in (abi.cycle_screen_host, lambda t, e: SC.cycle_screen(t, e, device=False)):
        out, s = fn(txns, edges)
        for f in ("reach_lo", "reach_hi", "mark"):
            assert out[f].tolist() == ref[f], (what, f, out[f].tolist(), ref[f])
        in_rt = set().union(*ref["rt_sccs"]) if ref["rt_sccs"] else set()
        in_scc = set().union(*ref["sccs"]) if ref["sccs"] else set()
        mark = out["mark"]
        assert {t for t in range(len(mark)) if mark[t] & SC.RT} == in_rt, (what, "bit 0 <=> an SCC with an rt edge")
        assert all(mark[t] for t in in_scc), (what, "every member of an SCC has a bit")
        assert all(mark[t] == 0 for t in range(len(mark)) if txns["type"][t] == abi.LC_AP_FAIL), what
        assert (s["clean"] == 1) == ref["clean"] and s["clean"] in (0, 1), (what, s)
        assert s["n_rt_members"] == len(ref["flagged"]) and s["n_trim_survivors"] == len(ref["survivors"]), (what, s)
        assert 1 <= s["label_rounds"] <= s["max_rounds"] and 1 <= s["trim_rounds"] <= s["max_rounds"], (what, s)
    return s


# ---------------------------------------------------------------- KATs

@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(kat):
    ref = ref_of(kat["txns"], kat["edges"])
    for f in ("reach_lo", "reach_hi", "mark"):
        assert ref[f] == kat[f], (f, kat["why"])
    assert ref["clean"] == bool(kat["clean"]), kat["why"]
    s = agree(ref, *arrays(kat["txns"], kat["edges"]), what=kat["name"])
    for f in ("label_rounds", "trim_rounds"):
        if f in kat:
            assert s[f] == kat[f], (f, kat["why"])


def test_kats_cover_what_they_should():
    refs = {k["name"]: ref_of(k["txns"], k["edges"]) for k in KATS}
    cats = {name: REF.category(r) for name, r in refs.items()}
    for kind in ("clean", "rt-only", "data-only", "both", "stray-survivor"):
        assert any(c[kind] for c in cats.values()), kind
    assert any(len(s) == 3 and s not in r["rt_sccs"] for r in refs.values() for s in r["sccs"])
    assert any(all(t[0] == "info" for t in k["txns"]) for k in KATS)                      # no OK txn
    assert any(any(k["txns"][t][0] == "info" for s in refs[k["name"]]["sccs"] for t in s) for k in KATS)
    assert any(t[0] == "fail" for k in KATS for t in k["txns"])
    pair = refs["overlapping-pair-one-class-no-cycle"]
    assert pair["clean"] and len(set(zip(pair["reach_lo"], pair["reach_hi"]))) == 1 and not pair["survivors"]


def graph_of(history, which):
    """A history's graph twice: from the checker's reference (op level) and
    from the library's host checker (the arrays the screen is handed)."""
    if which == "append":
        ref = AREF.check(history)
        enc = AP.encode(history)
        out, _ = abi.append_check_host(enc.txns, enc.mops, enc.values)
    else:
        ref = WREF.check(history)
        enc = WR.encode(history)
        out, _ = abi.wr_check_host(enc.txns, enc.mops)
    edges = {(a, b, EDGE[typ], k) for a, b, typ, k in ref["edges"]}
    return ref["txns"], edges, enc.txns, out["edges"]


@pytest.mark.parametrize("which,kat", [("append", k) for k in AP_KATS] + [("wr", k) for k in WR_KATS],
                         ids=["append-" + k["name"] for k in AP_KATS] + ["wr-" + k["name"] for k in WR_KATS])
def test_checker_kat_graphs(which, kat):
    rtxns, redges, txns, edges = graph_of(kat["history"], which)
    agree(REF.screen(rtxns, redges), txns, edges, kat["name"])


# ---------------------------------------------------------------- random histories

N_RANDOM, N_COMPOSED, AT_LEAST = 2000, 40, 20
KINDS = ("clean", "rt-only", "data-only", "both", "stray-survivor")
_batch = []


def composed_history(seed):
    """What random_history never produced in 7,000 tries: two data cycles in
    one (H, K) class with a txn between them.  Built from wr_cases.op: two
    write cycles of wr_cases.script's g0 shape on keys of their own, A and B,
    and a chain of 1 to 3 joiners from A to B, all of them overlapping; the
    order of the invokes and of the completions is drawn at random (in three
    of four histories with a txn of A invoked last and one of B completed
    first, which makes one class of them all), and some histories have a
    sequential txn before or after.  Which kind a history is,
    the reference says."""
    rng = random.Random(seed)
    val = iter(range(1, 1000))
    ax1, ax2, ay1, ay2, bx1, bx2, by1, by2 = (next(val) for _ in range(8))
    n_join = rng.randint(1, 3)
    links = [next(val) for _ in range(n_join)]
    txs = [[["r", 10, ax2], ["w", 10, ax1], ["w", 11, ay1]],
           [["r", 11, ay1], ["w", 11, ay2], ["w", 10, ax2]]]
    for i in range(n_join):  # joiner i reads what the one before wrote (the first: A's y2) and writes link i
        txs.append([["r", 11, ay2] if i == 0 else ["r", 30 + i - 1, links[i - 1]], ["w", 30 + i, links[i]]])
    txs += [[["r", 30 + n_join - 1, links[-1]], ["r", 20, bx2], ["w", 20, bx1], ["w", 21, by1]],
            [["r", 21, by1], ["w", 21, by2], ["w", 20, bx2]]]
    h = []
    if rng.random() < 0.4:
        h += [WC.op("invoke", 100, [["w", 50, 900]], len(h)), WC.op("ok", 100, [["w", 50, 900]], len(h) + 1)]
    inv, comp = list(range(len(txs))), list(range(len(txs)))
    rng.shuffle(inv)
    rng.shuffle(comp)
    if rng.random() < 0.75:  # one class for all: A's txn invoked last reaches all, B's completed first is reached by all
        a, b = rng.randrange(2), len(txs) - 1 - rng.randrange(2)
        inv.append(inv.pop(inv.index(a)))
        comp.insert(0, comp.pop(comp.index(b)))
    for p in inv:
        h.append(WC.op("invoke", p, [[f, k, None if f == "r" else v] for f, k, v in txs[p]], len(h)))
    for p in comp:
        h.append(WC.op("ok", p, [list(m) for m in txs[p]], len(h)))
    if rng.random() < 0.4:
        h += [WC.op("invoke", 101, [["r", 50, None]], len(h)), WC.op("ok", 101, [["r", 50, None]], len(h) + 1)]
    return h


def batch():
    """[(name, the reference's txns and edges, the library's arrays, screen_ref's result)], made once."""
    if not _batch:
        for seed in range(N_RANDOM // 2):
            for which, cases in (("append", AC), ("wr", WC)):
                g = graph_of(cases.random_history(seed), which)
                _batch.append(("%s %d" % (which, seed), g, REF.screen(g[0], g[1])))
        for seed in range(N_COMPOSED):
            g = graph_of(composed_history(seed), "wr")
            _batch.append(("composed %d" % seed, g, REF.screen(g[0], g[1])))
    return _batch


def test_batch_holds_every_kind():
    """From the reference alone: each kind in at least 20 histories."""
    seen = dict.fromkeys(KINDS, 0)
    for _, _, ref in batch():
        for kind, is_one in REF.category(ref).items():
            seen[kind] += is_one
    assert all(seen[k] >= AT_LEAST for k in KINDS), seen


def test_batch_agrees():
    for name, (_, _, txns, edges), ref in batch():
        agree(ref, txns, edges, name)


# ---------------------------------------------------------------- refusals and limits

class MarkedCall(abi._ScreenCall):
    """A call whose outputs are filled with a marker first, so that a call
    that must write nothing can be seen to have written nothing."""
    MARK = -77

    def __init__(self, txns, edges):
        super().__init__(txns, edges)
        for a in self.arrays.values():
            a.view(np.int8)[...] = self.MARK
        self.summary.clean = self.MARK
        self.summary.max_rounds = self.MARK

    def run(self, ctx=None):
        if ctx is None:
            return abi.lib().lc_cycle_screen_host(*self.args())
        return abi.lib().lc_cycle_screen(ctx._h, *self.args())

    def untouched(self):
        return (self.summary.clean, self.summary.max_rounds) == (self.MARK, self.MARK) and \
            all((a.view(np.int8) == np.int8(self.MARK)).all() for a in self.arrays.values())


GOOD = ([("ok", 0, 2), ("fail", 1, 3), ("info", 4, None), ("ok", 5, 6)], [(0, 2, 0, 1), (0, 3, 1, 1), (2, 3, 2, 1)])


def _bad(what):
    txns, edges = arrays(*GOOD)
    if what == "txns-unsorted":
        txns["inv_pos"][2] = 1
    elif what == "txns-equal-inv":
        txns["inv_pos"][1] = 0
    elif what == "inv-too-large":
        txns["inv_pos"][3], txns["comp_pos"][3] = 2 ** 31 - 1, 2 ** 31 - 1
    elif what == "info-with-comp":
        txns["comp_pos"][2] = 9
    elif what == "comp-not-above-inv":
        txns["comp_pos"][3] = 5
    elif what == "comp-too-large":
        txns["comp_pos"][3] = 2 ** 31 - 1
    elif what == "unknown-type":
        txns["type"][0] = 3
    elif what == "edge-to-fail":
        edges["to"][0] = 1
    elif what == "edge-from-fail":
        edges[0] = (1, 2, 0, 0, 1)
    elif what == "edge-end-negative":
        edges["from"][0] = -1
    elif what == "edge-end-past-the-txns":
        edges["to"][2] = 4
    elif what == "edge-to-itself":
        edges[2] = (3, 3, 0, 0, 1)
    elif what == "edges-unsorted":
        edges[[0, 1]] = edges[[1, 0]]
    elif what == "edges-unsorted-by-key":
        edges = edges[[0, 0, 1, 2]]
        edges["key"][0] = 2
    elif what == "edges-twice":
        edges = edges[[0, 1, 1, 2]]
    else:
        raise KeyError(what)
    return txns, edges


EINVAL_CASES = ("txns-unsorted", "txns-equal-inv", "inv-too-large", "info-with-comp", "comp-not-above-inv",
                "comp-too-large", "unknown-type", "edge-to-fail", "edge-from-fail", "edge-end-negative",
                "edge-end-past-the-txns", "edge-to-itself", "edges-unsorted", "edges-unsorted-by-key", "edges-twice")


def test_the_good_call_is_good():
    call = MarkedCall(*arrays(*GOOD))
    assert call.run() == 0 and not call.untouched()
    agree(ref_of(*GOOD), *arrays(*GOOD))


@pytest.mark.parametrize("what", EINVAL_CASES)
def test_einval_writes_nothing(what):
    call = MarkedCall(*_bad(what))
    assert call.run() == -errno.EINVAL and call.untouched()


@pytest.mark.parametrize("missing", ("reach_lo", "reach_hi", "mark", "out"))
def test_null_out_is_einval(missing):
    call = MarkedCall(*arrays(*GOOD))
    args = list(call.args())
    if missing == "out":
        args[4] = None
    else:
        setattr(call.out, missing, None)
    assert abi.lib().lc_cycle_screen_host(*args) == -errno.EINVAL and call.untouched()
    assert abi.lib().lc_screen_limits(None) == -errno.EINVAL


def test_no_txns_is_clean():
    out, s = abi.cycle_screen_host(np.zeros(0, dtype=abi.AP_TXN_DTYPE), np.zeros(0, dtype=abi.AP_EDGE_DTYPE))
    assert all(len(a) == 0 for a in out.values())
    assert [s[f] for f in COUNTS[:5]] == [1, 0, 0, 0, 0]
    call = MarkedCall(np.zeros(0, dtype=abi.AP_TXN_DTYPE), np.zeros(0, dtype=abi.AP_EDGE_DTYPE))
    args = list(call.args())
    args[5] = None  # sum may be null
    assert abi.lib().lc_cycle_screen_host(*args) == 0


def against_order(hops):
    """hops + 1 INFO txns, txn i + 1 -> txn i: K takes one round per hop.  At the
    fixpoint all have one (H, K), so the trim takes the chain apart from both
    ends: (hops + 2) // 2 rounds that drop something and a quiet one."""
    return arrays([("info", i, None) for i in range(hops + 1)], [(i + 1, i, 0, 1) for i in range(hops)])


def test_rounds_follow_the_graph_and_the_limit(monkeypatch):
    lim = SC.limits()
    assert lim["max_rounds"] == lim["default_max_rounds"] >= 2
    assert lim["default_max_rounds"] & (lim["default_max_rounds"] - 1) == 0
    for hops in (1, 2, 5):
        _, s = abi.cycle_screen_host(*against_order(hops))
        assert (s["clean"], s["label_rounds"], s["trim_rounds"]) == (1, hops + 1, (hops + 2) // 2 + 1)
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "8")
    assert SC.limits() == {"max_rounds": 8, "default_max_rounds": lim["default_max_rounds"]}
    for hops, clean, rounds in ((6, 1, 7), (7, 1, 8), (8, -1, 8), (9, -1, 8)):
        out, s = abi.cycle_screen_host(*against_order(hops))
        assert (s["clean"], s["label_rounds"], s["max_rounds"]) == (clean, rounds, 8), hops
        assert s["trim_rounds"] == ((hops + 2) // 2 + 1 if clean == 1 else 0) and not out["mark"].any()
        # a screen that gave up still has sound labels: K never above the fixpoint's
        assert (out["reach_hi"] <= hops).all() and (out["reach_hi"][-1] == hops)
    for bad in ("0", "-3", "x"):
        monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", bad)
        assert SC.limits()["max_rounds"] == lim["default_max_rounds"]
    # the trim gives up the same way: an in-class chain loses one node at each end per round
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "40")
    n = 31  # all overlapping, txn i + 1 -> txn i, and a 2-cycle at each end pins (H, K) for all
    txns = [("ok", i, 100 + i) for i in range(n)]
    edges = [(i + 1, i, 0, 1) for i in range(n - 1)] + [(0, 1, 0, 2), (n - 2, n - 1, 0, 2)]
    ref = ref_of(txns, edges)
    assert len(ref["survivors"]) == n and len(set(zip(ref["reach_lo"], ref["reach_hi"]))) == 1
    agree(ref, *arrays(txns, edges))
    edges = edges[:-2]  # without the cycles: an acyclic in-class chain, emptied from both ends
    ref = ref_of(txns, edges)
    assert ref["clean"] and len(set(zip(ref["reach_lo"], ref["reach_hi"]))) == 1
    s = agree(ref, *arrays(txns, edges))
    assert s["trim_rounds"] == (n + 1) // 2 + 1
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "31")  # (the labels take n rounds)
    out, s = abi.cycle_screen_host(*arrays(txns, edges))
    assert (s["clean"], s["trim_rounds"]) == (1, 17)
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "30")
    out, s = abi.cycle_screen_host(*arrays(txns, edges))
    assert s["clean"] == -1 and s["label_rounds"] == 30
