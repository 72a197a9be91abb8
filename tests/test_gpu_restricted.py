"""lc_append_check_restricted against lc_append_check and
lc_wr_check_restricted against lc_wr_check (the wfr inference on and off), as
tests/test_gpu_screened.py compares the screened calls: every output array and
every count of the summary equal, on the two checkers' KATs, on the same 300
random histories per checker and on planted stale reads, with
LC_CYCLE_MIN_WORK=0 so that tiny histories reach the device.  Then the Python
checkers with device_cycles=True."""
import ctypes
import errno

import numpy as np
import pytest

import append_cases as AC
import append_ref as AREF
import planted_cycles as PC
import wr_cases as WC
import wr_ref as WREF
from jepsen.etcd_amd import abi, append as AP, wr as WR
from test_append import KATS as AP_KATS, strip_cycles as ap_strip
from test_gpu_append import COUNTS as AP_COUNTS, N_BULK
from test_gpu_screened import SCREEN_KEYS
from test_gpu_wr import COUNTS as WR_COUNTS, bulk_history
from test_wr import KATS as WR_KATS, strip_cycles as wr_strip

pytestmark = pytest.mark.gpu

SEARCH_KEYS = {"restricted", "marked", "device-searches", "device-queries", "host-fallbacks", "search-ms"}


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def every_search_on_the_device(monkeypatch):
    monkeypatch.setenv("LC_CYCLE_MIN_WORK", "0")


def _same(want, ws, got, gs, scr, srch, counts, what):
    for f in want:
        assert want[f].shape == got[f].shape, (what, f, want[f].shape, got[f].shape)
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), want[f][bad[:3]].tolist(), got[f][bad[:3]].tolist())
    assert [gs[k] for k in counts] == [ws[k] for k in counts], (what, gs, ws)
    assert scr["clean"] == -1 or (scr["clean"] == 1) == (ws["n_scc"] == 0), (what, scr, ws["n_scc"])
    # the marked pass ran exactly where the screen neither proved the graph clean nor gave up
    assert srch["restricted"] == (scr["clean"] == 0), (what, scr, srch)
    if srch["restricted"]:
        assert srch["n_marked"] >= int((want["scc"] >= 0).sum()) >= 2, (what, srch)
        assert srch["n_device_queries"] >= srch["n_device_searches"] and srch["n_host_fallbacks"] == 0, (what, srch)
        assert srch["search_ms"] >= 0
    else:
        assert [srch[k] for k in ("n_marked", "n_device_searches", "n_device_queries", "n_host_fallbacks",
                                  "search_ms")] == [0] * 5, (what, srch)
    return scr, srch


def append_agree(ctx, arrays, what=""):
    want, ws = ctx.append_check(*arrays)
    got, gs, scr, srch = ctx.append_check_restricted(*arrays)
    return _same(want, ws, got, gs, scr, srch, AP_COUNTS, what) + (want, ws)


def wr_agree(ctx, arrays, wfr, what=""):
    want, ws = ctx.wr_check(*arrays, wfr)
    got, gs, scr, srch = ctx.wr_check_restricted(*arrays, wfr)
    return _same(want, ws, got, gs, scr, srch, WR_COUNTS, what) + (want, ws)


def ap_arrays(history):
    enc = AP.encode(history)
    return enc.txns, enc.mops, enc.values


def wr_arrays(history):
    enc = WR.encode(history)
    return enc.txns, enc.mops


def test_append_kats(ctx):
    restricted = sum(append_agree(ctx, ap_arrays(kat["history"]), kat["name"])[1]["restricted"] for kat in AP_KATS)
    assert 0 < restricted < len(AP_KATS)


@pytest.mark.parametrize("wfr", (True, False), ids=("wfr", "no-wfr"))
def test_wr_kats(ctx, wfr):
    restricted = sum(wr_agree(ctx, wr_arrays(kat["history"]), wfr, kat["name"])[1]["restricted"] for kat in WR_KATS)
    assert 0 < restricted < len(WR_KATS)


def test_append_random_histories(ctx):
    restricted = searched = 0
    for i in range(N_BULK):  # tests/test_gpu_append.py's bulk histories
        h = AC.random_history(20000 + i, n_txns=5 + (i * 37) % 296, faults=AC.FAULTS + AC.SCRIPTED, p_fault=0.1,
                              sliding=True)
        srch = append_agree(ctx, ap_arrays(h), i)[1]
        restricted += srch["restricted"]
        searched += srch["n_device_searches"] > 0
    assert restricted and searched, (restricted, searched)


def test_wr_random_histories(ctx):
    restricted = searched = 0
    for i in range(N_BULK):  # tests/test_gpu_wr.py's bulk histories
        arrays = wr_arrays(bulk_history(i))
        srch = wr_agree(ctx, arrays, True, i)[1]
        restricted += srch["restricted"]
        searched += srch["n_device_searches"] > 0
        if i % 3 == 0:
            wr_agree(ctx, arrays, False, (i, "no-wfr"))
    assert restricted and searched, (restricted, searched)


@pytest.mark.parametrize("conc", PC.CONCS)
@pytest.mark.parametrize("back", PC.BACKS)
def test_planted_stale_reads(ctx, back, conc):
    """One stale read looking `back` txns back: one SCC of class
    G-single-realtime (6), its witness the unscreened call's, and which member
    closes it asked of the device.  Beside the issue's cases, the rw-register
    plant once more without the wfr inference, which orders no versions from
    such a history: it is valid there, and the call is the screened one."""
    for agree, arrays in ((append_agree, (PC.append_plant(back, conc),)), (wr_agree, (PC.wr_plant(back, conc), True)),
                          (wr_agree, (PC.wr_plant(back, conc), False))):
        scr, srch, want, ws = agree(ctx, *arrays, (back, conc))
        if arrays[-1] is False:
            assert ws["valid"] == 1 and scr["clean"] == 1 and srch["restricted"] == 0
            continue
        assert ws["n_scc"] == 1 and ws["n_class"][6] == 1 and len(want["steps"]) >= 2, ws
        assert srch["restricted"] == 1 and srch["n_device_searches"] >= 1 and srch["n_device_queries"] >= 1, srch
        assert srch["n_marked"] < len(arrays[0][0])


def test_a_data_only_g_single_is_decided_on_the_device(ctx):
    """Three txns that all overlap, so no real-time edge exists.  T0 reads x as
    [] and y as [1]; T1 appends x:1 and y:1; T2's read fixes x's order as [1].
    T1 -wr(y)-> T0 and T0 -rw(x)-> T1: a G-single (class 2, not 6), found at
    k = 2 with T0 as the only candidate."""
    h = [AC.op("invoke", 0, [["r", "x", None], ["r", "y", None]], 0),
         AC.op("invoke", 1, [["append", "x", 1], ["append", "y", 1]], 1),
         AC.op("invoke", 2, [["r", "x", None]], 2),
         AC.op("ok", 0, [["r", "x", []], ["r", "y", [1]]], 3),
         AC.op("ok", 1, [["append", "x", 1], ["append", "y", 1]], 4),
         AC.op("ok", 2, [["r", "x", [1]]], 5)]
    scr, srch, want, ws = append_agree(ctx, ap_arrays(h), "data-only G-single")
    assert ws["n_scc"] == 1 and ws["n_class"][2] == 1 and want["steps"]["txn"].tolist() == [0, 1], (ws, want["steps"])
    assert (srch["restricted"], srch["n_device_searches"], srch["n_device_queries"]) == (1, 1, 1), srch
    assert AREF.check(h)["result"]["anomaly-types"] == ["G-single"]


def test_a_screen_that_gives_up_leaves_the_whole_graph_pass(ctx, monkeypatch):
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "1")
    gave_up = 0
    for seed in range(12):
        scr, srch, want, ws = wr_agree(ctx, wr_arrays(WC.random_history(900 + seed, n_txns=60, conc=8)), True, seed)
        gave_up += scr["clean"] == -1
        assert scr["clean"] != -1 or srch["restricted"] == 0
    assert gave_up


def test_errors_and_empty_calls_are_the_screened_call_s(ctx):
    none = (np.zeros(0, abi.AP_TXN_DTYPE), np.zeros(0, abi.AP_MOP_DTYPE), np.zeros(0, np.int64))
    out, s, scr, srch = ctx.append_check_restricted(*none)
    assert s["valid"] == -1 and (scr["clean"], scr["label_rounds"], srch["restricted"]) == (1, 0, 0)
    out, s, scr, srch = ctx.wr_check_restricted(np.zeros(0, abi.WR_TXN_DTYPE), np.zeros(0, abi.WR_MOP_DTYPE))
    assert s["valid"] == -1 and (scr["clean"], scr["label_rounds"], srch["restricted"]) == (1, 0, 0)
    # a contract violation: -EINVAL, nothing written, neither summary; a good call after it
    scr, srch = abi.LcScreenSummary(clean=-77), abi.LcCycleSearchSummary(restricted=-77, n_marked=-77)
    good = AP.encode(AC.sequential(8))
    call = AC.MarkedCall(good.txns[::-1].copy(), good.mops, good.values)
    rc = abi.lib().lc_append_check_restricted(ctx._h, *call.args(), ctypes.byref(scr), ctypes.byref(srch))
    assert rc == -errno.EINVAL and call.untouched() and scr.clean == -77 and (srch.restricted, srch.n_marked) == (-77, -77)
    append_agree(ctx, (good.txns, good.mops, good.values), "after an error")
    append_agree(ctx, PC.append_plant(63, 1), "a restricted call after an error")
    good = WR.encode(WC.sequential(8))
    call = WC.MarkedCall(good.txns[::-1].copy(), good.mops)
    rc = abi.lib().lc_wr_check_restricted(ctx._h, *call.args(), ctypes.byref(scr), ctypes.byref(srch))
    assert rc == -errno.EINVAL and call.untouched() and scr.clean == -77 and (srch.restricted, srch.n_marked) == (-77, -77)
    wr_agree(ctx, (good.txns, good.mops), True, "after an error")
    # scr and srch may be null
    call = AC.MarkedCall(*PC.append_plant(63, 1))
    assert abi.lib().lc_append_check_restricted(ctx._h, *call.args(), None, None) == 0 and call.summary.n_scc == 1


def test_above_min_work_only(ctx, monkeypatch):
    """With the default min_work a tiny SCC takes the host loop, the pass still restricted."""
    monkeypatch.delenv("LC_CYCLE_MIN_WORK")
    scr, srch, want, ws = append_agree(ctx, PC.append_plant(2, 1), "default min_work")
    assert srch["restricted"] == 1 and srch["n_device_searches"] == 0 and ws["n_scc"] == 1


def test_append_checker_with_device_cycles(ctx):
    on, off = AP.AppendChecker(device_mask=1, device_cycles=True), AP.AppendChecker(device_mask=1)
    try:
        restricted = set()
        for seed, faults in ((1, ()), (2, ("stale", "split")), (3, ("garble", "leak", "behind")), (4, ("insert", "skew"))):
            h = AC.random_history(500 + seed, n_txns=40, faults=faults, p_fault=0.2, sliding=True)
            a, b = on.check({}, h, {}), off.check({}, h, {})
            scr, sub = a.pop("scc-screen"), a.pop("cycle-search")
            assert "cycle-search" not in b and a == b, (seed, a, b)
            assert ap_strip(a) == AREF.check(h)["result"], seed
            assert set(scr) == SCREEN_KEYS and set(sub) == SEARCH_KEYS
            assert sub["restricted"] is (scr["clean"] is False)
            restricted.add(sub["restricted"])
        assert restricted == {True, False}
    finally:
        on.close()
        off.close()


def test_wr_checker_with_device_cycles(ctx):
    for wfr in (True, False):
        on, off = WR.WrChecker(device_mask=1, wfr_keys=wfr, device_cycles=True), WR.WrChecker(device_mask=1, wfr_keys=wfr)
        try:
            for seed, faults in ((1, ()), (2, ("stale", "split")), (3, ("garble", "leak", "behind")),
                                 (4, ("double", "skew")), (5, ("loop", "g0"))):
                h = WC.random_history(500 + seed, n_txns=40, faults=faults, p_fault=0.2, sliding=True)
                a, b = on.check({}, h, {}), off.check({}, h, {})
                scr, sub = a.pop("scc-screen"), a.pop("cycle-search")
                assert "cycle-search" not in b and a == b, (seed, a, b)
                assert wr_strip(a) == WREF.check(h, wfr)["result"], seed
                assert set(scr) == SCREEN_KEYS and set(sub) == SEARCH_KEYS
                assert sub["restricted"] is (scr["clean"] is False)
        finally:
            on.close()
            off.close()


def test_device_cycles_without_the_symbol_is_device_scc(ctx, monkeypatch):
    monkeypatch.setattr(abi, "has_restricted", lambda: False)
    on = WR.WrChecker(device_mask=1, device_cycles=True)
    try:
        r = on.check({}, WC.sequential(12), {})
        assert "scc-screen" in r and "cycle-search" not in r and on.last_search is None
    finally:
        on.close()
    monkeypatch.setattr(abi, "has_screened", lambda: False)
    on = AP.AppendChecker(device_mask=1, device_cycles=True)
    try:
        r = on.check({}, AC.sequential(12), {})
        assert "scc-screen" not in r and "cycle-search" not in r
    finally:
        on.close()
