"""lc_append_check_screened against lc_append_check and lc_wr_check_screened
against lc_wr_check (the wfr inference on and off): every output array and
every count of the summary equal, the screen clean exactly on the histories
without an SCC; on the two checkers' KATs and on the 300 random histories of
tests/test_gpu_append.py's and tests/test_gpu_wr.py's generators.  Then the
Python checkers with device_scc=True against device_scc=False and against the
references."""
import ctypes
import errno

import numpy as np
import pytest

import append_cases as AC
import append_ref as AREF
import wr_cases as WC
import wr_ref as WREF
from jepsen.etcd_amd import abi, append as AP, wr as WR
from test_append import KATS as AP_KATS, strip_cycles as ap_strip
from test_gpu_append import COUNTS as AP_COUNTS, N_BULK
from test_gpu_wr import COUNTS as WR_COUNTS, bulk_history
from test_wr import KATS as WR_KATS, strip_cycles as wr_strip

pytestmark = pytest.mark.gpu

SCREEN_KEYS = {"clean", "label-rounds", "trim-rounds", "max-rounds", "rt-members", "trim-survivors", "kernel-ms", "ms"}


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def _same(want, ws, got, gs, scr, counts, what):
    for f in want:
        assert want[f].shape == got[f].shape, (what, f, want[f].shape, got[f].shape)
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), want[f][bad[:3]].tolist(), got[f][bad[:3]].tolist())
    assert [gs[k] for k in counts] == [ws[k] for k in counts], (what, gs, ws)
    if len(want["txn_flags"]):  # (a call without txns never reaches the screen's rounds)
        assert 1 <= scr["label_rounds"] <= scr["max_rounds"], (what, scr)
    assert (scr["clean"] == 1) == (ws["n_scc"] == 0), (what, scr, ws["n_scc"])
    assert scr["clean"] != 0 or scr["n_rt_members"] + scr["n_trim_survivors"] >= 2, (what, scr)
    assert scr["h2d_ms"] == 0
    return scr


def append_agree(ctx, enc, what=""):
    want, ws = ctx.append_check(enc.txns, enc.mops, enc.values)
    got, gs, scr = ctx.append_check_screened(enc.txns, enc.mops, enc.values)
    return _same(want, ws, got, gs, scr, AP_COUNTS, what)


def wr_agree(ctx, enc, wfr, what=""):
    want, ws = ctx.wr_check(enc.txns, enc.mops, wfr)
    got, gs, scr = ctx.wr_check_screened(enc.txns, enc.mops, wfr)
    return _same(want, ws, got, gs, scr, WR_COUNTS, what)


def test_append_kats(ctx):
    clean = 0
    for kat in AP_KATS:
        clean += append_agree(ctx, AP.encode(kat["history"]), kat["name"])["clean"] == 1
    assert 0 < clean < len(AP_KATS)


@pytest.mark.parametrize("wfr", (True, False), ids=("wfr", "no-wfr"))
def test_wr_kats(ctx, wfr):
    clean = 0
    for kat in WR_KATS:
        clean += wr_agree(ctx, WR.encode(kat["history"]), wfr, kat["name"])["clean"] == 1
    assert 0 < clean < len(WR_KATS)


def test_append_random_histories(ctx):
    seen = {1: 0, 0: 0, -1: 0}
    for i in range(N_BULK):  # tests/test_gpu_append.py's bulk histories
        h = AC.random_history(20000 + i, n_txns=5 + (i * 37) % 296, faults=AC.FAULTS + AC.SCRIPTED, p_fault=0.1,
                              sliding=True)
        seen[append_agree(ctx, AP.encode(h), i)["clean"]] += 1
    assert seen[1] and seen[0], seen  # (both the path that skips the host pass and the one that runs it)


def test_wr_random_histories(ctx):
    seen = {1: 0, 0: 0, -1: 0}
    for i in range(N_BULK):  # tests/test_gpu_wr.py's bulk histories
        enc = WR.encode(bulk_history(i))
        seen[wr_agree(ctx, enc, True, i)["clean"]] += 1
        if i % 3 == 0:
            wr_agree(ctx, enc, False, (i, "no-wfr"))
    assert seen[1] and seen[0], seen  # (both the path that skips the host pass and the one that runs it)


def test_a_screen_that_gives_up_leaves_the_host_pass(ctx, monkeypatch):
    """One round allowed: the screen proves nothing of a history whose labels
    move, and the call's results are the unscreened call's all the same."""
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "1")
    gave_up = 0
    for seed in range(12):
        enc = WR.encode(WC.random_history(900 + seed, n_txns=60, conc=8))
        want, ws = ctx.wr_check(enc.txns, enc.mops, True)
        got, gs, scr = ctx.wr_check_screened(enc.txns, enc.mops, True)
        assert all((want[f] == got[f]).all() for f in want) and [gs[k] for k in WR_COUNTS] == [ws[k] for k in WR_COUNTS]
        assert scr["clean"] in (-1, 0) or ws["n_scc"] == 0
        gave_up += scr["clean"] == -1
    assert gave_up


def test_errors_and_empty_calls_are_the_unscreened_call_s(ctx):
    none = (np.zeros(0, abi.AP_TXN_DTYPE), np.zeros(0, abi.AP_MOP_DTYPE), np.zeros(0, np.int64))
    out, s, scr = ctx.append_check_screened(*none)
    assert s["valid"] == -1 and (scr["clean"], scr["label_rounds"], scr["trim_rounds"]) == (1, 0, 0)
    out, s, scr = ctx.wr_check_screened(np.zeros(0, abi.WR_TXN_DTYPE), np.zeros(0, abi.WR_MOP_DTYPE))
    assert s["valid"] == -1 and (scr["clean"], scr["label_rounds"]) == (1, 0)
    # a contract violation: -EINVAL, nothing written, the summary of the screen neither; a good call after it
    good = AP.encode(AC.sequential(8))
    call = AC.MarkedCall(good.txns[::-1].copy(), good.mops, good.values)
    scr = abi.LcScreenSummary(clean=-77)
    rc = abi.lib().lc_append_check_screened(ctx._h, *call.args(), ctypes.byref(scr))
    assert rc == -errno.EINVAL and call.untouched() and scr.clean == -77
    append_agree(ctx, good, "after an error")
    good = WR.encode(WC.sequential(8))
    call = WC.MarkedCall(good.txns[::-1].copy(), good.mops)
    rc = abi.lib().lc_wr_check_screened(ctx._h, *call.args(), ctypes.byref(scr))
    assert rc == -errno.EINVAL and call.untouched() and scr.clean == -77
    wr_agree(ctx, good, True, "after an error")
    # scr may be null
    call = AC.MarkedCall(*[getattr(AP.encode(AC.sequential(8)), f) for f in ("txns", "mops", "values")])
    assert abi.lib().lc_append_check_screened(ctx._h, *call.args(), None) == 0 and call.summary.valid == 1


def test_append_checker_with_device_scc(ctx):
    on, off = AP.AppendChecker(device_mask=1, device_scc=True), AP.AppendChecker(device_mask=1)
    try:
        cleans = set()
        for seed, faults in ((1, ()), (2, ("stale", "split")), (3, ("garble", "leak", "behind")), (4, ("insert", "skew"))):
            h = AC.random_history(500 + seed, n_txns=40, faults=faults, p_fault=0.2, sliding=True)
            a, b = on.check({}, h, {}), off.check({}, h, {})
            sub = a.pop("scc-screen")
            assert "scc-screen" not in b and a == b, (seed, a, b)
            assert ap_strip(a) == AREF.check(h)["result"], seed
            assert set(sub) == SCREEN_KEYS and (sub["clean"] is True) == (on.last_summary["n_scc"] == 0)
            cleans.add(sub["clean"])
        assert cleans == {True, False}
    finally:
        on.close()
        off.close()


def test_wr_checker_with_device_scc(ctx):
    for wfr in (True, False):
        on, off = WR.WrChecker(device_mask=1, wfr_keys=wfr, device_scc=True), WR.WrChecker(device_mask=1, wfr_keys=wfr)
        try:
            for seed, faults in ((1, ()), (2, ("stale", "split")), (3, ("garble", "leak", "behind")),
                                 (4, ("double", "skew")), (5, ("loop", "g0"))):
                h = WC.random_history(500 + seed, n_txns=40, faults=faults, p_fault=0.2, sliding=True)
                a, b = on.check({}, h, {}), off.check({}, h, {})
                sub = a.pop("scc-screen")
                assert "scc-screen" not in b and a == b, (seed, a, b)
                assert wr_strip(a) == WREF.check(h, wfr)["result"], seed
                assert set(sub) == SCREEN_KEYS and (sub["clean"] is True) == (on.last_summary["n_scc"] == 0)
        finally:
            on.close()
            off.close()


def test_device_scc_without_the_symbol_is_the_unscreened_call(ctx, monkeypatch):
    monkeypatch.setattr(abi, "has_screened", lambda: False)
    on = WR.WrChecker(device_mask=1, device_scc=True)
    try:
        h = WC.sequential(12)
        assert "scc-screen" not in on.check({}, h, {}) and on.last_screen is None
    finally:
        on.close()
