"""lc_perf_stats_host and jepsen/etcd_amd/perfstats.py against the hand-derived
cases of tests/golden/perfstats_kat.json and against tests/perfstats_ref.py, an
independent restatement (sorted by (process, position), dicts).  Everything is
integer-exact.  No GPU."""
import json
import os
import random

import numpy as np
import pytest

import perfstats_ref as R
from jepsen.etcd_amd import abi, perfstats as P
from jepsen.etcd_amd.setfull import Unsupported

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "perfstats_kat.json")))["cases"]
TABLES = ("by_f", "comp_pos", "latency_ns", "rate", "quant", "quant_n")
EINVAL, E2BIG, ENOSPC = -22, -7, -28


def events_of(rows):
    ev = np.zeros(len(rows), dtype=abi.PS_EVENT_DTYPE)
    for i, (t, p, f, ty) in enumerate(rows):
        ev[i] = (t, p, f, ty, 0)
    return ev


def assert_equal(out, s, want, want_s, what=""):
    for name in TABLES:
        got = out[name].tolist()
        assert got == want[name], (what, name, got, want[name])
    assert {k: s[k] for k in R.COUNTERS} == want_s, (what, s, want_s)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_known_answers(kat):
    out, s = abi.perf_stats_host(events_of(kat["events"]), kat["n_f"], kat["qs"], kat["rate_dt"], kat["quant_dt"])
    assert_equal(out, s, kat, kat["summary"], kat["name"])
    # and the reference agrees with the hand-derived values
    ref, ref_s = R.reference([tuple(e) for e in kat["events"]], kat["n_f"], kat["qs"], kat["rate_dt"],
                             kat["quant_dt"])
    assert all(ref[name] == kat[name] for name in TABLES) and ref_s == kat["summary"]


def random_history(rng, n, n_proc, n_f, crash, t_step, nemesis=0.05):
    """A seeded history: processes invoke and complete; an :info renumbers the
    process (a crash), some completions come without an invoke, some invokes
    twice, some completions change f, clocks sometimes step back."""
    rows, t = [], rng.randrange(0, 3 * t_step + 1)
    procs = list(range(n_proc))
    pending = {}
    next_id = n_proc
    while len(rows) < n:
        t = max(0, t + rng.randrange(-t_step // 4, t_step + 1))
        if rng.random() < nemesis:
            rows.append((t, -1 - rng.randrange(3), rng.randrange(n_f), rng.randrange(4)))
            continue
        i = rng.randrange(len(procs))
        p = procs[i]
        if p in pending and rng.random() < 0.9:
            f = pending.pop(p)
            if rng.random() < 0.03:
                f = rng.randrange(n_f)
            ty = 3 if rng.random() < crash else rng.choice((1, 1, 1, 2))
            rows.append((t, p, f, ty))
            if ty == 3:
                procs[i] = next_id
                next_id += n_proc
        elif rng.random() < 0.03:
            rows.append((t, p, rng.randrange(n_f), rng.choice((1, 2, 3))))  # a completion with no invoke
        else:
            pending[p] = rng.randrange(n_f)
            rows.append((t, p, pending[p], 0))
    return rows


def test_against_the_reference_on_random_histories():
    rng = random.Random(0x9E5F)
    sizes = [0, 1, 2, 3, 5, 17, 64, 65, 200, 500, 1000, 3000]
    for i in range(240):
        n = sizes[i % len(sizes)] if i < 200 else rng.randrange(0, 4000)
        n_proc, n_f = rng.randint(1, 40), rng.randint(1, 70)
        crash = rng.choice((0.0, 0.01, 0.2))
        t_step = rng.choice((1, 7, 1000, 10 ** 9))
        rate_dt = rng.choice((1, 3, 10, 1000, 10 ** 9, 10 ** 10)) if t_step < 10 ** 9 else 10 ** 10
        quant_dt = rate_dt * rng.choice((1, 3)) + rng.choice((0, 1))
        if n * t_step // min(rate_dt, quant_dt) > 20000:
            rate_dt = quant_dt = max(1, n * t_step // 500)
        qs = rng.choice(([0.5, 0.95, 0.99, 1.0], [], [0.0], [1.0, 0.0, 0.25], [i / 7 for i in range(8)]))
        rows = random_history(rng, n, n_proc, n_f, crash, t_step)
        out, s = abi.perf_stats_host(events_of(rows), n_f, qs, rate_dt, quant_dt)
        want, want_s = R.reference(rows, n_f, qs, rate_dt, quant_dt)
        assert_equal(out, s, want, want_s, (i, n, n_proc, n_f))
        if i % 10 == 0:  # the tables do not depend on the point arrays
            out2, s2 = abi.perf_stats_host(events_of(rows), n_f, qs, rate_dt, quant_dt, points=False)
            assert out2["comp_pos"] is None and out2["latency_ns"] is None
            assert all((out2[k] == out[k]).all() for k in ("by_f", "rate", "quant", "quant_n"))
            assert {k: s2[k] for k in R.COUNTERS} == want_s


OK_ROWS = [(0, 0, 0, 0), (5, 0, 0, 1)]


def refused(rows, n_f=1, **kw):
    with pytest.raises(abi.LcError) as e:
        abi.perf_stats_host(events_of(rows), n_f, **kw)
    return e.value.code


def test_refusals():
    assert refused([(-1, 0, 0, 0)]) == EINVAL                      # a negative time
    assert refused([(-1, -1, 0, 0)]) == EINVAL                     # ... of a nemesis op too
    assert refused([(0, 0, 0, 4)]) == EINVAL                       # a type above 3
    assert refused([(0, 0, 1, 0)]) == EINVAL                       # a client's f >= n_f
    assert refused([(0, 0, 2, 1)], n_f=2) == EINVAL
    abi.perf_stats_host(events_of([(0, -1, 9, 3)]), 1)             # a nemesis op's f is not looked at
    assert refused(OK_ROWS, n_f=0) == EINVAL
    assert refused(OK_ROWS, n_f=-3) == EINVAL
    assert refused(OK_ROWS, qs=[0.5] * 9) == EINVAL                # n_q outside [0, 8]
    assert refused(OK_ROWS, qs=[1.0000001]) == EINVAL
    assert refused(OK_ROWS, qs=[-0.1]) == EINVAL
    assert refused(OK_ROWS, qs=[float("nan")]) == EINVAL
    assert refused(OK_ROWS, rate_dt_ns=0) == EINVAL
    assert refused(OK_ROWS, quant_dt_ns=0) == EINVAL
    assert refused(OK_ROWS, rate_dt_ns=-5) == EINVAL
    lim = abi.perf_stats_limits()
    assert refused(OK_ROWS, n_f=lim["max_f"] + 1) == E2BIG
    abi.perf_stats_host(events_of(OK_ROWS), lim["max_f"])
    big = [(0, 0, 0, 0), (lim["max_table_entries"], 0, 0, 1)]      # n_f * 3 * (t_max / 1 + 1) entries
    assert refused(big, rate_dt_ns=1, quant_dt_ns=10 ** 9) == E2BIG
    assert refused(big, rate_dt_ns=10 ** 9, quant_dt_ns=1) == E2BIG
    # 3 (2^22 + 1) and 4 (2^21 + 1) entries: both below the bound
    abi.perf_stats_host(events_of(big), 1, rate_dt_ns=4, quant_dt_ns=8)


def test_n_events_of_2_to_the_31_is_refused_before_the_array_is_read():
    p = abi.LcPsParams(n_f=1, n_q=0, rate_dt_ns=1, quant_dt_ns=1)
    room = np.zeros(8, dtype=np.int64)
    out = abi.LcPsOut(by_f=abi._ptr(room), rate=abi._ptr(room), quant_n=abi._ptr(room), rate_cap=1, quant_cap=1)
    s = abi.LcPsSummary()
    import ctypes
    ev = events_of(OK_ROWS)
    for n in (2 ** 31, -1):
        assert abi.lib().lc_perf_stats_host(abi._ptr(ev), n, ctypes.byref(p), ctypes.byref(out),
                                            ctypes.byref(s)) == EINVAL


def test_enospc_then_a_call_with_room():
    rows = [(0, 0, 0, 0), (95, 0, 0, 1), (96, 1, 0, 0)]
    with pytest.raises(abi.LcError) as e:
        abi.perf_stats_host(events_of(rows), 1, rate_dt_ns=10, quant_dt_ns=30, rate_cap=9, quant_cap=4)
    assert e.value.code == ENOSPC and e.value.needed == (10, 4)
    with pytest.raises(abi.LcError) as e:
        abi.perf_stats_host(events_of(rows), 1, rate_dt_ns=10, quant_dt_ns=30, rate_cap=10, quant_cap=3)
    assert e.value.code == ENOSPC and e.value.needed == (10, 4)
    out, s = abi.perf_stats_host(events_of(rows), 1, rate_dt_ns=10, quant_dt_ns=30, rate_cap=e.value.needed[0],
                                 quant_cap=e.value.needed[1])
    want, want_s = R.reference(rows, 1, list(abi.PS_DEFAULT_QS), 10, 30)
    assert_equal(out, s, want, want_s)
    # more room than needed: the rest of every row is written too
    out, s = abi.perf_stats_host(events_of(rows), 1, rate_dt_ns=10, quant_dt_ns=30, rate_cap=13, quant_cap=6)
    assert out["rate"][:, :, :10].tolist() == want["rate"] and (out["rate"][:, :, 10:] == 0).all()
    assert out["quant"][:, :4].tolist() == want["quant"] and (out["quant"][:, 4:] == abi.LC_PS_NONE).all()
    assert out["quant_n"][:, :4].tolist() == want["quant_n"] and (out["quant_n"][:, 4:] == 0).all()


# min(n - 1, floor(q n)), written out: q n integral or within an ulp of it
QUANTILE_CASES = {
    1: {0.5: 0, 0.95: 0, 0.99: 0, 1.0: 0, 0.0: 0},
    2: {0.5: 1, 0.95: 1, 0.99: 1, 1.0: 1, 0.0: 0},
    20: {0.5: 10, 0.95: 19, 0.99: 19, 1.0: 19, 0.0: 0},
    100: {0.5: 50, 0.95: 95, 0.99: 99, 1.0: 99, 0.0: 0},
    200: {0.5: 100, 0.95: 190, 0.99: 198, 1.0: 199, 0.0: 0},
}


@pytest.mark.parametrize("n", sorted(QUANTILE_CASES))
def test_quantile_index(n):
    qs = sorted(QUANTILE_CASES[n])
    # n pairs on n processes, one group, latencies 1000 .. 1000 + n - 1 in a shuffled order
    lats = list(range(1000, 1000 + n))
    random.Random(n).shuffle(lats)
    rows = [(0, p, 0, 0) for p in range(n)] + [(lats[p], p, 0, 1) for p in range(n)]
    out, s = abi.perf_stats_host(events_of(rows), 1, qs, 10 ** 6, 10 ** 6)
    assert s["n_pairs"] == n and out["quant_n"].tolist() == [[n]]
    assert out["quant"][0, 0].tolist() == [1000 + QUANTILE_CASES[n][q] for q in qs]


def op(t, process, ty, f, **kw):
    return dict({"time": t, "process": process, "type": ty, "f": f}, **kw)


HISTORY = [
    op(0, 0, "invoke", "read"), op(1 * 10 ** 9, 0, "ok", "read"),
    op(2 * 10 ** 9, 1, ":invoke", ":write"), op(3 * 10 ** 9, ":nemesis", "info", "start-partition"),
    op(12 * 10 ** 9, 1, ":fail", ":write"),
    op(13 * 10 ** 9, 0, "invoke", "read"), op(31 * 10 ** 9, 0, "info", "read"),
    op(32 * 10 ** 9, 2, "invoke", "cas"),
]


def test_stats_checker():
    r = P.StatsChecker(device=False).check({}, HISTORY, {})
    assert r == {"valid?": False, "count": 3, "ok-count": 1, "fail-count": 1, "info-count": 1,
                 "by-f": {"read": {"valid?": True, "count": 2, "ok-count": 1, "fail-count": 0, "info-count": 1},
                          "write": {"valid?": False, "count": 1, "ok-count": 0, "fail-count": 1, "info-count": 0}}}
    ok = P.StatsChecker(device=False).check({}, HISTORY[:2], {})
    assert ok["valid?"] is True and list(ok["by-f"]) == ["read"]
    assert P.StatsChecker(device=False).check({}, [], {})["valid?"] is True


def test_perf_checker():
    ch = P.PerfChecker(device=False, points=True)
    r = ch.check({}, HISTORY, {})
    assert r["valid?"] is True
    # read: latencies 1 s (invoke at 0 s, bucket 0) and 18 s (invoke at 13 s, bucket 0); write: 10 s
    assert r["latency-quantiles"] == {
        "read": {0.5: [[15.0, 18000.0]], 0.95: [[15.0, 18000.0]], 0.99: [[15.0, 18000.0]], 1.0: [[15.0, 18000.0]]},
        "write": {q: [[15.0, 10000.0]] for q in (0.5, 0.95, 0.99, 1.0)}}
    assert r["rate"] == {"read": {"ok": [[5.0, 0.1]], "info": [[35.0, 0.1]]}, "write": {"fail": [[15.0, 0.1]]}}
    assert r["latencies"] == {"read": {"ok": [[0.0, 1000.0]], "info": [[13.0, 18000.0]]},
                              "write": {"fail": [[2.0, 10000.0]]}}
    assert (r["n-events"], r["n-client"], r["n-pairs"], r["n-pending"]) == (8, 7, 3, 1)
    assert "latencies" not in P.PerfChecker(device=False).check({}, HISTORY, {})
    assert ch.last_summary["n_quant_buckets"] == 2 and ch.last_summary["n_rate_buckets"] == 4


def test_encode():
    ev, names = P.encode(HISTORY)
    assert names == ["read", "write", "cas"]
    assert ev["process"].tolist() == [0, 0, 1, -1, 1, 0, 0, 2] and ev["f"].tolist() == [0, 0, 1, 0, 1, 0, 0, 2]
    assert ev["type"].tolist() == [0, 1, 0, 3, 2, 0, 3, 0]
    with pytest.raises(Unsupported):
        P.encode([{"process": 0, "type": "invoke", "f": "read"}])
    with pytest.raises(Unsupported):
        P.encode([op(1.5, 0, "invoke", "read")])


class Raises:
    def check(self, test, history, opts=None):
        raise RuntimeError("boom")


class Says:
    def __init__(self, valid):
        self.valid = valid

    def check(self, test, history, opts=None):
        return {"valid?": self.valid}


def test_compose():
    r = P.compose({"stats": P.StatsChecker(device=False), "perf": P.PerfChecker(device=False)}).check({}, HISTORY, {})
    assert set(r) == {"stats", "perf", "valid?"} and r["valid?"] is False and r["perf"]["valid?"] is True
    r = P.compose({"stats": P.StatsChecker(device=False), "perf": P.PerfChecker(device=False)}).check(
        {}, HISTORY[:2], {})
    assert r["valid?"] is True
    assert P.compose({"a": Says(True), "b": Says("unknown")}).check({}, [], {})["valid?"] == "unknown"
    assert P.compose({"a": Says(False), "b": Says("unknown")}).check({}, [], {})["valid?"] is False
    assert P.compose({}).check({}, [], {}) == {"valid?": True}


def test_compose_with_a_raising_checker():
    r = P.compose({"stats": P.StatsChecker(device=False), "workload": Raises()}).check({}, HISTORY[:2], {})
    assert r["workload"]["valid?"] == "unknown" and "boom" in r["workload"]["error"]
    assert r["stats"]["valid?"] is True and r["valid?"] == "unknown"
    r = P.compose({"stats": P.StatsChecker(device=False), "workload": Raises()}).check({}, HISTORY, {})
    assert r["valid?"] is False  # false over unknown
