"""lc_cycle_reach_host (include/lincheck_cycles.h) against tests/cycles_ref.py
on the hand-written KATs of tests/golden/cycles_kat.json and on 200 random
graphs; its contract; and cycles_host_marked against cycles_host through
lc_cycles_host, on the two Elle checkers' KATs, on the random histories of
tests/test_gpu_screened.py and on the planted stale reads, the class loop's
searches answered by the host loop and again by a hook that answers from
tests/cycles_ref.py.  No GPU."""
import errno
import json
import os

import numpy as np
import pytest

import append_cases as AC
import cycles_ref as REF
import planted_cycles as PC
import wr_cases as WC
from jepsen.etcd_amd import abi, append as AP, cycles as CY, wr as WR
from test_append import KATS as AP_KATS
from test_wr import KATS as WR_KATS

HERE = os.path.dirname(os.path.abspath(__file__))
KATS = json.load(open(os.path.join(HERE, "golden", "cycles_kat.json")))["cases"]
N_BULK = 300  # tests/test_gpu_append.py's and tests/test_gpu_wr.py's


def kat_arrays(kat):
    return (kat["n_nodes"],) + tuple(REF.csr(kat["n_nodes"], kat["edges"])) + tuple(REF.queries(kat["queries"]))


def random_graph(seed):
    """1..300 nodes, sparse to dense, queries on a random subset of the nodes
    with 0..4 heads each."""
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 301))
    n_edges = int(rng.integers(0, 3 * n + 1))
    edges = [(int(a), int(b)) for a, b in rng.integers(0, n, (n_edges, 2))]
    qs = []
    for src in np.nonzero(rng.random(n) < rng.choice((0.05, 0.3, 1.0)))[0]:
        heads = [int(h) for h in rng.integers(0, n, int(rng.integers(0, 5))) if h != src]
        qs.append((int(src), heads))
    return (n,) + tuple(REF.csr(n, edges)) + tuple(REF.queries(qs))


def host_reach(*args, **kw):
    return CY.cycle_reach(*args, device=False, **kw)


def agree_with_ref(args, what, run=host_reach):
    """Both modes of `run` (the host's by default) against the reference."""
    want_hit, want_first, want_visited = REF.reach(*args)
    hit, s = run(*args, all_queries=True)
    assert hit.tolist() == want_hit, what
    assert (s["first_hit"], s["nodes_visited"], s["n_queries_run"]) == (want_first, want_visited, len(want_hit)), what
    hit, s = run(*args)
    assert hit is None and s["first_hit"] == want_first, what
    return want_first


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(kat):
    args = kat_arrays(kat)
    assert REF.reach(*args) == (kat["hit"], kat["first_hit"], kat["nodes_visited"])  # (the reference itself)
    assert agree_with_ref(args, kat["name"]) == kat["first_hit"]


def test_random_graphs():
    firsts = [agree_with_ref(random_graph(seed), seed) for seed in range(200)]
    assert sum(f == -1 for f in firsts) >= 20 and sum(f > 0 for f in firsts) >= 20, firsts


def test_the_early_exit_does_less():
    """Without LC_REACH_ALL the host stops at the first hitting query, and at its first head."""
    args = kat_arrays(next(k for k in KATS if k["name"].startswith("two hitting")))
    _, s = CY.cycle_reach(*args, device=False)
    assert (s["first_hit"], s["n_queries_run"]) == (1, 2) and s["nodes_visited"] < 14


def test_empty_calls():
    for args in ((0, [0], [], [], [0], []), (3, [0, 1, 1, 1], [2], [], [0], [])):
        hit, s = CY.cycle_reach(*args, all_queries=True, device=False)
        assert len(hit) == 0 and (s["first_hit"], s["n_queries_run"], s["nodes_visited"]) == (-1, 0, 0)


def bad_calls():
    """(name, the arguments of a call that breaks one clause of the contract)."""
    n, po, pr, qn, qo, qh = kat_arrays(KATS[5])

    def w(**kw):
        d = dict(n_nodes=n, pred_off=list(po), pred=list(pr), q_node=list(qn), q_head_off=list(qo), q_heads=list(qh))
        d.update(kw)
        return tuple(d[k] for k in ("n_nodes", "pred_off", "pred", "q_node", "q_head_off", "q_heads"))

    return [("pred_off decreases", w(pred_off=[0, 2, 1, 3, 4, 4])),
            ("pred_off ends short", w(pred_off=[0, 1, 2, 3, 3, 3])),
            ("pred_off starts above 0", w(pred_off=[1, 1, 2, 3, 4, 4])),
            ("q_head_off decreases", w(q_head_off=[0, 1, 0, 2, 3])),
            ("q_head_off ends past", w(q_head_off=[0, 0, 1, 2, 4])),
            ("a predecessor out of range", w(pred=[1, 2, 5, 4])),
            ("a negative predecessor", w(pred=[1, -1, 3, 4])),
            ("a source out of range", w(q_node=[0, 1, 2, 5])),
            ("q_node not ascending", w(q_node=[0, 2, 1, 3])),
            ("q_node repeats", w(q_node=[0, 1, 1, 3])),
            ("a head out of range", w(q_heads=[4, 0, 5])),
            ("a head that is its source", w(q_heads=[1, 0, 4])),
            ("negative n_nodes", w(n_nodes=-1))]


@pytest.mark.parametrize("name,args", bad_calls(), ids=[b[0] for b in bad_calls()])
def test_einval_writes_nothing(name, args):
    for all_queries in (True, False):
        call = abi._ReachCall(*args, all_queries)
        call.summary.first_hit = -77
        assert abi.lib().lc_cycle_reach_host(*call.args()) == -errno.EINVAL, name
        assert (call.hit == -7).all() and call.summary.first_hit == -77, name


def test_null_hit_and_unknown_flags():
    args = list(abi._ReachCall(*kat_arrays(KATS[0]), True).args())
    assert abi.lib().lc_cycle_reach_host(*args[:10], None, None) == -errno.EINVAL  # LC_REACH_ALL without hit
    assert abi.lib().lc_cycle_reach_host(*args[:9], 0, None, None) == 0            # neither hit nor summary
    assert abi.lib().lc_cycle_reach_host(*args[:9], 2, *args[10:]) == -errno.EINVAL


def test_limits(monkeypatch):
    monkeypatch.delenv("LC_CYCLE_MIN_WORK", raising=False)
    lim = CY.limits()
    assert lim["max_nodes"] == 262144 and lim["max_workgroups"] == 512 and lim["min_work"] == lim["default_min_work"]
    assert lim["default_min_work"] & (lim["default_min_work"] - 1) == 0
    for text, want in (("0", 0), ("12345", 12345), ("-3", lim["default_min_work"]), ("x", lim["default_min_work"])):
        monkeypatch.setenv("LC_CYCLE_MIN_WORK", text)
        assert CY.limits()["min_work"] == want, text


# ---- cycles_host_marked against cycles_host ----

CYCLE_FIELDS = ("scc", "scc_class", "steps", "cycle_off", "cycle_scc")


def same_cycles(want, got, what):
    n = len(want["cycle_scc"])  # (the checkers' bindings cut these to the cycles returned)
    for f in CYCLE_FIELDS:
        g = got[f][:n + 1] if f == "cycle_off" else got[f][:n] if f == "cycle_scc" else got[f]
        assert len(g) == len(want[f]) and (g == want[f]).all(), (what, f)
    assert (got["cycle_scc"][n:] == -1).all() and (got["cycle_off"][n:] == len(want["steps"])).all(), what


def marked_agrees(txns, out, s, what, stats):
    """lc_cycles_host over marks of three kinds against the checker's own rule
    7 (cycles_host): the screen's, every txn, a random superset of the SCCs."""
    edges = out["edges"]
    whole, _ = abi.cycles_host(txns, edges)
    same_cycles(out, whole, (what, "whole"))
    assert whole["n_class"].tolist() == s["n_class"] and whole["n_scc"] == s["n_scc"]
    arrays, scr = abi.cycle_screen_host(txns, edges)
    assert scr["clean"] in (0, 1)
    rng = np.random.default_rng(len(txns))
    marks = [("screen", arrays["mark"]), ("all", np.ones(len(txns), np.int32)),
             ("superset", ((out["scc"] >= 0) | (rng.random(len(txns)) < 0.3)).astype(np.int32))]
    for name, mark in marks:
        asked = []

        def oracle(*args):
            asked.append(len(args[3]))
            return REF.first_hit(*args)

        for hook_name, hook in (("host loop", None), ("oracle", oracle)):
            got, srch = abi.cycles_host(txns, edges, mark, hook, min_work=0)
            same_cycles(out, got, (what, name, hook_name))
            assert got["n_class"].tolist() == s["n_class"] and got["n_scc"] == s["n_scc"], (what, name, hook_name)
            assert srch["restricted"] == 1 and srch["n_marked"] == int(((mark != 0) & (txns["type"] != 2)).sum())
            assert (srch["n_device_searches"], srch["n_device_queries"]) == \
                ((len(asked), sum(asked)) if hook else (0, 0)), (what, name, hook_name)
        stats["searches"] += len(asked)
        stats["histories"] += 1
        stats["with_scc"] += s["n_scc"] > 0
    # below min_work the hook is not asked: the host loop, and no fallback counted
    got, srch = abi.cycles_host(txns, edges, marks[0][1], lambda *a: 1 / 0, min_work=1 << 62)
    same_cycles(out, got, (what, "min_work"))
    assert (srch["n_device_searches"], srch["n_host_fallbacks"]) == (0, 0)
    # the two fallbacks: a hook that refuses every search (what -E2BIG from the device is), and an SCC
    # above max_nodes, which the hook is not asked about; each counted once per search, the outputs the same
    refused = []
    got, srch = abi.cycles_host(txns, edges, marks[0][1], lambda *a: refused.append(a[0]), min_work=0)
    same_cycles(out, got, (what, "refused"))
    assert (srch["n_device_searches"], srch["n_device_queries"], srch["n_host_fallbacks"]) == (0, 0, len(refused))
    got, srch = abi.cycles_host(txns, edges, marks[0][1], lambda *a: 1 / 0, min_work=0, max_nodes=1)
    same_cycles(out, got, (what, "max_nodes"))
    assert (srch["n_device_searches"], srch["n_host_fallbacks"]) == (0, len(refused))  # (every SCC has 2 members at least)
    big = max(refused, default=0)
    if big > 2:  # at the edge: an SCC of exactly max_nodes members is asked, one member more is not
        asked = []
        got, srch = abi.cycles_host(txns, edges, marks[0][1], lambda *a: asked.append(a[0]) or REF.first_hit(*a),
                                    min_work=0, max_nodes=big - 1)
        same_cycles(out, got, (what, "max_nodes edge"))
        assert max(asked, default=0) <= big - 1 and srch["n_host_fallbacks"] == sum(n >= big for n in refused)
        assert srch["n_device_searches"] == len(asked) == len(refused) - srch["n_host_fallbacks"]
    stats["fallbacks"] = stats.get("fallbacks", 0) + len(refused)


def test_marked_pass_on_the_append_kats_and_random_histories():
    stats = {"searches": 0, "histories": 0, "with_scc": 0}
    for kat in AP_KATS:
        enc = AP.encode(kat["history"])
        marked_agrees(enc.txns, *abi.append_check_host(enc.txns, enc.mops, enc.values), kat["name"], stats)
    for i in range(N_BULK):
        enc = AP.encode(AC.random_history(20000 + i, n_txns=5 + (i * 37) % 296, faults=AC.FAULTS + AC.SCRIPTED,
                                          p_fault=0.1, sliding=True))
        marked_agrees(enc.txns, *abi.append_check_host(enc.txns, enc.mops, enc.values), i, stats)
    assert stats["with_scc"] >= 60 and stats["searches"] >= 20 and stats["fallbacks"] >= 5, stats


@pytest.mark.parametrize("wfr", (True, False), ids=("wfr", "no-wfr"))
def test_marked_pass_on_the_wr_kats_and_random_histories(wfr):
    stats = {"searches": 0, "histories": 0, "with_scc": 0}
    for kat in WR_KATS:
        enc = WR.encode(kat["history"])
        marked_agrees(enc.txns, *abi.wr_check_host(enc.txns, enc.mops, wfr), kat["name"], stats)
    for i in range(0, N_BULK, 1 if wfr else 3):
        enc = WR.encode(WC.random_history(20000 + i, n_txns=5 + (i * 37) % 296, faults=WC.FAULTS + WC.SCRIPTED,
                                          p_fault=0.1, sliding=True))
        marked_agrees(enc.txns, *abi.wr_check_host(enc.txns, enc.mops, wfr), i, stats)
    assert stats["with_scc"] >= 20 and stats["searches"] >= 5 and stats["fallbacks"] >= 2, stats


@pytest.mark.parametrize("conc", PC.CONCS)
@pytest.mark.parametrize("back", PC.BACKS)
def test_marked_pass_on_the_planted_stale_reads(back, conc):
    """One SCC of class G-single-realtime (6) in every case."""
    for name, (txns, out, s) in (("append", (lambda a: (a[0],) + abi.append_check_host(*a))(PC.append_plant(back, conc))),
                                 ("wr", (lambda a: (a[0],) + abi.wr_check_host(*a))(PC.wr_plant(back, conc)))):
        stats = {"searches": 0, "histories": 0, "with_scc": 0}
        marked_agrees(txns, out, s, (name, back, conc), stats)
        assert s["n_scc"] == 1 and s["n_class"][6] == 1 and len(out["steps"]) >= 2, (name, s)
        assert stats["searches"] >= 3  # (the three marks each asked k = 6 at least)
