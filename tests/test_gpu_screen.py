"""lc_cycle_screen on the GPU against lc_cycle_screen_host: every output array,
every count and both round counts equal, at the smallest shapes where the
kernels can go wrong: txn and edge counts round the wave, the block and the
scans' tiles, FAIL txns at the scans' edges, chains that take one round per hop
round the batch of rounds and the give-up edge, same-address atomics, the
extreme positions, the trim's chains, every error, workspace reuse, and in
bulk."""
import errno

import numpy as np
import pytest

import append_cases as AC
import screen_ref as REF
import wr_cases as WC
from jepsen.etcd_amd import abi, append as AP, screen as SC, wr as WR
from test_screen import (AP_KATS, COUNTS, EINVAL_CASES, GOOD, KATS, KINDS, WR_KATS, MarkedCall, _bad, against_order,
                         arrays, composed_history)

pytestmark = pytest.mark.gpu

OK, INFO, FAIL = abi.LC_AP_OK, abi.LC_AP_INFO, abi.LC_AP_FAIL
NAMES = {OK: "ok", INFO: "info", FAIL: "fail"}


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


@pytest.fixture
def many_rounds(monkeypatch):
    """Room for the chains that take more rounds than the default allows."""
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "256")


def _agree(ctx, txns, edges, what=""):
    want, ws = abi.cycle_screen_host(txns, edges)
    got, gs = ctx.cycle_screen(txns, edges)
    for f in want:
        assert want[f].shape == got[f].shape, (what, f)
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), want[f][bad[:3]].tolist(), got[f][bad[:3]].tolist())
    assert [gs[k] for k in COUNTS] == [ws[k] for k in COUNTS], (what, gs, ws)
    return got, gs


def graph(n, n_edges, seed, width=6, p_info=0.1, p_fail=0.1, types=None, p_back=0.2):
    """n txns whose lifetimes span up to `width` later invokes, positions
    distinct; n_edges distinct edges between nodes at most 2 * width apart,
    p_back of them against txn order."""
    rng = np.random.default_rng(seed)
    typ = rng.choice([OK, INFO, FAIL], size=n, p=[1 - p_info - p_fail, p_info, p_fail]) if types is None \
        else np.asarray(types)
    when = np.concatenate([np.arange(n, dtype=np.float64),
                           np.arange(n) + rng.integers(0, width + 1, size=n) + 0.25 + 0.5 * rng.random(n)])
    pos = np.empty(2 * n, dtype=np.int64)
    pos[np.argsort(when, kind="stable")] = np.arange(2 * n)
    txns = np.zeros(n, dtype=abi.AP_TXN_DTYPE)
    txns["inv_pos"], txns["comp_pos"], txns["type"] = pos[:n], np.where(typ == INFO, -1, pos[n:]), typ
    nodes = np.nonzero(typ != FAIL)[0]
    rows = set()
    if len(nodes) >= 2:
        while len(rows) < n_edges:
            i = int(rng.integers(0, len(nodes)))
            j = i + int(rng.integers(1, 2 * width + 1))
            if j >= len(nodes):
                i, j = len(nodes) - 2, len(nodes) - 1
            a, b = int(nodes[i]), int(nodes[j])
            if rng.random() < p_back:
                a, b = b, a
            rows.add((a, b, int(rng.integers(0, 3)), int(rng.integers(0, 1 << 40))))
    edges = np.array(sorted(rows), dtype=np.int64).reshape(-1, 4)
    e = np.zeros(len(edges), dtype=abi.AP_EDGE_DTYPE)
    e["from"], e["to"], e["type"], e["key"] = edges[:, 0], edges[:, 1], edges[:, 2], edges[:, 3]
    return txns, e


def overlapping(n, edges):
    """n OK txns all invoked before any completes."""
    return arrays([("ok", i, n + i) for i in range(n)], edges)


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(ctx, kat):
    got, gs = _agree(ctx, *arrays(kat["txns"], kat["edges"]), what=kat["name"])
    assert got["mark"].tolist() == kat["mark"] and gs["clean"] == kat["clean"]


@pytest.mark.parametrize("n_txns", (1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097))
def test_txn_and_edge_counts(ctx, n_txns):
    for n_edges in (0, 1, 64, 65):
        if n_edges and n_txns < 2:
            continue
        for p_back in (0.0, 0.3):
            txns, edges = graph(n_txns, n_edges, 1000 * n_txns + n_edges, p_info=0.05, p_fail=0.0, p_back=p_back)
            _agree(ctx, txns, edges, (n_txns, n_edges, p_back))


def test_all_info_and_all_fail_but_one(ctx):
    for n in (1, 64, 300):
        _agree(ctx, *graph(n, min(n - 1, 40), n, types=[INFO] * n), what=("info", n))
        for keep in (0, n // 2, n - 1):
            types = [FAIL] * n
            types[keep] = OK
            got, gs = _agree(ctx, *graph(n, 0, n, types=types), what=("fail", n, keep))
            assert gs["clean"] == 1 and (got["reach_hi"] >= 0).sum() == 1


@pytest.mark.parametrize("where", (0, 255, 256, 257, 512))
def test_a_fail_txn_at_an_edge_enters_no_scan(ctx, where):
    """A FAIL txn at the first index, the last and round a block edge keeps the
    scans' identities; taken for an OK txn it would have moved a label of its
    neighbours (the host function says so)."""
    n = 513
    types = [OK] * n
    types[where] = FAIL
    txns, edges = graph(n, 64, where, width=4, types=types, p_back=0.0)
    got, gs = _agree(ctx, txns, edges, where)
    assert got["reach_lo"][where] == 2 ** 31 - 1 and got["reach_hi"][where] == -1 and got["mark"][where] == 0
    as_ok = txns.copy()
    as_ok["type"][where] = OK
    other, _ = abi.cycle_screen_host(as_ok, edges)
    assert where in (0, n - 1) or (other["reach_hi"] != got["reach_hi"]).any() or \
        (other["reach_lo"] != got["reach_lo"]).any()


@pytest.mark.parametrize("hops", (1, 2, 3, 4, 5, 63, 64, 65))
def test_chains_against_txn_order_take_a_round_per_hop(ctx, many_rounds, hops):
    got, gs = _agree(ctx, *against_order(hops), what=hops)
    assert (gs["clean"], gs["label_rounds"], gs["trim_rounds"]) == (1, hops + 1, (hops + 2) // 2 + 1)
    assert (got["reach_hi"] == hops).all()


@pytest.mark.parametrize("hops", (6, 7, 8, 9))
def test_the_give_up_edge(ctx, monkeypatch, hops):
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", "8")
    got, gs = _agree(ctx, *against_order(hops), what=hops)
    assert (gs["clean"], gs["label_rounds"], gs["max_rounds"]) == ((1, hops + 1, 8) if hops < 8 else (-1, 8, 8))
    # the trim's give-up edge: an in-class chain of 2 r - 1 or 2 r nodes takes r + 1 rounds
    n = 2 * hops
    txns, edges = overlapping(n, [(i + 1, i, 0, 1) for i in range(n - 1)])
    monkeypatch.setenv("LC_SCREEN_MAX_ROUNDS", str(n))  # (the labels take n rounds)
    _, gs = _agree(ctx, txns, edges, what=("trim", hops))
    assert (gs["clean"], gs["trim_rounds"]) == (1, hops + 1)
    txns, edges = overlapping(n, [(i + 1, i, 0, 1) for i in range(n - 1)] + [(0, 1, 0, 2), (n - 2, n - 1, 0, 2)])
    _, gs = _agree(ctx, txns, edges, what=("kept", hops))
    assert (gs["clean"], gs["trim_rounds"], gs["n_trim_survivors"]) == (0, 1, n)


def test_a_forward_chain_takes_one_round(ctx):
    n = 4096
    txns, edges = arrays([("ok", 2 * i, 2 * i + 1) for i in range(n)], [(i, i + 1, 1, 7) for i in range(n - 1)])
    _, gs = _agree(ctx, txns, edges)
    assert (gs["clean"], gs["label_rounds"], gs["trim_rounds"]) == (1, 1, 2)
    txns, edges = arrays([("info", i, None) for i in range(n)], [(i, i + 1, 0, 7) for i in range(n - 1)])
    _, gs = _agree(ctx, txns, edges)
    assert (gs["clean"], gs["label_rounds"], gs["trim_rounds"]) == (1, 1, 2)


def test_a_hub_takes_same_address_atomics(ctx):
    """300 later txns -> the hub -> 300 earlier ones, all overlapping: every
    in-edge raises the hub's K and every out-edge lowers its H, in one round."""
    n, hub = 601, 300
    rows = [(u, hub, 0, u) for u in range(hub + 1, n)] + [(hub, v, 1, v) for v in range(hub)]
    got, gs = _agree(ctx, *overlapping(n, rows))
    assert got["reach_hi"][hub] == n - 1 and got["reach_lo"][hub] == n and gs["clean"] == 1
    # the same txns one after the other: one SCC with real time inside
    txns, edges = arrays([("ok", 2 * i, 2 * i + 1) for i in range(n)], rows)
    got, gs = _agree(ctx, txns, edges)
    assert gs["clean"] == 0 and gs["n_rt_members"] == n


def test_extreme_positions(ctx):
    top = 2 ** 31 - 2
    for txns, rows in (([("ok", 0, top)], []),
                       ([("ok", 0, 1), ("ok", top - 1, top)], [(1, 0, 1, 5)]),
                       ([("ok", 0, top), ("info", top - 1, None)], [(1, 0, 0, 5), (0, 1, 0, 5)]),
                       ([("info", 0, None), ("ok", 1, 2), ("info", top, None)], [(2, 0, 0, 5)])):
        _agree(ctx, *arrays(txns, rows), what=txns)


@pytest.mark.parametrize("n", (1, 2, 64, 65))
def test_the_trim_empties_an_acyclic_chain(ctx, many_rounds, n):
    txns, edges = overlapping(n, [(i + 1, i, 0, 1) for i in range(n - 1)])
    got, gs = _agree(ctx, txns, edges, n)
    assert (gs["clean"], gs["trim_rounds"]) == (1, (n + 1) // 2 + 1)
    assert len(set(zip(got["reach_lo"].tolist(), got["reach_hi"].tolist()))) == 1  # one class


def test_the_trim_keeps_a_cycle_and_drops_its_tail(ctx, many_rounds):
    n = 66  # a 2-cycle of txns 0 and 1, and 64 txns in its class that lead into it
    txns, edges = overlapping(n, [(i + 1, i, 0, 1) for i in range(n - 1)] + [(0, 1, 0, 2)])
    got, gs = _agree(ctx, txns, edges)
    assert got["mark"].tolist() == [2, 2] + [0] * 64 and (gs["clean"], gs["trim_rounds"]) == (0, 65)


def test_workspace_reuse_with_sizes_flipped():
    big, small = graph(5000, 9000, 1), graph(40, 60, 2)
    for order in ((big, small, big), (small, big, small)):
        with abi.Context(device_mask=1) as c:
            for txns, edges in order:
                _agree(c, txns, edges, len(txns))


@pytest.mark.parametrize("what", EINVAL_CASES)
def test_a_good_call_after_every_error(ctx, what):
    call = MarkedCall(*_bad(what))
    assert call.run(ctx) == -errno.EINVAL and call.untouched()
    assert "lc_cycle_screen" in ctx.last_error()
    _agree(ctx, *arrays(*GOOD))


def test_no_txns(ctx):
    got, gs = _agree(ctx, np.zeros(0, dtype=abi.AP_TXN_DTYPE), np.zeros(0, dtype=abi.AP_EDGE_DTYPE))
    assert gs["clean"] == 1 and gs["label_rounds"] == 0


def _as_ref(txns, edges):
    return ([{"type": NAMES[int(t["type"])], "inv": int(t["inv_pos"]), "comp": int(t["comp_pos"])} for t in txns],
            {(int(e["from"]), int(e["to"]), int(e["type"]), int(e["key"])) for e in edges})


def test_random_histories(ctx):
    """300 histories of up to 300 txns through the checkers' host functions,
    their graphs through both screens; the kinds counted by screen_ref."""
    rng = np.random.default_rng(7)
    seen = dict.fromkeys(KINDS, 0)
    for seed in range(300):
        if seed % 3 == 0:
            enc = WR.encode(composed_history(seed)) if seed < 120 else \
                WR.encode(WC.random_history(seed, n_txns=int(rng.integers(1, 301)), n_keys=4, conc=6))
            out, _ = abi.wr_check_host(enc.txns, enc.mops)
        elif seed % 3 == 1:
            enc = WR.encode(WC.random_history(seed, n_txns=int(rng.integers(1, 40)), conc=12,
                                              faults=("stale", "split", "double", "g0")))
            out, _ = abi.wr_check_host(enc.txns, enc.mops)
        else:
            big = seed % 2 == 0
            enc = AP.encode(AC.random_history(seed, n_txns=int(rng.integers(1, 301 if big else 40)),
                                              n_keys=4 if big else 3, conc=6 if big else 4))
            out, _ = abi.append_check_host(enc.txns, enc.mops, enc.values)
        _agree(ctx, enc.txns, out["edges"], seed)
        for kind, is_one in REF.category(REF.screen(*_as_ref(enc.txns, out["edges"]))).items():
            seen[kind] += is_one
    assert all(seen[k] >= 20 for k in KINDS), seen


def test_checker_kat_graphs(ctx):
    for kat in AP_KATS:
        enc = AP.encode(kat["history"])
        out, _ = abi.append_check_host(enc.txns, enc.mops, enc.values)
        _agree(ctx, enc.txns, out["edges"], kat["name"])
    for kat in WR_KATS:
        enc = WR.encode(kat["history"])
        out, _ = abi.wr_check_host(enc.txns, enc.mops)
        _agree(ctx, enc.txns, out["edges"], kat["name"])


def test_twenty_thousand_txns(ctx):
    txns, edges = graph(20000, 40000, 5, width=8, p_back=0.0, p_fail=0.05)
    _, gs = _agree(ctx, txns, edges, "forward")
    assert gs["clean"] == 1  # (no edge against txn order: no cycle)
    txns, edges = graph(20000, 40000, 6, width=8, p_back=0.02, p_fail=0.05)
    _, gs = _agree(ctx, txns, edges, "some back")
    assert gs["clean"] == 0


def test_the_module(ctx):
    txns, edges = arrays(*GOOD)
    want, ws = SC.cycle_screen(txns, edges, device=False)
    for got, gs in (SC.cycle_screen(txns, edges, ctx=ctx), SC.cycle_screen(txns, edges)):
        assert all((want[f] == got[f]).all() for f in want) and [gs[k] for k in COUNTS] == [ws[k] for k in COUNTS]
    assert SC.available()
