"""lc_wr_check_lin on the GPU against lc_wr_check_lin_host under all four flag
combinations: every output array, the lc_wr_lin_key records and every count of
both summaries equal, on the hand-derived histories and at the smallest shapes
where each kernel can go wrong: touch segments round the wave and the
workgroup, successor runs round the wave and the item chunk, one version edge
from many pairs, closures in a wavefront (2 .. 64 versions) and in a workgroup
(65 .. max_key_versions), ww / rw products round the wave, every error,
workspace reuse, and in bulk."""
import errno

import numpy as np
import pytest

import wr_cases as C
import wr_lin_ref as REF
from jepsen.etcd_amd import abi, wr as WR
from test_gpu_wr import COUNTS, INFO, FAIL, NIL, OK, build, overlapping, serial
from test_wr_lin import COMBOS, COMBO_IDS, KATS, MarkedLinCall, certify_version_cycles, same_outputs, strip

pytestmark = pytest.mark.gpu

LIN_COUNTS = ("n_touches", "n_pairs", "n_vedges", "max_key_versions")
MAX_V = 512      # lc_wr_lin_limits' max_key_versions
ITEM_CHUNK = 4096  # txngraph.h, kItemChunk
WW, WR_, RW = abi.LC_AP_WW, abi.LC_AP_WR, abi.LC_AP_RW


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def _agree(ctx, txns, mops, wfr=True, lin=True, what=""):
    want, ws, wl = abi.wr_check_lin_host(txns, mops, wfr, lin)
    got, gs, gl = ctx.wr_check_lin(txns, mops, wfr, lin)
    for f in want:
        assert want[f].shape == got[f].shape, (what, f, want[f].shape, got[f].shape)
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), want[f][bad[:3]].tolist(), got[f][bad[:3]].tolist())
    assert [gs[k] for k in COUNTS] == [ws[k] for k in COUNTS], (what, gs, ws)
    assert [gl[k] for k in LIN_COUNTS] == [wl[k] for k in LIN_COUNTS], (what, gl, wl)
    return got, gs, gl


def _agree_all(ctx, txns, mops, what=""):
    """All four combinations; -> the (wfr, lin) result."""
    for wfr, lin in COMBOS:
        r = _agree(ctx, txns, mops, wfr, lin, (what, wfr, lin))
    return r


def at(inv, comp, ms, typ=OK):
    return (typ, inv, -1 if typ == INFO else comp, ms)


def info_writers(key, values, pos=0):
    """INFO txns (never in K) that write the values, invoked from pos on."""
    return [at(pos + i, -1, [("w", key, v)], INFO) for i, v in enumerate(values)]


# ---------------------------------------------------------------- the hand-derived histories

@pytest.mark.parametrize("combo", range(4), ids=COMBO_IDS)
@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(ctx, kat, combo):
    wfr, lin = COMBOS[combo]
    enc = WR.encode(kat["history"])
    got, gs, gl = _agree(ctx, enc.txns, enc.mops, wfr, lin, kat["name"])
    assert {1: True, 0: False, -1: "unknown"}[gs["valid"]] == kat["expect"][COMBO_IDS[combo]]["valid"]


# ---------------------------------------------------------------- touch segments and the sort

@pytest.mark.parametrize("n", (1, 2, 63, 64, 65, 255, 256, 257))
def test_touches_of_one_key(ctx, n):
    """One write and n - 1 reads of it: n touches, one after the other (a
    chain of n - 1 pairs) and all together (none)."""
    txs = [[("w", 1, 1)]] + [[("r", 1, 1)] for _ in range(n - 1)]
    got, gs, gl = _agree_all(ctx, *serial(txs), what=("serial", n))
    assert (gl["n_touches"], gl["n_pairs"], gs["valid"]) == (n, n - 1, 1)
    got, gs, gl = _agree_all(ctx, *overlapping(txs), what=("overlapping", n))
    assert (gl["n_touches"], gl["n_pairs"], gs["valid"]) == (n, 0, 1)


@pytest.mark.parametrize("n_keys", (1, 2, 65))
def test_touches_over_keys(ctx, n_keys):
    """130 txns over n_keys keys in turn, each writing its key: every key's
    touches are a segment of their own, chained."""
    txs = [[("w", i % n_keys, i + 1)] for i in range(130)]
    got, gs, gl = _agree_all(ctx, *serial(txs), what=n_keys)
    assert gl["n_touches"] == 130 and gl["n_pairs"] == 130 - n_keys and gs["valid"] == 1
    assert got["lin_keys"]["n_touches"].tolist() == [130 // n_keys] * n_keys


def test_a_txn_touching_four_keys_and_other_txn_types_between(ctx):
    four = [("w", 1, 1), ("r", 2, NIL), ("w", 3, 3), ("r", 4, NIL), ("r", 1, 1), ("w", 3, 4)]
    txs = [four, [("w", 2, 20)], [("r", 1, None), ("w", 4, 40)], [("r", 3, 4), ("r", 2, 20)], [("w", 1, 5)],
           [("r", 4, 41), ("r", 1, 1)]]
    types = {1: INFO, 2: FAIL, 4: FAIL}
    got, gs, gl = _agree_all(ctx, *serial(txs, types), what="four keys")
    assert got["lin_keys"]["n_touches"].tolist() == [2, 2, 2, 2]  # OK txns only: txns 0, 3 and 5


def test_positions_at_both_ends(ctx):
    txns, mops = build([at(0, 5, [("w", 1, 1)]), at(6, 2 ** 31 - 2, [("r", 1, 1)])])
    got, gs, gl = _agree_all(ctx, txns, mops, what="positions")
    assert gl["n_pairs"] == 1 and gs["valid"] == 1
    txns, mops = build([at(0, 2 ** 31 - 2, [("w", 1, 1)]), at(6, 7, [("r", 1, 1)])])
    got, gs, gl = _agree_all(ctx, txns, mops, what="positions, nested")
    assert gl["n_pairs"] == 0


# ---------------------------------------------------------------- ranges and pair items

@pytest.mark.parametrize("n", (1, 63, 64, 65, 300))
def test_one_txn_and_its_concurrent_successors(ctx, n):
    specs = [at(0, 1, [("w", 1, 1)])] + [at(2 + i, 2 + n + i, [("r", 1, 1)]) for i in range(n)]
    got, gs, gl = _agree_all(ctx, *build(specs), what=n)
    assert gl["n_pairs"] == n and gs["valid"] == 1


def test_pairs_across_the_item_chunk(ctx):
    """70 concurrent txns, then 70 more: 4,900 pairs, across kItemChunk; each
    first txn wrote a value of its own, each second one reads value 1."""
    specs = [at(i, 100 + i, [("w", 1, i + 1)]) for i in range(70)]
    specs += [at(200 + i, 300 + i, [("r", 1, 1)]) for i in range(70)]
    assert 70 * 70 > ITEM_CHUNK
    got, gs, gl = _agree_all(ctx, *build(specs), what="70 x 70")
    assert gl["n_pairs"] == 4900 and got["lin_keys"]["n_vedges"].tolist() == [70 + 69]  # nil -> i, i -> 1 (not 1 -> 1)


@pytest.mark.parametrize("bound", (0, 2, 4))
def test_the_successor_that_bounds_the_run(ctx, bound):
    """Five successors invoked at 10 .. 14; the one at `bound` completes at 15,
    before a sixth txn is invoked at 16: that one is no successor of txn 0."""
    specs = [at(0, 1, [("w", 1, 1)])]
    specs += [at(10 + i, 15 if i == bound else 20 + i, [("r", 1, 1)]) for i in range(5)]
    specs += [at(16, 17, [("r", 1, 1)])]
    got, gs, gl = _agree_all(ctx, *build(specs), what=bound)
    assert gl["n_pairs"] == 5 + 1  # txn 0's five, and (the bounding one, the sixth)


# ---------------------------------------------------------------- set semantics

def test_one_version_edge_from_many_pairs(ctx):
    """65 concurrent readers of 1, then a reader of 2: 65 pairs, all of them
    1 -> 2.  The key has nil -> 1, nil -> 2 and 1 -> 2, and version 1 one
    child: 65 rw edges (each reader to the writer of 2), not 65 x 65."""
    specs = info_writers(1, (1, 2)) + [at(10 + i, 100 + i, [("r", 1, 1)]) for i in range(65)]
    specs += [at(200, 201, [("r", 1, 2)])]
    got, gs, gl = _agree_all(ctx, *build(specs), what="65 pairs")
    assert gl["n_pairs"] == 65 and got["lin_keys"]["n_vedges"].tolist() == [3]
    assert int((got["edges"]["type"] == RW).sum()) == 65 and gs["n_edges_raw"] == 65 + 1 + 65 + 1  # rw, ww, wr


# ---------------------------------------------------------------- the closure, a wavefront per key

def blind_chain(n, key=1, base=0):
    return [[("w", key, base + i + 1)] for i in range(n)]


@pytest.mark.parametrize("n", (2, 3, 63, 64))
def test_wave_chains_and_cycles(ctx, n):
    """n blind writes one after the other: a chain of n versions; one stale
    read of the first closes it into a cycle over all of them."""
    got, gs, gl = _agree_all(ctx, *serial(blind_chain(n)), what=("chain", n))
    assert (gs["valid"], gs["n_cyclic_keys"], gl["max_key_versions"]) == (1, 0, n)
    assert int((got["edges"]["type"] == WW).sum()) == n - 1 and got["lin_keys"]["n_vedges"].tolist() == [2 * n - 1]
    got, gs, gl = _agree_all(ctx, *serial(blind_chain(n, base=9) + [[("r", 1, 10)]]), what=("cycle", n))
    assert (gs["valid"], gs["n_cyclic_keys"]) == (0, 1) and got["keys"]["cyc_value"].tolist() == [10]
    assert not (got["edges"]["type"] != WR_).any()  # a cyclic key keeps its wr edges alone


def test_wave_cycle_through_nil_and_negative_values(ctx):
    got, gs, gl = _agree_all(ctx, *serial([[("w", 1, 7)], [("r", 1, NIL)]]), what="nil")
    assert got["keys"]["cyc_value"].tolist() == [7] and got["lin_keys"]["n_vedges"].tolist() == [2]
    got, gs, gl = _agree_all(ctx, *serial([[("w", 1, 3)], [("w", 1, -5)], [("r", 1, 3)]]), what="negative")
    assert got["keys"]["cyc_value"].tolist() == [-5]
    got, gs, gl = _agree_all(ctx, *serial([[("w", 1, 2 ** 63 - 1)], [("w", 1, -2 ** 63 + 1)], [("r", 1, 2 ** 63 - 1)]]),
                             what="extremes")
    assert got["keys"]["cyc_value"].tolist() == [-2 ** 63 + 1]


def test_wave_self_loop_with_lin_edges_round_it(ctx):
    """Txn 1 reads 5 and writes 5 (a wfr self-loop, whatever wrote the first 5:
    nobody else may, so it is its own writer); lin edges lead to it and on."""
    txs = [[("w", 1, 1)], [("r", 1, 5), ("w", 1, 5)], [("w", 1, 9)], [("r", 1, 9)]]
    got, gs, gl = _agree_all(ctx, *serial(txs), what="self-loop")
    assert got["keys"]["cyc_value"].tolist() == [5] and gs["n_cyclic_keys"] == 1
    got, gs, gl = _agree(ctx, *serial(txs), False, True, "self-loop, no wfr")
    assert gs["n_cyclic_keys"] == 0


def test_wave_tail_below_a_cycle(ctx):
    """1000 <-> 1001 by a stale read, then 60 smaller values written one after
    the other: below the cycle, not on it; 62 versions."""
    txs = [[("w", 1, 1000)], [("w", 1, 1001)], [("r", 1, 1000)]] + blind_chain(60)
    got, gs, gl = _agree_all(ctx, *serial(txs), what="tail")
    assert got["keys"]["cyc_value"].tolist() == [1000] and gl["max_key_versions"] == 62


# ---------------------------------------------------------------- the closure, a workgroup per key

@pytest.mark.parametrize("n", (65, 66, MAX_V - 1, MAX_V))
def test_block_chains_and_cycles(ctx, n):
    got, gs, gl = _agree_all(ctx, *serial(blind_chain(n)), what=("chain", n))
    assert (gs["valid"], gs["n_cyclic_keys"], gl["max_key_versions"]) == (1, 0, n)
    assert int((got["edges"]["type"] == WW).sum()) == n - 1
    # the cycle over all of it: the last txn reads the first value; a small key beside it keeps its edges
    txs = blind_chain(n, base=9) + [[("w", 2, 1)], [("w", 2, 2)], [("r", 1, 10)]]
    got, gs, gl = _agree_all(ctx, *serial(txs), what=("cycle", n))
    assert got["keys"]["cyc_value"].tolist() == [10, NIL] and gl["max_key_versions"] == n
    assert {int(x["type"]) for x in got["edges"][got["edges"]["key"] == 2]} == {WW}


def test_above_max_key_versions_is_e2big_and_writes_nothing(ctx):
    assert abi.wr_lin_limits()["max_key_versions"] == MAX_V
    txns, mops = serial(blind_chain(MAX_V + 1))
    call = MarkedLinCall(txns, mops, 3)
    assert call.run(ctx) == -errno.E2BIG and call.untouched()
    assert str(MAX_V + 1) in ctx.last_error()
    _agree(ctx, txns, mops, True, False, "flag off above the limit")  # lc_wr_check has no such limit
    _agree_all(ctx, *serial(blind_chain(MAX_V)), what="a good call after")


# ---------------------------------------------------------------- rule 7''s edges

@pytest.mark.parametrize("r", (0, 1, 63, 64, 65))
@pytest.mark.parametrize("c", (0, 1, 63, 64, 65))
def test_reader_child_products(ctx, r, c):
    """Txn 0 writes 1; r txns read it together; then c txns write together,
    and c more read values nobody wrote: version 1 has r readers and a writer
    against 2 c children (r = 0: txn 0's pairs make the same edges), half of
    them heads without a writer."""
    specs = [at(0, 1, [("w", 1, 1)])] + [at(10 + i, 100 + i, [("r", 1, 1)]) for i in range(r)]
    specs += [at(200 + i, 400 + i, [("w", 1, 1000 + i)]) for i in range(c)]
    specs += [at(300 + i, 500 + i, [("r", 1, 2000 + i)]) for i in range(c)]
    got, gs, gl = _agree(ctx, *build(specs), True, True, what=(r, c))
    assert int((got["edges"]["type"] == RW).sum()) == r * c and int((got["edges"]["type"] == WW).sum()) == c
    assert gs["n_phantom"] == c and gl["n_pairs"] == r + max(r, 1) * 2 * c
    _agree(ctx, *build(specs), False, True, what=(r, c, "no wfr"))


def test_a_cyclic_key_beside_one_that_keeps_its_edges(ctx):
    txs = [[("w", 1, 1), ("w", 2, 21)], [("w", 1, 2), ("w", 2, 22)], [("r", 1, 1), ("r", 2, 22)]]
    got, gs, gl = _agree_all(ctx, *serial(txs), what="two keys")
    assert got["keys"]["flags"].tolist() == [abi.LC_WR_K_CYCLIC, 0]
    e = got["edges"]
    assert {int(x["type"]) for x in e[e["key"] == 1]} == {WR_} and {int(x["type"]) for x in e[e["key"] == 2]} == {WW, WR_}


def test_enospc_and_the_binding_s_retry(ctx):
    specs = [at(0, 1, [("w", 1, 1)])] + [at(10 + i, 100 + i, [("r", 1, 1)]) for i in range(65)]
    specs += [at(200 + i, 400 + i, [("w", 1, 1000 + i)]) for i in range(65)]
    txns, mops = build(specs)
    want, ws, _ = abi.wr_check_lin_host(txns, mops)
    assert ws["n_edges"] > 2 * len(mops) + 16  # the default room does not hold them: the binding comes again
    call = MarkedLinCall(txns, mops, 3)
    assert call.run(ctx) == -errno.ENOSPC and call.arrays_untouched()
    assert (call.summary.n_edges, call.summary.n_edges_raw) == (ws["n_edges"], ws["n_edges_raw"])
    assert call.lin_summary.n_touches == call.MARK
    _agree(ctx, txns, mops, what="retry")


# ---------------------------------------------------------------- reuse, errors, bulk

def composed_history(seed):
    """The rare kind, composed: a fault-free random history, and on a key of
    its own a stale read across two blind writes (w 1, w 2, r 1, one after the
    other), its six ops dropped among the others at random: valid under wfr
    alone wherever the host history is, cyclic with lin."""
    rng = np.random.default_rng(seed)
    h = C.random_history(seed, n_txns=int(rng.integers(4, 30)), faults=[])
    ops = []
    for p, mop in ((100, ["w", 777, 900001]), (101, ["w", 777, 900002]), (102, ["r", 777, 900001])):
        ops += [C.op("invoke", p, [[mop[0], mop[1], None if mop[0] == "r" else mop[2]]], 0), C.op("ok", p, [mop], 0)]
    for at_, o in zip(sorted(rng.integers(0, len(h) + 1, 6).tolist(), reverse=True), reversed(ops)):
        h.insert(at_, o)
    for i, o in enumerate(h):
        o["index"] = i
    return h


def sized_history(seed):
    """A random history of 4 .. 300 txns, most of them small; every tenth is composed_history's."""
    if seed % 10 == 9:
        return composed_history(seed)
    rng = np.random.default_rng(seed)
    n = int(rng.choice((4, 8, 12, 20, 40, 100, 300), p=(0.2, 0.25, 0.2, 0.15, 0.1, 0.05, 0.05)))
    return C.random_history(seed, n_txns=n, n_keys=int(rng.integers(1, 5)), conc=int(rng.integers(2, 8)))


def test_workspace_reuse_with_the_sizes_flipped():
    big, small = serial(blind_chain(300) + [[("r", 1, 1)]]), serial(blind_chain(3) + [[("r", 1, 1)]])
    for order in ((big, small, big), (small, big, small)):
        with abi.Context(device_mask=1) as c:
            for txns, mops in order:
                _agree(c, txns, mops, what="reuse")
                _agree(c, txns, mops, True, False, what="reuse, flag off")


def test_a_good_call_after_every_error(ctx):
    good = serial(blind_chain(5) + [[("r", 1, 2)]])
    enc = WR.encode(C.sequential(4))
    two = enc.mops.copy()
    two["value"][3] = 1
    errors = [(MarkedLinCall(enc.txns, enc.mops, 4), errno.EINVAL), (MarkedLinCall(enc.txns, enc.mops, 8), errno.EINVAL),
              (MarkedLinCall(enc.txns, two, 3), errno.EINVAL),
              (MarkedLinCall(*serial(blind_chain(MAX_V + 1)), 2), errno.E2BIG),
              (MarkedLinCall(*good, 3, edge_cap=0), errno.ENOSPC)]
    for call, code in errors:
        assert call.run(ctx) == -code and call.arrays_untouched(), code
        assert code == errno.ENOSPC or call.untouched()
        _agree_all(ctx, *good, what=("after", code))


def test_flag_off_equals_lc_wr_check(ctx):
    for seed in range(20):
        enc = WR.encode(sized_history(seed))
        for wfr in (True, False):
            out, s, ls = ctx.wr_check_lin(enc.txns, enc.mops, wfr, False)
            out0, s0 = ctx.wr_check(enc.txns, enc.mops, wfr)
            same_outputs(out, s, out0, s0)
            assert not out["lin_keys"].view(np.int8).any() and not any(ls.values())


def test_random_histories_in_bulk(ctx):
    """300 random histories of up to 300 txns under all four combinations; from
    the host function alone, each kind of history occurs in at least 20."""
    def nil_on_a_cycle(history, enc, out, keys):
        """By the binding's own version edges: nil reaches itself in one of the keys' graphs."""
        nm = WR._Names(history, enc, out)
        for k in keys:
            succ = WR.lin_version_edges(nm, k, True)
            stack, seen_v = list(succ.get(NIL, ())), set()
            while stack:
                v = stack.pop()
                if v == NIL:
                    return True
                if v not in seen_v:
                    seen_v.add(v)
                    stack.extend(succ.get(v, ()))
        return False

    seen = {}
    for seed in range(300):
        history = sized_history(seed)
        enc = WR.encode(history)
        res = {}
        for wfr, lin in COMBOS:
            res[(wfr, lin)] = _agree(ctx, enc.txns, enc.mops, wfr, lin, seed)
        (o0, s0, _), (o1, s1, l1) = res[(True, False)], res[(True, True)]
        cyc0 = set(o0["keys"]["key"][(o0["keys"]["flags"] & abi.LC_WR_K_CYCLIC) != 0].tolist())
        cyc1 = set(o1["keys"]["key"][(o1["keys"]["flags"] & abi.LC_WR_K_CYCLIC) != 0].tolist())
        # initial edges: a node txn's write each; without wfr every further version edge is a lin edge
        n_init = int((enc.txns["type"][np.repeat(np.arange(len(enc.txns)), enc.txns["mop_len"])] != FAIL)
                     [enc.mops["f"] == abi.LC_WR_WRITE].sum())
        kinds = {"valid-under-wfr": s0["valid"] == 1, "valid-to-cyclic": s0["valid"] == 1 and bool(cyc1),
                 "cyclic-only-with-lin": bool(cyc1 - cyc0),
                 "cycle-through-nil": nil_on_a_cycle(history, enc, o1, sorted(cyc1)),
                 "lin-edges-no-cycle": not cyc1 and res[(False, True)][2]["n_vedges"] > n_init,
                 "larger": len(enc.txns) >= 100}
        for k, v in kinds.items():
            seen[k] = seen.get(k, 0) + bool(v)
    print("kinds:", seen)
    assert all(seen[k] >= 20 for k in seen), seen


def test_synth_is_valid(ctx):
    txns, mops = WR.synth_arrays(20000)
    got, gs, gl = _agree(ctx, txns, mops, what="synth")
    assert gs["valid"] == 1 and gs["n_cyclic_keys"] == 0 and gl["n_pairs"] > gl["n_touches"] > 0


def test_checker_on_the_device_against_the_host_and_the_reference():
    dev = WR.WrChecker(device_mask=1, linearizable_keys=True)
    host = WR.WrChecker(device=False, linearizable_keys=True)
    try:
        for seed in range(40):
            h = C.random_history(seed)
            ref = REF.check(h, True, True)
            r = dev.check({}, h, {})
            assert r == host.check({}, h, {}), seed
            assert strip(r) == ref["result"], seed
            if ref["valid"] != "unknown":
                certify_version_cycles(r, ref)
            assert dev.last_lin["n_pairs"] == ref["lin_totals"]["pairs"]
    finally:
        dev.close()
