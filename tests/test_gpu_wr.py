"""lc_wr_check on the GPU against lc_wr_check_host: every output array and
every count equal, with the wfr inference on and off, at the smallest shapes
where the kernels can go wrong: txn and key counts round the wave, version
chains and cycles round the wave and the pointer doubling's rounds, reader x
child products round the wave and the item pass's chunk, table collisions and
wrap-round, the real-time extremes, every error, workspace reuse, and in
bulk."""
import errno

import numpy as np
import pytest

import wr_cases as C
import wr_ref as REF
from jepsen.etcd_amd import abi, wr as WR
from test_wr import EINVAL_CASES, KATS, _good, certify_cycles, lib_view, marked, strip_cycles

pytestmark = pytest.mark.gpu

COUNTS = ("valid", "n_internal", "n_phantom", "n_g1a", "n_g1b", "n_cyclic_keys", "n_lost_update", "n_class",
          "n_keys", "n_versions", "n_ok", "n_nodes", "n_edges", "n_edges_raw", "n_scc", "n_cycles_returned")
ITEM_CHUNK = 4096  # txngraph.h, kItemChunk
M64 = (1 << 64) - 1
I64_MAX, I64_LOW = 2 ** 63 - 1, -2 ** 63 + 1
NIL = abi.LC_WR_NIL
OK, INFO, FAIL = abi.LC_WR_OK, abi.LC_WR_INFO, abi.LC_WR_FAIL
BOTH = pytest.mark.parametrize("wfr", (True, False), ids=("wfr", "no-wfr"))


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def _agree(ctx, txns, mops, wfr=True, what=""):
    want, ws = abi.wr_check_host(txns, mops, wfr)
    got, gs = ctx.wr_check(txns, mops, wfr)
    for f in want:
        assert want[f].shape == got[f].shape, (what, f, want[f].shape, got[f].shape)
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), want[f][bad[:3]].tolist(), got[f][bad[:3]].tolist())
    assert [gs[k] for k in COUNTS] == [ws[k] for k in COUNTS], (what, gs, ws)
    return got, gs


def _agree_history(ctx, history, wfr=True, what=""):
    enc = WR.encode(history)
    return _agree(ctx, enc.txns, enc.mops, wfr, what)


def build(specs):
    """[(type, inv_pos, comp_pos, [("w", key, value) | ("r", key, value, NIL or None: unknown)])] -> arrays."""
    txns = np.zeros(len(specs), dtype=abi.WR_TXN_DTYPE)
    mops = []
    for i, (typ, inv, comp, ms) in enumerate(specs):
        txns[i] = (len(mops), inv, comp, typ, len(ms))
        for f, k, v in ms:
            if f == "w":
                mops.append((k, v, abi.LC_WR_WRITE, 0))
            elif v is None:
                mops.append((k, 0, abi.LC_WR_READ, 0))
            else:
                mops.append((k, v, abi.LC_WR_READ, 1))
    return txns, np.array(mops, dtype=abi.WR_MOP_DTYPE).reshape(-1)


def serial(txn_mops, types=None):
    """The txns one after the other: txn i at positions 2 i, 2 i + 1."""
    return build([((types or {}).get(i, OK), 2 * i, -1 if (types or {}).get(i) == INFO else 2 * i + 1, ms)
                  for i, ms in enumerate(txn_mops)])


def overlapping(txn_mops):
    """All txns invoked before any completes: no real-time edge."""
    n = len(txn_mops)
    return build([(OK, i, n + i, ms) for i, ms in enumerate(txn_mops)])


def _mix64(x):
    x &= M64
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & M64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & M64
    x ^= x >> 33
    return x


def _hash_pair(key, value):
    """txngraph.h's hash_pair."""
    return _mix64(_mix64(key) + 0x9E3779B97F4A7C15 + (value & M64))


def chain(n, key=1, first=None, base=0):
    """n versions base + 1 .. base + n of one key: txn i reads version i and
    writes version i + 1; the first txn reads `first` (None: it only writes)."""
    txs = [([("r", key, first)] if first is not None else []) + [("w", key, base + 1)]]
    return txs + [[("r", key, base + i), ("w", key, base + i + 1)] for i in range(1, n)]


@BOTH
@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(ctx, kat, wfr):
    got, gs = _agree_history(ctx, kat["history"], wfr, kat["name"])
    assert {1: True, 0: False, -1: "unknown"}[gs["valid"]] == kat["valid" if wfr else "valid-off"]


@BOTH
@pytest.mark.parametrize("n_txns", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("n_keys", (1, 2, 65))
def test_txn_and_key_counts(ctx, n_txns, n_keys, wfr):
    for h in (C.sequential(n_txns, n_keys), C.concurrent(n_txns, n_keys)):
        got, gs = _agree_history(ctx, h, wfr, (n_txns, n_keys))
        assert gs["valid"] == 1 and gs["n_keys"] == min(n_keys, n_txns) and gs["n_nodes"] == n_txns


CHAINS = (1, 2, 3, 63, 64, 65, 4096, 4097)


@BOTH
@pytest.mark.parametrize("n", CHAINS)
def test_version_chains(ctx, n, wfr):
    """A wfr chain of n versions on one key, txn after txn: acyclic, valid,
    and with wfr one ww edge per link."""
    got, gs = _agree(ctx, *serial(chain(n)), wfr, what=n)
    assert gs["valid"] == 1 and gs["n_cyclic_keys"] == 0 and got["keys"]["n_versions"].tolist() == [n + 1]
    assert int((got["edges"]["type"] == abi.LC_AP_WW).sum()) == (n - 1 if wfr else 0)


@BOTH
@pytest.mark.parametrize("n", CHAINS)
def test_version_cycles(ctx, n, wfr):
    """The same chain closed: the first txn reads the last version.  n = 1 is
    the self-loop.  The versions are 10 .. 9 + n: cyc_value is 10."""
    got, gs = _agree(ctx, *overlapping(chain(n, first=9 + n, base=9)), wfr, what=n)
    # (without wfr a txn that reads what it alone writes is nothing; two or more still read in a wr cycle)
    assert gs["valid"] == (1 if n == 1 and not wfr else 0) and gs["n_cyclic_keys"] == (1 if wfr else 0)
    assert got["keys"]["cyc_value"].tolist() == [10 if wfr else NIL]
    assert not (got["edges"]["type"] != abi.LC_AP_WR).any()  # a cyclic key keeps its wr edges alone


@BOTH
def test_long_chain_below_a_short_cycle(ctx, wfr):
    """5000 <-> 5001, and a chain of 4,096 smaller versions hanging from 5000:
    below the cycle, not on it."""
    txs = [[("r", 1, 5001), ("w", 1, 5000)], [("r", 1, 5000), ("w", 1, 5001)]] + chain(4096, first=5000)
    got, gs = _agree(ctx, *overlapping(txs), wfr, what="below")
    assert got["keys"]["cyc_value"].tolist() == [5000 if wfr else NIL] and gs["n_lost_update"] == 1


@BOTH
def test_a_cyclic_key_takes_no_other_key_s_edges(ctx, wfr):
    cyc = [[("r", 1, 12), ("w", 1, 11)], [("r", 1, 11), ("w", 1, 12)]]
    other = [[("r", 2, NIL)], [("w", 2, 21)], [("r", 2, 21), ("w", 2, 22)]]
    got, gs = _agree(ctx, *overlapping(cyc + other), wfr, what="two keys")
    e = got["edges"]
    on2 = {(int(x["from"]), int(x["to"]), int(x["type"])) for x in e[e["key"] == 2]}
    assert on2 == {(2, 3, abi.LC_AP_RW), (2, 4, abi.LC_AP_RW), (3, 4, abi.LC_AP_WR)} | \
        ({(3, 4, abi.LC_AP_WW)} if wfr else set())
    assert {int(x["type"]) for x in e[e["key"] == 1]} == {abi.LC_AP_WR}
    assert got["keys"]["flags"].tolist() == [abi.LC_WR_K_CYCLIC if wfr else 0, 0]


@BOTH
@pytest.mark.parametrize("r", (0, 1, 63, 64, 65))
@pytest.mark.parametrize("c", (0, 1, 63, 64, 65))
def test_reader_child_products(ctx, r, c, wfr):
    """Key 1: version 1, r txns that read it and c txns that read it and write
    (r + c readers x c children with wfr).  Key 2: r readers of nil against c
    writers.  All concurrent."""
    txs = [[("w", 1, 1)]] + [[("r", 1, 1)] for _ in range(r)] + [[("r", 1, 1), ("w", 1, 100 + i)] for i in range(c)]
    txs += [[("r", 2, NIL)] for _ in range(r)] + [[("w", 2, 200 + i)] for i in range(c)]
    got, gs = _agree(ctx, *overlapping(txs), wfr, what=(r, c))
    rw = int((got["edges"]["type"] == abi.LC_AP_RW).sum())
    assert rw == r * c + ((r + c) * c - c if wfr else 0)  # (a child's own rw leads to itself)
    assert gs["n_lost_update"] == (1 if c >= 2 else 0)


def test_product_across_the_item_chunk(ctx):
    """300 readers of nil against 300 writers: 90,000 items, 22 chunks; the
    binding's default edge room does not hold them, so it comes again."""
    txs = [[("r", 1, NIL)] for _ in range(300)] + [[("w", 1, i + 1)] for i in range(300)]
    assert 300 * 300 > 21 * ITEM_CHUNK
    got, gs = _agree(ctx, *overlapping(txs), True, what="300 x 300")
    assert gs["n_edges"] == gs["n_edges_raw"] == 90000 and gs["valid"] == 1


@BOTH
@pytest.mark.parametrize("n_writers", (1, 64, 65))
def test_nil_readers_against_writers(ctx, n_writers, wfr):
    """Three nil readers, then the writers one after the other, each reading
    its predecessor's value: every reader precedes every writer."""
    txs = [[("r", 1, NIL)] for _ in range(3)] + chain(n_writers, first=NIL)
    got, gs = _agree(ctx, *serial(txs), wfr, what=n_writers)
    assert int((got["edges"]["type"] == abi.LC_AP_RW).sum()) == 3 * n_writers + (n_writers - 1)
    assert gs["valid"] == 1


@BOTH
def test_version_table_collisions_and_wrap(ctx, wfr):
    """(key, value) pairs that hash to the table's last slot (capacity 64 for
    up to 32 mops), written and read, and one that is only read: the probes
    wrap to the first slots."""
    key, cap = 3, 64
    last = [v for v in range(1, 6000) if _hash_pair(key, v) & (cap - 1) == cap - 1]
    assert len(last) >= 7
    txs = chain(1, key, base=last[0] - 1) + [[("r", key, a), ("w", key, b)] for a, b in zip(last[:5], last[1:6])]
    txs.append([("r", key, last[6])])  # behind the wrapped run, nobody's
    arrays = serial(txs)
    assert len(arrays[1]) <= 32
    got, gs = _agree(ctx, *arrays, wfr, what="wrap")
    assert gs["n_phantom"] == 1 and gs["n_versions"] == 8 and gs["n_internal"] == 0


def test_key_table_collisions_and_wrap(ctx):
    cap = 64
    keys = [k for k in range(1, 4000) if _mix64(k) & (cap - 1) == cap - 1][:4]
    txs = [[("w", k, 10 * k + j)] for k in keys for j in range(3)] + [[("r", k, 10 * k + 2)] for k in keys]
    assert len(serial(txs)[1]) <= 32
    got, gs = _agree(ctx, *serial(txs), what="key-wrap")
    assert gs["valid"] == 1 and got["keys"]["key"].tolist() == sorted(keys)


@BOTH
def test_extreme_keys_and_values_and_a_value_equal_across_keys(ctx, wfr):
    ext = [I64_MAX, I64_LOW, -1, 0, 1, I64_MAX - 1]
    txs = [[("w", k, v)] for k in ext for v in ext]          # every value on every key
    txs += [[("r", k, v), ("r", k2, v)] for k, k2, v in zip(ext, ext[1:] + ext[:1], ext)]
    # a cycle among the extremes: its least value is the int64 order's, not the unsigned one's
    txs += [[("r", 7, I64_MAX), ("w", 7, I64_LOW)], [("r", 7, I64_LOW), ("w", 7, -1)], [("r", 7, -1), ("w", 7, I64_MAX)]]
    got, gs = _agree(ctx, *overlapping(txs), wfr, what="extreme")
    assert gs["n_keys"] == len(ext) + 1 and gs["n_phantom"] == 0
    assert got["keys"]["cyc_value"][got["keys"]["key"] == 7].tolist() == [I64_LOW if wfr else NIL]


@BOTH
def test_real_time_sequential_and_concurrent(ctx, wfr):
    got, gs = _agree_history(ctx, C.sequential(130), wfr, "sequential")
    assert (got["rt_hi"] - got["rt_lo"]).tolist() == [0] + [1] * 129
    assert got["byc"][got["rt_lo"][1:]].tolist() == list(range(129))
    got, gs = _agree_history(ctx, C.concurrent(130), wfr, "concurrent")
    assert (got["rt_hi"] - got["rt_lo"]).tolist() == [0] * 130


def test_real_time_spanning_txn_and_infos(ctx):
    """An INFO txn before everything, one OK txn spanning the whole history,
    70 short txns inside it, an INFO txn after everything."""
    specs = [(INFO, 0, -1, [("w", 1, 1000)]), (OK, 1, 500, [("r", 2, NIL)])]
    for i in range(70):
        specs.append((OK, 2 + 2 * i, 3 + 2 * i, [("w", 1, i + 1)]))
    specs.append((INFO, 501, -1, [("w", 1, 2000), ("r", 1, None)]))
    got, gs = _agree(ctx, *build(specs), what="spanning")
    lo, hi = got["rt_lo"], got["rt_hi"]
    assert hi[0] == lo[0] and hi[1] == lo[1] and (hi[3:72] - lo[3:72] == 1).all()
    assert set(got["byc"][lo[72]:hi[72]].tolist()) == {1, 71}  # the spanning txn and the last short one
    assert gs["valid"] == 1 and gs["n_nodes"] == 73 and gs["n_ok"] == 71


def test_errors_leave_the_context_usable(ctx):
    good = _good()
    _agree(ctx, *good, what="before")
    for what in EINVAL_CASES:  # "pair-twice" is found only after the device has worked
        call = marked(what)
        assert call.run(ctx) == -errno.EINVAL and call.untouched(), what
        assert "lc_wr_check" in ctx.last_error(), what
        _agree(ctx, *good, what=("after", what))
    call = C.MarkedCall(*good)
    call.flags = 2
    assert call.run(ctx) == -errno.EINVAL and call.untouched() and "flag" in ctx.last_error()
    # the same pair twice among many writes, far apart
    txs = [[("w", 1, v)] for v in range(1, 600)] + [[("w", 1, 300)]]
    call = C.MarkedCall(*serial(txs))
    assert call.run(ctx) == -errno.EINVAL and call.untouched() and "two writes" in ctx.last_error()
    with pytest.raises(abi.LcError) as e:
        ctx.wr_check(*serial(txs))
    assert e.value.code == -errno.EINVAL and "two writes" in str(e.value)
    _agree(ctx, *good, what="after far pair")


def test_candidate_edges_above_the_limit_are_e2big(ctx, monkeypatch):
    arrays = serial([[("r", 1, NIL)], [("r", 1, NIL)], [("w", 1, 1)], [("w", 1, 2)], [("r", 1, 2)]])
    monkeypatch.setenv("LC_WR_MAX_EDGES", "8")  # five mop slots and four rw items
    call = C.MarkedCall(*arrays)
    assert call.run(ctx) == -errno.E2BIG and call.untouched() and "max_edges" in ctx.last_error()
    monkeypatch.setenv("LC_WR_MAX_EDGES", "9")
    _agree(ctx, *arrays, what="at the limit")
    monkeypatch.delenv("LC_WR_MAX_EDGES")
    monkeypatch.setenv("LC_WR_MAX_MOPS", "4")  # the call has five
    call = C.MarkedCall(*arrays)
    assert call.run(ctx) == -errno.E2BIG and call.untouched() and "max_mops" in ctx.last_error()
    monkeypatch.delenv("LC_WR_MAX_MOPS")
    _agree(ctx, *arrays, what="after E2BIG")


def test_enospc_names_both_numbers_and_writes_no_array(ctx):
    lost = next(k for k in KATS if k["name"] == "lost-update")
    enc = WR.encode(lost["history"])
    call = C.MarkedCall(enc.txns, enc.mops, True, edge_cap=5)
    assert call.run(ctx) == -errno.ENOSPC and call.arrays_untouched()
    assert call.summary.n_edges == 6 and call.summary.n_edges_raw == 6
    assert "6 edges" in ctx.last_error() and "edge_cap 5" in ctx.last_error()
    call = C.MarkedCall(enc.txns, enc.mops, True, edge_cap=6)
    assert call.run(ctx) == 0 and call.summary.n_edges == 6
    _agree(ctx, enc.txns, enc.mops, what="after ENOSPC")


def test_empty_inputs(ctx):
    none = (np.zeros(0, abi.WR_TXN_DTYPE), np.zeros(0, abi.WR_MOP_DTYPE))
    got, gs = _agree(ctx, *none, what="no txns")
    assert gs["valid"] == -1
    got, gs = _agree(ctx, *serial([[], []]), what="txns without mops")
    assert gs["valid"] == 1 and gs["n_keys"] == 0
    got, gs = _agree(ctx, *serial([[("r", 1, NIL)]]), what="one nil read")
    assert gs["valid"] == 1 and gs["n_edges"] == 0 and gs["n_versions"] == 1
    got, gs = _agree(ctx, *serial([[("w", 1, 1)]], {0: FAIL}), what="no ok txn")
    assert gs["valid"] == -1


def test_txns_without_mops_after_flagged_txns(ctx):
    """No kernel writes per-txn flags for a call without mops: what an earlier
    call on the context left in the workspace must not come back."""
    got, gs = _agree(ctx, *serial([[("r", 1, 9)], [("r", 1, 8)], [("r", 2, 7)]]), what="flagged")
    assert (got["txn_flags"] == abi.LC_WR_R_PHANTOM).all() and gs["n_phantom"] == 3
    got, gs = _agree(ctx, *serial([[], [], []]), what="txns without mops, after flags")
    assert not got["txn_flags"].any() and gs["valid"] == 1
    got, gs = _agree(ctx, *serial([[], []], {0: INFO, 1: FAIL}), what="no ok, no mops")
    assert not got["txn_flags"].any() and gs["valid"] == -1


def test_workspace_reuse(ctx):
    small, large = WR.synth_arrays(200, seed=3), WR.synth_arrays(5000, seed=4)
    bad = WR.encode(C.random_history(7, n_txns=60, faults=("garble", "split", "loop"), p_fault=0.3))
    for what, arrays in (("small", small), ("large", large), ("small again", small),
                         ("anomalous", (bad.txns, bad.mops)), ("large again", large)):
        _agree(ctx, *arrays, what=what)
    # the mix of sizes flips while the total stays about the same: many txns
    # with one mop each and hardly an rw item, against few txns with four mops
    # each whose nil readers and writers make many items.  On a fresh context
    # the per-txn arrays shrink and the edge buffers grow inside an arena that
    # the first call sized, and back.
    many_txns = serial([[("w", i % 2, i + 1)] for i in range(1500)])
    products = overlapping([[("r", k, NIL) for k in range(4)] for _ in range(30)] +
                           [[("w", k, 100 * j + k) for k in range(4)] for j in range(30)])
    assert len(many_txns[0]) > 20 * len(products[0])
    with abi.Context(device_mask=1) as c:
        for what, arrays in (("many txns", many_txns), ("products", products), ("many txns again", many_txns),
                             ("products again", products)):
            _, gs = _agree(c, *arrays, what=what)
            assert gs["valid"] == 1, what
    with abi.Context(device_mask=1) as c:  # the item count above the first run's guess on a new arena
        _, gs = _agree(c, *products, what="products first")
        assert gs["n_edges"] == 4 * 30 * 30


N_BULK, AT_LEAST = 300, 20
BULK_NAMES = abi.LC_AP_CLASSES + ("n_internal", "n_phantom", "n_g1a", "n_g1b", "n_cyclic_keys", "n_lost_update")


def bulk_history(i):
    return C.random_history(20000 + i, n_txns=5 + (i * 37) % 296, faults=C.FAULTS + C.SCRIPTED, p_fault=0.1,
                            sliding=True)


def test_bulk_random_histories(ctx):
    seen = {}
    for i in range(N_BULK):
        enc = WR.encode(bulk_history(i))
        got, gs = _agree(ctx, enc.txns, enc.mops, True, what=i)
        certify_cycles(got, gs)
        if i % 3 == 0:
            _agree(ctx, enc.txns, enc.mops, False, what=(i, "no-wfr"))
        for name in [c for c, n in zip(abi.LC_AP_CLASSES, gs["n_class"]) if n] + [f for f in BULK_NAMES[8:] if gs[f]]:
            seen[name] = seen.get(name, 0) + 1
    short = {n: seen.get(n, 0) for n in BULK_NAMES if seen.get(n, 0) < AT_LEAST}
    assert not short, (short, seen)


@BOTH
def test_twenty_thousand_txns(ctx, wfr):
    got, gs = _agree(ctx, *WR.synth_arrays(20000, seed=11), wfr, what="20k")
    assert gs["valid"] == 1 and gs["n_nodes"] == 20000 and gs["n_edges"] > 20000


def test_checker_on_the_device(ctx):
    for wfr in (True, False):
        dev, host = WR.WrChecker(device_mask=1, wfr_keys=wfr), WR.WrChecker(device=False, wfr_keys=wfr)
        try:
            for seed, faults in ((1, ()), (2, ("stale", "split")), (3, ("garble", "leak", "behind")),
                                 (4, ("double", "skew")), (5, ("loop", "g0"))):
                h = C.random_history(500 + seed, n_txns=40, faults=faults, p_fault=0.2, sliding=True)
                a, b = dev.check({}, h, {}), host.check({}, h, {})
                assert a == b, (seed, a, b)
                ref = REF.check(h, wfr)
                assert strip_cycles(a) == ref["result"], seed
                assert lib_view(WR.encode(h), dev.last_out, dev.last_summary)["edges"] == ref["edges"]
        finally:
            dev.close()
