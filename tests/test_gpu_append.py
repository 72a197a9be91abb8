"""lc_append_check on the GPU against lc_append_check_host: every output array
and every count equal, at the smallest shapes where the kernels can go wrong:
read lengths and txn counts round the wave and the item pass's chunk, table
collisions and wrap-round, longest-read ties, the real-time extremes, the
host's slow paths, every error, workspace reuse, and in bulk."""
import errno

import numpy as np
import pytest

import append_cases as C
import append_ref as REF
from jepsen.etcd_amd import abi, append as AP
from test_append import EINVAL_CASES, KATS, _break, _good, certify_cycles, lib_view, strip_cycles

pytestmark = pytest.mark.gpu

COUNTS = ("valid", "n_incompatible_order", "n_nonprefix", "n_duplicate", "n_g1a", "n_phantom", "n_g1b",
          "n_internal", "n_class", "n_keys", "n_ok", "n_nodes", "n_edges", "n_scc", "n_cycles_returned")
ITEM_CHUNK = 4096  # txngraph.h, kItemChunk
M64 = (1 << 64) - 1
I64_MAX, I64_LOW = 2 ** 63 - 1, -2 ** 63 + 1


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


def _agree(ctx, txns, mops, values, what=""):
    want, ws = abi.append_check_host(txns, mops, values)
    got, gs = ctx.append_check(txns, mops, values)
    for f in want:
        assert want[f].shape == got[f].shape, (what, f, want[f].shape, got[f].shape)
        bad = np.nonzero(want[f] != got[f])[0]
        assert len(bad) == 0, (what, f, bad[:5].tolist(), want[f][bad[:3]].tolist(), got[f][bad[:3]].tolist())
    assert [gs[k] for k in COUNTS] == [ws[k] for k in COUNTS], (what, gs, ws)
    return got, gs


def _agree_history(ctx, history, what=""):
    enc = AP.encode(history)
    return _agree(ctx, enc.txns, enc.mops, enc.values, what)


def build(specs):
    """[(type, inv_pos, comp_pos, [("a", key, element) | ("r", key, payload or None)])] -> arrays."""
    txns = np.zeros(len(specs), dtype=abi.AP_TXN_DTYPE)
    mops, values = [], []
    for i, (typ, inv, comp, ms) in enumerate(specs):
        txns[i] = (len(mops), inv, comp, typ, len(ms))
        for f, k, v in ms:
            if f == "a":
                mops.append((k, v, abi.LC_AP_APPEND, 0))
            elif v is None:
                mops.append((k, 0, abi.LC_AP_READ, -1))
            else:
                mops.append((k, len(values), abi.LC_AP_READ, len(v)))
                values.extend(v)
    return txns, np.array(mops, dtype=abi.AP_MOP_DTYPE).reshape(-1), np.array(values, dtype=np.int64)


def serial(txn_mops, types=None):
    """The txns one after the other: txn i at positions 2 i, 2 i + 1."""
    return build([((types or {}).get(i, abi.LC_AP_OK), 2 * i,
                   -1 if (types or {}).get(i) == abi.LC_AP_INFO else 2 * i + 1, ms)
                  for i, ms in enumerate(txn_mops)])


def _mix64(x):
    x &= M64
    x ^= x >> 33
    x = x * 0xFF51AFD7ED558CCD & M64
    x ^= x >> 33
    x = x * 0xC4CEB9FE1A85EC53 & M64
    x ^= x >> 33
    return x


def _hash_pair(key, element):
    """txngraph.h's hash_pair."""
    return _mix64(_mix64(key) + 0x9E3779B97F4A7C15 + (element & M64))


@pytest.mark.parametrize("kat", KATS, ids=[k["name"] for k in KATS])
def test_kat(ctx, kat):
    got, gs = _agree_history(ctx, kat["history"], kat["name"])
    assert {1: True, 0: False, -1: "unknown"}[gs["valid"]] == kat["valid"]


@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, ITEM_CHUNK - 1, ITEM_CHUNK, ITEM_CHUNK + 1))
def test_read_lengths(ctx, n):
    """One key of n elements, each appended by its own txn; a read of every
    edge length up to n, each when the list has that length; then one
    non-prefix read one entry short."""
    elems = list(range(1, n + 1))
    edge = {0, 1, 63, 64, 65, n - 1, n}
    txs = [[("r", 7, [])]]
    for i, e in enumerate(elems, 1):
        txs.append([("a", 7, e)])
        if i in edge:
            txs.append([("r", 7, elems[:i])])
    got, gs = _agree(ctx, *serial(txs), what=n)
    assert gs["valid"] == 1 and gs["n_slow_reads"] == 0 and got["keys"]["len"].tolist() == [n]
    if n >= 2:
        txs.append([("r", 7, elems[1:])])
        got, gs = _agree(ctx, *serial(txs), what=(n, "non-prefix"))
        assert gs["n_nonprefix"] == 1 and gs["n_slow_reads"] == 1 and gs["n_incompatible_order"] == 1


@pytest.mark.parametrize("n_txns", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("n_keys", (1, 2, 65))
def test_txn_and_key_counts(ctx, n_txns, n_keys):
    for h in (C.sequential(n_txns, n_keys), C.concurrent(n_txns, n_keys)):
        got, gs = _agree_history(ctx, h, (n_txns, n_keys))
        assert gs["valid"] == 1 and gs["n_keys"] == min(n_keys, n_txns) and gs["n_nodes"] == n_txns


def test_writer_table_collisions_and_wrap(ctx):
    """Five (key, element) pairs that hash to the table's last slot (capacity
    64 for up to 32 appends): the probes wrap to slots 0..3.  Then elements
    that are read but were never written and hash there too."""
    key, cap = 3, 64
    last = [e for e in range(1, 4000) if _hash_pair(key, e) & (cap - 1) == cap - 1]
    assert len(last) >= 8
    txs = [[("a", key, e)] for e in last[:3]] + [[("r", key, last[:3])]] + \
        [[("a", key, e)] for e in last[3:5]] + [[("r", key, last[:5])]]
    got, gs = _agree(ctx, *serial(txs), what="wrap")
    assert gs["valid"] == 1 and gs["n_edges"] == 4 + 3  # ww; wr; wr and rw
    txs.append([("r", key, last[:5] + last[5:7])])  # two phantoms behind the wrapped run
    got, gs = _agree(ctx, *serial(txs), what="wrap-phantom")
    assert gs["n_phantom"] == 1 and got["keys"]["first_phantom"].tolist() == [5]


def test_key_table_collisions_and_wrap(ctx):
    """Keys whose slots are the key table's last (capacity 64 for 24 mops)."""
    cap = 64
    keys = [k for k in range(1, 4000) if _mix64(k) & (cap - 1) == cap - 1][:4]
    txs = [[("a", k, 10 * k + j)] for k in keys for j in range(3)] + [[("r", k, [10 * k, 10 * k + 1])] for k in keys]
    assert len(serial(txs)[1]) <= 32
    got, gs = _agree(ctx, *serial(txs), what="key-wrap")
    assert gs["valid"] == 1 and got["keys"]["key"].tolist() == sorted(keys)


def test_extreme_keys_and_elements(ctx):
    ext = [I64_MAX, I64_LOW, -1, 0, 1, I64_MAX - 1]
    txs = [[("a", k, e)] for k in ext for e in ext]
    txs += [[("r", k, ext)] for k in ext] + [[("r", ext[0], ext + [-2 ** 63])]]  # the reserved value, read
    got, gs = _agree(ctx, *serial(txs), what="extreme")
    assert gs["n_keys"] == len(ext) and gs["n_phantom"] == 1 and gs["n_nonprefix"] == 0


@pytest.mark.parametrize("shape", ("agree", "differ", "longest-last", "longest-first"))
def test_longest_read_ties(ctx, shape):
    txs = [[("a", 1, e)] for e in (1, 2, 3)]
    reads = {"agree": ([1, 2], [1, 2], [1]), "differ": ([1, 2], [2, 1], [1]),
             "longest-last": ([1], [1, 2], [1, 2, 3]), "longest-first": ([1, 2, 3], [1, 2], [1])}[shape]
    txs += [[("r", 1, list(r))] for r in reads]
    got, gs = _agree(ctx, *serial(txs), what=shape)
    first_longest = 3 + [len(r) for r in reads].index(max(map(len, reads)))
    assert got["keys"]["longest"].tolist() == [first_longest]
    assert gs["n_nonprefix"] == (1 if shape == "differ" else 0)


def test_real_time_sequential_and_concurrent(ctx):
    got, gs = _agree_history(ctx, C.sequential(130), "sequential")
    assert (got["rt_hi"] - got["rt_lo"]).tolist() == [0] + [1] * 129
    assert got["byc"][got["rt_lo"][1:]].tolist() == list(range(129))
    got, gs = _agree_history(ctx, C.concurrent(130), "concurrent")
    assert (got["rt_hi"] - got["rt_lo"]).tolist() == [0] * 130


def test_real_time_spanning_txn_and_infos(ctx):
    """An INFO txn before everything, one OK txn spanning the whole history,
    70 short txns inside it, an INFO txn after everything."""
    specs = [(abi.LC_AP_INFO, 0, -1, [("a", 1, 1000)]), (abi.LC_AP_OK, 1, 500, [("r", 2, [])])]
    for i in range(70):
        specs.append((abi.LC_AP_OK, 2 + 2 * i, 3 + 2 * i, [("a", 1, i + 1)]))
    specs.append((abi.LC_AP_INFO, 501, -1, [("a", 1, 2000), ("r", 1, None)]))
    got, gs = _agree(ctx, *build(specs), what="spanning")
    lo, hi = got["rt_lo"], got["rt_hi"]
    assert hi[0] == lo[0] and hi[1] == lo[1] and (hi[3:72] - lo[3:72] == 1).all()
    assert set(got["byc"][lo[72]:hi[72]].tolist()) == {1, 71}  # the spanning txn and the last short one
    assert gs["valid"] == 1 and gs["n_nodes"] == 73 and gs["n_ok"] == 71


def test_slow_paths(ctx):
    """Non-prefix reads with duplicates and failed elements inside them, an
    order with two phantoms that are one element, and internal reads behind a
    non-prefix read of the same txn."""
    txs = [[("a", 1, 1)], [("a", 1, 2)], [("a", 1, 3)], [("a", 1, 4), ("a", 2, 5)],
           [("r", 1, [1, 2, 3, 4])],
           [("r", 1, [2, 2, 1])],                       # non-prefix, a duplicate inside
           [("r", 1, [3, 4])],                          # non-prefix, a failed element inside
           [("r", 1, [2, 1]), ("r", 1, [2, 1]), ("a", 1, 6), ("r", 1, [2, 1])],  # internal behind a non-prefix read
           [("r", 2, [5, 77, 77])],                     # the order itself: two phantoms, one element
           [("r", 2, [5, 77])], [("r", 2, [5])]]
    got, gs = _agree(ctx, *serial(txs, {3: abi.LC_AP_FAIL}), what="slow")
    assert gs["n_slow_reads"] == 8 and gs["n_nonprefix"] == 5 and gs["n_duplicate"] == 2
    assert gs["n_g1a"] == 5 and gs["n_internal"] == 1 and gs["n_phantom"] == 2
    assert got["keys"]["first_dup"].tolist() == [-1, 2] and got["keys"]["first_phantom"].tolist() == [-1, 1]


def test_errors_leave_the_context_usable(ctx):
    good = _good()
    _agree(ctx, *good, what="before")
    for what in EINVAL_CASES:  # "pair-twice" is found only after the device has worked
        call = C.MarkedCall(*_break(what))
        assert call.run(ctx) == -errno.EINVAL and call.untouched(), what
        assert "lc_append_check" in ctx.last_error(), what
        with pytest.raises(abi.LcError) as e:
            ctx.append_check(*_break(what))
        assert e.value.code == -errno.EINVAL and "lc_append_check" in str(e.value), what
        _agree(ctx, *good, what=("after", what))
    # the same pair twice among many appends, far apart
    txs = [[("a", 1, e)] for e in range(1, 600)] + [[("a", 1, 300)]]
    call = C.MarkedCall(*serial(txs))
    assert call.run(ctx) == -errno.EINVAL and call.untouched() and "two appends" in ctx.last_error()
    _agree(ctx, *good, what="after far pair")


def test_empty_inputs(ctx):
    none = (np.zeros(0, abi.AP_TXN_DTYPE), np.zeros(0, abi.AP_MOP_DTYPE), [])
    got, gs = _agree(ctx, *none, what="no txns")
    assert gs["valid"] == -1
    got, gs = _agree(ctx, *serial([[], []]), what="txns without mops")
    assert gs["valid"] == 1 and gs["n_keys"] == 0
    got, gs = _agree(ctx, *serial([[("r", 1, [])], [("a", 1, 1)]]), what="no payload")
    assert gs["valid"] == 1 and gs["n_edges"] == 0
    got, gs = _agree(ctx, *serial([[("a", 1, 1)]], {0: abi.LC_AP_FAIL}), what="no ok txn")
    assert gs["valid"] == -1


def test_txns_without_mops_after_flagged_txns(ctx):
    """No kernel writes per-txn flags for a call without mops: what an earlier
    call on the context left in the workspace must not come back."""
    got, gs = _agree(ctx, *serial([[("r", 1, [9])], [("r", 1, [9, 8])], [("r", 2, [7])]]), what="flagged")
    assert (got["txn_flags"] == abi.LC_AP_R_PHANTOM).all() and gs["n_phantom"] == 3
    got, gs = _agree(ctx, *serial([[], [], []]), what="txns without mops, after flags")
    assert not got["txn_flags"].any() and gs["valid"] == 1
    got, gs = _agree(ctx, *serial([[], []], {0: abi.LC_AP_INFO, 1: abi.LC_AP_FAIL}), what="no ok, no mops")
    assert not got["txn_flags"].any() and gs["valid"] == -1


def test_only_the_unique_edges_are_written(ctx):
    """Key 1's order is a b c d by T0 T1 T0 T1: ww T0 -> T1 twice and T1 -> T0
    once among the set slots; the caller's edge array holds three records and
    nothing behind them."""
    specs = [(abi.LC_AP_OK, 0, 2, [("a", 1, 1), ("a", 1, 3)]), (abi.LC_AP_OK, 1, 3, [("a", 1, 2), ("a", 1, 4)]),
             (abi.LC_AP_OK, 4, 5, [("r", 1, [1, 2, 3, 4])])]
    got, gs = _agree(ctx, *build(specs), what="repeated edge")
    assert gs["n_edges"] == 3 and gs["n_class"][0] == 1  # the two ww edges and wr T1 -> T2; G0
    call = C.MarkedCall(*build(specs))
    assert call.run(ctx) == 0 and call.summary.n_edges == 3
    rest = call.arrays["edges"][3:]
    assert len(rest) == 3 and (rest.view(np.int8) == np.int8(C.MarkedCall.MARK)).all()


def test_payload_above_the_limit_is_e2big(ctx, monkeypatch):
    monkeypatch.setenv("LC_AP_MAX_PAYLOAD", "3")
    call = C.MarkedCall(*serial([[("a", 1, e)] for e in (1, 2, 3, 4)] + [[("r", 1, [1, 2, 3, 4])]]))
    assert call.run(ctx) == -errno.E2BIG and call.untouched() and "max_payload" in ctx.last_error()
    monkeypatch.delenv("LC_AP_MAX_PAYLOAD")
    monkeypatch.setenv("LC_AP_MAX_MOPS", "4")  # the call has five
    call = C.MarkedCall(call.txns, call.mops, call.values)
    assert call.run(ctx) == -errno.E2BIG and call.untouched() and "max_mops" in ctx.last_error()
    monkeypatch.delenv("LC_AP_MAX_MOPS")
    _agree(ctx, call.txns, call.mops, call.values, what="after E2BIG")


def test_workspace_reuse(ctx):
    small, large = AP.synth_arrays(200, seed=3), AP.synth_arrays(5000, seed=4)
    bad = AP.encode(C.random_history(7, n_txns=60, faults=("garble", "split"), p_fault=0.3))
    for what, arrays in (("small", small), ("large", large), ("small again", small),
                         ("anomalous", (bad.txns, bad.mops, bad.values)), ("large again", large)):
        _agree(ctx, *arrays, what=what)
    # the mix of sizes flips while the total stays about the same: many txns on
    # two keys with a short read now and then (of its own key while that is
    # short, later of a key nobody appends to), against few txns on many keys
    # whose reads are long.  On a fresh context the per-txn arrays shrink and
    # the per-item arrays grow, so every array moves inside a workspace that
    # does not grow, and back.
    lists = {0: [], 1: []}
    many_txns = []
    for i in range(400):
        lists[i % 2].append(i + 1)
        read = ("r", i % 2, list(lists[i % 2])) if i < 24 else ("r", 2, [])
        many_txns.append([("a", i % 2, i + 1)] + [read] * (i % 8 == 7))
    long_reads = []
    for k in range(30):
        elems = [1000 + 8 * k + j for j in range(8)]
        long_reads += [[("a", k, e) for e in elems], [("r", k, elems)], [("r", k, elems)]]
    many_txns, long_reads = serial(many_txns), serial(long_reads)
    assert len(many_txns[0]) > 4 * len(long_reads[0]) and 3 * len(many_txns[2]) < len(long_reads[2])
    with abi.Context(device_mask=1) as c:
        for what, arrays in (("many txns", many_txns), ("long reads", long_reads), ("many txns again", many_txns)):
            _, gs = _agree(c, *arrays, what=what)
            assert gs["valid"] == 1, what


N_BULK, AT_LEAST = 300, 20


def test_bulk_random_histories(ctx):
    seen = {}
    for i in range(N_BULK):
        h = C.random_history(20000 + i, n_txns=5 + (i * 37) % 296, faults=C.FAULTS + C.SCRIPTED, p_fault=0.1,
                             sliding=True)
        enc = AP.encode(h)
        got, gs = _agree(ctx, enc.txns, enc.mops, enc.values, what=i)
        certify_cycles(enc, got, gs)
        for name in [c for c, n in zip(abi.LC_AP_CLASSES, gs["n_class"]) if n] + \
                [f for f in COUNTS[2:8] if gs[f]]:
            seen[name] = seen.get(name, 0) + 1
    short = {n: seen.get(n, 0) for n in abi.LC_AP_CLASSES + COUNTS[2:8] if seen.get(n, 0) < AT_LEAST}
    assert not short, (short, seen)


def test_twenty_thousand_txns(ctx):
    got, gs = _agree(ctx, *AP.synth_arrays(20000, seed=11), what="20k")
    assert gs["valid"] == 1 and gs["n_slow_reads"] == 0 and gs["n_nodes"] == 20000 and gs["n_edges"] > 20000


def test_checker_on_the_device(ctx):
    dev, host = AP.AppendChecker(device_mask=1), AP.AppendChecker(device=False)
    try:
        for seed, faults in ((1, ()), (2, ("stale", "split")), (3, ("garble", "leak", "behind")),
                             (4, ("insert", "skew"))):
            h = C.random_history(500 + seed, n_txns=40, faults=faults, p_fault=0.2, sliding=True)
            a, b = dev.check({}, h, {}), host.check({}, h, {})
            assert a == b, (seed, a, b)
            assert strip_cycles(a) == REF.check(h)["result"], seed
            enc = AP.encode(h)
            assert lib_view(enc, dev.last_out, dev.last_summary)["edges"] == REF.check(h)["edges"]
    finally:
        dev.close()
