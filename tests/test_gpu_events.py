"""lc_check_events on the GPU: the device's split / completion / packing
against lc_events_pack_host bit for bit, and its results against lc_check32 on
the host-packed records, at every size where the kernels change path."""
import errno

import numpy as np
import pytest

import events_ref as ER
from events_ref import CAS, FAIL, INFO, INV, OK, R, W
from jepsen.etcd_amd import abi, events as E, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = abi.Context(device_mask=1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def limits():
    return abi.events_limits()


@pytest.fixture(scope="module")
def jepsen_batch():
    hist, labels = synth.jepsen_history(40, 150, p_info=0.05, p_anomaly=0.3, seed=77)
    return hist, labels


def _same_pack(host, dev, what):
    for name, a, b in zip(("ops32", "key_off", "key_base", "completion"), host, dev):
        assert a.shape == b.shape, (what, name, a.shape, b.shape)
        diff = np.nonzero((a != b).reshape(len(a), -1).any(axis=1))[0]
        assert len(diff) == 0, (what, name, diff[:5].tolist(), a[diff[:3]].tolist(), b[diff[:3]].tolist())


def _agree(ctx, ev, n_keys, opts=None, what=""):
    """events_pack and check_events against the host pack and check32 on it.
    Returns (results, witness, kind, cert, the call's statistics, host pack)."""
    host = abi.pack_events_host(ev, n_keys)
    _same_pack(host, ctx.events_pack(ev, n_keys), what + " events_pack")
    rc, res, wit, kind, cert, cset, packed = ctx.check_events(
        ev, n_keys, opts, witness=True, certificate=True, packed=True)
    stats = ctx.last_events_stats()
    _same_pack(host, packed, what + " check_events")
    ops32, key_off, key_base, _ = host
    rc2, rres, rwit, rkind, rcert, rcset = ctx.check32(ops32, key_off, key_base, opts, witness=True,
                                                       certificate=True)
    assert rc == rc2 == 0
    bad = np.nonzero(res != rres)[0]
    assert len(bad) == 0, (what, [(int(k), res[k].tolist(), rres[k].tolist()) for k in bad[:5]])
    assert (kind == rkind).all() and (cert == rcert).all(), what
    # the per-record outputs where the ABI defines them: the witness of a key
    # that has one, the first cert[3] set entries of a HALL / PROOF key
    for k in range(n_keys):
        a, b = int(key_off[k]), int(key_off[k + 1])
        if kind[k] != abi.LC_WITNESS_NONE:
            assert (wit[a:b] == rwit[a:b]).all(), (what, "witness", k)
        if cert[k][0] in (abi.LC_CERT_HALL, abi.LC_CERT_PROOF):
            c = int(cert[k][3])
            assert (cset[a:a + c] == rcset[a:a + c]).all(), (what, "certificate_set", k)
    assert stats["n_ops"] == len(ops32) and stats["n_events"] == len(ev)
    assert stats["n_client"] == int((ev[:, 0] >= 0).sum())
    return res, wit, kind, cert, stats, host


def test_hand_stream_every_rule(ctx):
    s = ER.Stream()
    # key 0: plain pairs, a crashed op, :info, double invoke, orphans
    s.add(0, 1, INV, W, 1)               # 0  ok pair
    s.add(2, 9, INV, CAS, 1, 2)          # 1  key 2: its only pairs fail -> empty key
    s.add(0, 1, OK, W, 1, version=1)     # 2
    s.skip()                             # 3
    s.add(0, 2, OK, R, 1, version=1)     # 4  completion without invoke: ignored
    s.add(0, 2, INV, R)                  # 5  invoke followed by an invoke: pending forever
    s.add(0, 2, INV, R)                  # 6  ... this one is paired
    s.add(1, 1, INV, W, 7)               # 7  key 1, the same process number as key 0's
    s.add(0, 2, OK, R, 1, version=1)     # 8
    s.add(0, 2, OK, R, 1, version=1)     # 9  repeated completion: ignored
    s.add(2, 9, FAIL, CAS, 1, 2)         # 10
    s.add(0, 3, INV, CAS, 2, 1)          # 11 fail pair: no record
    s.add(0, 3, FAIL, CAS, 2, 1)         # 12
    s.add(0, 3, INV, W, 3)               # 13 :info: the invoke's fields, ret = INF, completion kept
    s.add(0, 3, INFO, W, 9, version=5)   # 14
    s.add(1, 1, OK, W, 7, version=1)     # 15
    s.add(0, 4, INV, 3, 5)               # 16 unknown :f
    s.add(0, 4, OK, 3, 5)                # 17
    s.add(0, 5, INV, W, 2)               # 18 bad shape on the completion
    s.add(0, 5, OK, W, 2, version=2, bad=1)  # 19
    s.add(0, 6, INV, W, 2, bad=1)        # 20 bad shape on the invoke only: the :ok's fields count
    s.add(0, 6, OK, W, 2, version=2)     # 21
    s.add(0, 7, INV, W, 2, bad=1)        # 22 ... and with :info the invoke's do
    s.add(0, 7, INFO, W, 2)              # 23
    s.add(0, 8, INV, W, 4)               # 24 completion :f differs from the invoke's -> 3
    s.add(0, 8, OK, R, 4, version=3)     # 25
    s.add(2, 9, INV, CAS, 1, 2)          # 26
    s.add(2, 9, FAIL, CAS, 1, 2)         # 27
    s.add(1, -5, INV, R)                 # 28 a negative process number; never completed
    s.add(1, 2 ** 31 - 1, INV, R)        # 29
    s.add(1, 2 ** 31 - 1, OK, R, 7, version=1)  # 30
    s.skip()                             # 31
    s.add(0, 1, INFO, W, 1)              # 32 :info without invoke: ignored
    s.add(0, 1, INV, R)                  # 33
    s.add(0, 1, FAIL, R)                 # 34
    s.add(0, 1, INV, R)                  # 35 the stream ends on an open invoke
    ev = s.array()
    res, wit, kind, cert, stats, host = _agree(ctx, ev, 3, what="hand")
    ops32, key_off, key_base, completion = host
    assert key_off.tolist() == [0, 10, 13, 13] and key_base.tolist() == [0, 7, 0]
    inf = -1  # LC_INF32 read as int32
    assert ops32[:10].tolist() == [
        [W, 1, -1, 1, 0, 2], [R, -1, -1, -1, 5, inf], [R, 1, -1, 1, 6, 8], [W, 3, -1, -1, 13, inf],
        [3, -1, -1, -1, 16, 17], [3, -1, -1, -1, 18, 19], [W, 2, -1, 2, 20, 21],
        [3, -1, -1, -1, 22, inf], [3, -1, -1, -1, 24, 25], [R, -1, -1, -1, 35, inf]]
    assert completion[:10].tolist() == [2, -1, 8, 14, 17, 19, 21, 23, 25, -1]
    assert ops32[10:].tolist() == [[W, 7, -1, 1, 0, 8], [R, -1, -1, -1, 21, inf], [R, 7, -1, 1, 22, 23]]
    assert stats["n_fail_pairs"] == 4 and stats["n_ignored_completions"] == 3
    assert stats["n_big_keys"] == 0


def _boundary_sizes(L):
    return [1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024, 1025, L - 1, L, L + 1, 2 * L + 3]


def test_boundary_size_list_matches_limits(limits):
    assert _boundary_sizes(limits["max_lds_events"]) == _boundary_sizes(4096)


@pytest.mark.parametrize("n", _boundary_sizes(4096))
def test_boundary_sizes(ctx, limits, n):
    """Key 0 has n events, with one process's invoke on the last event of
    every 64-event chunk of its subhistory and the completion on the first of
    the next; key 1's three events are first, in the middle and last."""
    L = limits["max_lds_events"]
    k0 = ER.key_subhistory(n, key=0)
    k1 = [(1, 3, ER.tf(INV, W), 1, -1, -1), (1, 3, ER.tf(OK, W), 1, -1, 1),
          (1, 3, ER.tf(INV, R), -1, -1, -1)]
    rows = [k1[0]] + k0[:n // 2] + [k1[1]] + k0[n // 2:] + [k1[2]]
    ev = np.array(rows, dtype=np.int64).astype(np.int32)
    res, wit, kind, cert, stats, host = _agree(ctx, ev, 2, what="n=%d" % n)
    ops32, key_off, key_base, completion = host
    # the straddling pairs are there: one record per chunk edge, returning one event later
    sub = np.nonzero(ev[:, 0] == 0)[0]
    edges = [j for j in range(63, n - 1, 64)]
    recs = {(int(key_base[0]) + int(np.uint32(c)), int(key_base[0]) + int(np.uint32(r)))
            for c, r in ops32[:key_off[1], 4:6]}
    for j in edges:
        assert (int(sub[j]), int(sub[j + 1])) in recs, (n, j)
    assert (stats["n_big_keys"] >= 1) == (n > L)
    assert res["verdict"][1] == abi.LC_VALID
    assert res["verdict"][0] == abi.LC_VALID


@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_process_table_capacity(ctx, limits, delta):
    """P distinct processes in one key, each with one crashed invoke and then
    one :ok pair, for P around the LDS table's capacity."""
    P = limits["lds_process_capacity"] + delta
    procs = [(p * 7919) % 1000003 - 500000 for p in range(P)]
    assert len(set(procs)) == P
    s = ER.Stream()
    for p in procs:
        s.add(0, p, INV, R)
    version = 0
    for i, p in enumerate(procs):
        s.add(0, p, INV, W, i % 5)
        version += 1
        s.add(0, p, OK, W, i % 5, version=version)
    res, wit, kind, cert, stats, host = _agree(ctx, s.array(), 1, what="P=%d" % P)
    assert len(host[0]) == 2 * P and (host[3] >= 0).sum() == P
    # the same with a second key in front, so that the split runs too
    ev = np.concatenate([np.array(ER.pairs_key(0, 6), dtype=np.int64).astype(np.int32),
                         s.array() + np.array([1, 0, 0, 0, 0, 0], dtype=np.int32)])
    _, _, _, _, stats, host = _agree(ctx, ev, 2, what="P=%d, two keys" % P)
    assert host[1].tolist() == [0, 3, 3 + 2 * P]


def test_many_keys(ctx):
    n_keys = 257
    parts = [ER.pairs_key(k, 6 + k % 3, proc_base=k % 4) for k in range(n_keys)]
    # round-robin: event i belongs to key i mod 257 (as long as the key has events left)
    rows = [parts[k][j] for j in range(8) for k in range(n_keys) if j < len(parts[k])]
    rr = np.array(rows, dtype=np.int64).astype(np.int32)
    assert (rr[:6 * n_keys, 0] == np.arange(6 * n_keys) % n_keys).all()
    res, *_ = _agree(ctx, rr, n_keys, what="round-robin")
    assert (res["verdict"] == abi.LC_VALID).all()
    contiguous = np.array([r for p in parts for r in p], dtype=np.int64).astype(np.int32)
    res, *_ = _agree(ctx, contiguous, n_keys, what="contiguous")
    assert (res["verdict"] == abi.LC_VALID).all()
    n_keys = 5000
    ev = ER.interleave([ER.pairs_key(k, 6, proc_base=k % 7) for k in range(n_keys)], seed=3)
    res, _, _, _, stats, host = _agree(ctx, ev, n_keys, what="5000 keys")
    assert (np.diff(host[1]) == 3).all() and (res["verdict"] == abi.LC_VALID).all()


def test_hot_key(ctx, limits):
    parts = [ER.key_subhistory(20000, key=0)] + [ER.pairs_key(k, 10, proc_base=k) for k in range(1, 64)]
    ev = ER.interleave(parts, seed=4)
    res, _, _, _, stats, host = _agree(ctx, ev, 64, what="hot key")
    assert stats["n_big_keys"] == (1 if 20000 > limits["max_lds_events"] else 0)
    assert (res["verdict"] == abi.LC_VALID).all()


def test_one_key_mutex(ctx):
    """n_keys == 1: no split at all.  A 20,000-event lock history without
    jepsen.independent, nemesis ops in between."""
    hist = []
    for i in range(5000):
        p = i % 3
        for f in ("acquire", "release"):
            hist.append({"type": "invoke", "f": f, "process": p, "value": None})
            if i % 50 == 7 and f == "acquire":
                hist.append({"type": "info", "f": "start-partition", "process": "nemesis", "value": None})
            hist.append({"type": "ok", "f": f, "process": p, "value": None})
    hist = hist[:20000]
    ev, keys, _, _ = E.encode(hist, "mutex", independent=False)
    assert keys == [None] and len(ev) == 20000
    opts = abi.default_opts(init_value=0)
    res, _, _, _, stats, host = _agree(ctx, ev, 1, opts, what="one key")
    assert res["verdict"][0] == abi.LC_VALID and stats["n_big_keys"] == 0
    assert stats["n_client"] == 20000 - sum(1 for op in hist if op["process"] == "nemesis")


def test_skipped_events(ctx):
    """Half the stream is LC_EV_SKIP, with skipped events at positions 63-65
    and 255-257 of the stream."""
    parts = [ER.pairs_key(k, 40, proc_base=k) for k in range(5)]
    client = ER.interleave(parts, seed=5)
    n = 2 * len(client)
    skip = np.zeros(n, dtype=bool)
    skip[[63, 64, 65, 255, 256, 257]] = True
    rest = np.nonzero(~skip)[0]
    rng = np.random.default_rng(6)
    skip[rng.choice(rest, n // 2 - 6, replace=False)] = True
    ev = np.zeros((n, 6), dtype=np.int32)
    ev[:, 0] = E.LC_EV_SKIP
    ev[~skip] = client
    assert (ev[[63, 64, 65, 255, 256, 257], 0] == E.LC_EV_SKIP).all() and skip.sum() == n // 2
    res, *_ = _agree(ctx, ev, 5, what="skips")
    assert (res["verdict"] == abi.LC_VALID).all()
    # and with one key, where the walk itself passes over them
    one = ev.copy()
    one[~skip] = np.array(ER.pairs_key(0, len(client), n_procs=5), dtype=np.int64).astype(np.int32)
    res, *_ = _agree(ctx, one, 1, what="skips, one key")
    assert res["verdict"][0] == abi.LC_VALID


def test_end_to_end_jepsen_history(ctx, jepsen_batch):
    hist, labels = jepsen_batch
    ev, keys, _, _ = E.encode(hist)
    res, wit, kind, cert, stats, host = _agree(ctx, ev, len(keys), what="jepsen history")
    assert keys == list(range(40))
    # the generator's labels: a key with an anomaly is invalid, a clean key valid
    for k, lab in enumerate(labels):
        assert res["verdict"][k] == (abi.LC_VALID if lab == 0 else abi.LC_INVALID), (k, lab)
    assert (kind[res["verdict"] == abi.LC_INVALID] == abi.LC_WITNESS_PREFIX).all()
    assert stats["n_fail_pairs"] > 0


def test_flags_counted_and_witness(ctx):
    """A small mutex history with 70 crashed acquires: decided by the counted
    tier, with a certified order."""
    from jepsen.etcd_amd import witness as Wt
    hist = []
    for i in range(20):
        for f in ("acquire", "release"):
            hist.append({"type": "invoke", "f": f, "process": i % 2, "value": None})
            hist.append({"type": "ok", "f": f, "process": i % 2, "value": None})
        if i == 5:
            for p in range(70):
                hist.append({"type": "invoke", "f": "acquire", "process": 100 + p, "value": None})
    for p in range(70):
        hist.append({"type": "info", "f": "acquire", "process": 100 + p, "value": None})
    ev, keys, _, _ = E.encode(hist, "mutex", independent=False)
    flags = abi.LC_FLAG_COUNTED_CLASSES | abi.LC_FLAG_SEARCH_WITNESS | abi.LC_FLAG_COUNTED_WITNESS
    opts = abi.default_opts(init_value=0, flags=flags)
    res, wit, kind, cert, stats, host = _agree(ctx, ev, 1, opts, what="flags")
    assert res["verdict"][0] == abi.LC_VALID
    assert kind[0] == abi.LC_WITNESS_ORDER_FULL
    ops32, key_off, key_base, _ = host
    ops = np.zeros((len(ops32), 6), dtype=np.int64)
    ops[:, :4] = ops32[:, :4]
    ops[:, 4] = ops32[:, 4].astype(np.uint32)
    r = ops32[:, 5].astype(np.uint32).astype(np.int64)
    ops[:, 5] = np.where(r == abi.LC_INF32, abi.LC_INF, r)
    assert Wt.certify(ops, wit, int(kind[0]), cut=-2, init=(0, 0))


def test_workspace_reuse(ctx):
    big = ER.interleave([ER.pairs_key(k, 300, proc_base=k) for k in range(50)], seed=7)
    small = ER.interleave([ER.pairs_key(k, 5) for k in range(3)], seed=8)
    for what, ev, n_keys in (("big", big, 50), ("small", small, 3), ("big again", big, 50),
                             ("small, more keys than events use", small, 80)):
        res, *_ = _agree(ctx, ev, n_keys, what=what)
        assert (res["verdict"] == abi.LC_VALID).all()
    # the mix of sizes flips while the total stays about the same: on a fresh
    # context the per-event arrays shrink and the per-key arrays grow, so every
    # array moves inside a workspace that does not grow, and back
    one = np.array(ER.pairs_key(0, 800), dtype=np.int64).astype(np.int32)
    many = ER.interleave([ER.pairs_key(k, 4, proc_base=k % 5) for k in range(150)], seed=11)
    with abi.Context(device_mask=1) as c:
        for what, ev, n_keys in (("one key", one, 1), ("many keys", many, 150), ("one key again", one, 1)):
            res, *_ = _agree(c, ev, n_keys, what=what)
            assert (res["verdict"] == abi.LC_VALID).all()


def test_bad_key_in_the_middle(ctx):
    ev = ER.interleave([ER.pairs_key(k, 200, proc_base=k) for k in range(4)], seed=9)
    for col, val in ((0, 4), (0, -2), (2, 7)):
        bad = ev.copy()
        bad[len(ev) // 2, col] = val
        with pytest.raises(abi.LcError) as e:
            ctx.check_events(bad, 4)
        assert e.value.code == -errno.EINVAL
        with pytest.raises(abi.LcError) as e:
            ctx.events_pack(bad, 4)
        assert e.value.code == -errno.EINVAL and str(len(ev) // 2) in str(e.value)
        # the context stays usable
        res, *_ = _agree(ctx, ev, 4, what="after an error")
        assert (res["verdict"] == abi.LC_VALID).all()
    rc, res = ctx.check_events(np.zeros((0, 6), np.int32), 0)
    assert rc == 0 and len(res) == 0


def test_checker_device_split(jepsen_batch, capsys):
    from jepsen.etcd_amd import checker as C, diagnostics as D
    hist, _ = jepsen_batch
    a = C.register_checker(device_mask=1)
    b = C.register_checker(device_mask=1, device_split=True)
    try:
        ra, rb = a.check({}, hist, {}), b.check({}, hist, {})
    finally:
        a.close()
        b.close()
    assert b.split_fallbacks == 0
    assert ra["valid?"] == rb["valid?"] and ra["failures"] == rb["failures"] and ra["failures"]
    assert list(ra["results"]) == list(rb["results"])
    n_sets = 0
    for k in ra["results"]:
        la, lb = ra["results"][k]["linear"], rb["results"][k]["linear"]
        assert la["valid?"] == lb["valid?"], k
        for f in ("op", "fail-prefix-end", "previous-ok", "cause"):
            assert la.get(f) == lb.get(f), (k, f)
        assert la.get("certificate", {}).get("kind") == lb.get("certificate", {}).get("kind"), k
        # :configs / :final-paths list up to MAX_ENTRIES in an order that
        # follows id hashes: comparable as sets only where both list all
        for f in ("configs", "final-paths"):
            if f in la and f in lb and len(la[f]) < D.MAX_ENTRIES and len(lb[f]) < D.MAX_ENTRIES:
                assert sorted(map(repr, la[f])) == sorted(map(repr, lb[f])), (k, f)
                n_sets += 1
    with capsys.disabled():
        print("\ndevice_split: %d :configs / :final-paths lists compared as sets over %d invalid keys"
              % (n_sets, len(ra["failures"])))
