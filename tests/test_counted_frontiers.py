"""knossos's :configs from the counted search in one device call
(lc_check_frontiers_counted, include/lincheck_counted.h): keys with more than
64 ops open, every pending list whole.

Two hand-derived mutex keys pin pending lists beyond 64 entries exactly.  The
rest is compared with the oracle's JITC frontier (oracle.frontier), which is
exact in size and states, and in pending sets where a configuration has fewer
than 64 pending ops (it lists the first 64)."""
import collections
import functools
import random

import numpy as np
import pytest

import oracle
from helpers import FREE, HELD, INF, C, N, R, W, pack_keys
from jepsen.etcd_amd import abi
from test_counted import _crashed_writes, crashy, jitc, layout_ref, packed

ACQ, REL = [C, HELD, FREE, N], [C, FREE, HELD, N]


def k1():
    """70 crashed acquires, then two sequential :ok acquires: invalid at the
    second, whose frontier is (1, HELD) with 71 ops pending."""
    return [ACQ + [i, INF] for i in range(70)] + [ACQ + [70, 71], ACQ + [72, 73]]


def k2():
    """70 crashed releases, a crashed acquire called after each of the first
    three, then four sequential :ok releases: each of the first three needs
    one of the acquires, so the fourth (record 76) fails from (6, FREE) with
    every acquire linearized (retired) and every crashed release pending."""
    recs, t = [], 0
    for i in range(70):
        recs.append(REL + [t, INF]); t += 1
        if i < 3:
            recs.append(ACQ + [t, INF]); t += 1
    for _ in range(4):
        recs.append(REL + [t, t + 1]); t += 2
    return recs


# ------------------------------------------------------------------ CPU tests

def test_symbol_and_abi_version():
    L = abi.lib()
    assert L.lc_check_frontiers_counted is not None
    assert L.lc_abi_version() == 5


def test_null_context_is_einval():
    L = abi.lib()
    assert L.lc_check_frontiers_counted(None, None, None, 0, None, None, None, 1, None, None,
                                        None, 0) == -22


def test_binding_and_checker_import_without_a_gpu():
    import inspect
    from jepsen.etcd_amd import checker, diagnostics
    sig = inspect.signature(abi.Context.check_frontiers_counted)
    assert list(sig.parameters)[1:] == ["ops", "key_off", "stop_ops", "max_per_key", "opts"]
    assert sig.parameters["max_per_key"].default == 10
    assert abi.COUNTED_CONFIG_DTYPE.itemsize == 32
    assert checker.RegisterChecker()._fx is None
    # pending lists longer than 64 pass through to :configs
    done = [{"invoke": {"i": i}, "type": "info", "ret": INF, "call": i} for i in range(80)]
    out = diagnostics.frontier_analysis(done, 0, 100, [(1, 1, tuple(range(80)))], [0, 1],
                                        versioned=False)
    assert len(out["configs"][0]["pending"]) == 80


def test_checker_routes_the_keys_the_slot_search_left_out():
    """_configs gives the keys lc_check_frontiers left None one
    check_frontiers_counted call, under the one-key fallback's gate; an
    LcError from it is recorded on those keys, which then fall back."""
    from jepsen.etcd_amd import checker

    class Stub:
        def __init__(self, fail):
            self.fail, self.calls = fail, []

        def check_frontiers(self, ops, off, stops, mx, opts):
            return [[(0, 0, (0,))]] + [None] * (len(off) - 2)

        def check_frontiers_counted(self, ops, off, stops, mx, opts):
            self.calls.append((len(ops), off.tolist(), [int(s) for s in stops], mx))
            if self.fail:
                raise abi.LcError(-5, "boom")
            return [[(1, 1, tuple(range(70)))], None][:len(off) - 1], np.array([1, -1])

    recs = [[W, 1, N, N, 2 * i, 2 * i + 1] for i in range(3)]
    crashed = [[W, 1, N, N, i, INF] for i in range(20)]
    ops, off = pack_keys([recs, recs + recs, crashed, recs, crashed])
    res = np.zeros(5, dtype=abi.RESULT_DTYPE)
    res["verdict"] = [0, 0, 0, 1, 0]
    res["fail_op"] = [2, 5, 19, -1, 7]
    for fail in (False, True):
        ck = checker.RegisterChecker()
        ck._ctx = stub = Stub(fail)
        errors = {}
        # key 2 is witnessed with 20 crashed ops (beyond the gate); key 4 is not witnessed
        got = ck._configs(ops, off, res, None, [False, True, True, False, False], errors)
        assert stub.calls == [(26, [0, 6, 26], [5, 7], 10)]
        if fail:
            assert got == {0: [(0, 0, (0,))]}
            assert sorted(errors) == [1, 4] and all("boom" in e for e in errors.values())
        else:
            assert got == {0: [(0, 0, (0,))], 1: [(1, 1, tuple(range(70)))]} and errors == {}
        ck._ctx = None


def test_hand_derived_keys_against_the_oracle():
    """The oracle's verdicts on K1 / K2, and its frontier (capped at 64)."""
    for recs, fail, state in ((k1(), 71, (1, HELD)), (k2(), 76, (6, FREE))):
        ops, off = pack_keys([recs])
        _, j = oracle.check(ops, off, algo=oracle.JITC, init_value=FREE)
        assert (int(j["verdict"][0]), int(j["fail_op"][0])) == (0, fail)
        want, n = oracle.frontier(ops, fail, max_configs=16, init_value=FREE)
        assert n == 1
        (ver, val, pend), = want
        assert (ver, val) == state and len(pend) == 64


# ------------------------------------------------------------------ GPU tests

def check_invariants(recs, stop, cfgs):
    """Test 5: what holds of every configuration returned."""
    stop_ret = recs[stop][5]
    classes = collections.OrderedDict()  # tuple -> members called by the stop, in record order
    for i, r in enumerate(recs):
        if r[0] in (W, C) and r[5] == INF and r[4] < stop_ret:
            classes.setdefault(tuple(r[:4]), []).append(i)
    for ver, val, pend in cfgs:
        assert list(pend) == sorted(set(pend)), pend
        ps = set(pend)
        for i in pend:
            f, v, _, rver, call, ret = recs[i]
            assert call < stop_ret <= ret, (i, recs[i])
            assert not (f == R and ret == INF), i
            assert not (f == R and v == N and rver == N), i
        for members in classes.values():
            flags = [i in ps for i in members]
            assert flags == sorted(flags), (members, pend)  # a suffix


@pytest.fixture(scope="module")
def gctx():
    with abi.Context(1) as c:
        yield c


@pytest.mark.gpu
def test_k1_71_pending(gctx):
    recs = k1()
    ops, off = pack_keys([recs])
    cfgs, totals = gctx.check_frontiers_counted(ops, off, [71], 10, abi.default_opts(init_value=FREE))
    assert totals.dtype == np.int64 and totals.tolist() == [1]
    assert cfgs == [[(1, HELD, tuple(list(range(70)) + [71]))]]
    check_invariants(recs, 71, cfgs[0])


@pytest.mark.gpu
def test_k2_retired_acquires_are_not_pending(gctx):
    recs = k2()
    assert len(recs) == 77
    ops, off = pack_keys([recs])
    cfgs, totals = gctx.check_frontiers_counted(ops, off, [76], 10, abi.default_opts(init_value=FREE))
    releases = [i for i, r in enumerate(recs) if r[:4] == REL and r[5] == INF]
    assert len(releases) == 70
    assert totals.tolist() == [1]
    assert cfgs == [[(6, FREE, tuple(releases + [76]))]]
    check_invariants(recs, 76, cfgs[0])


AB_INVALID = {"A": [1, 3, 7, 11, 14, 15, 17], "B": [1, 3]}
AB_BELOW_64 = {"A": [3, 11, 15, 17], "B": [1, 3]}  # every oracle configuration < 64 pending


@functools.lru_cache(maxsize=None)
def ab_frontier(name, k):
    """The oracle's frontier of batch key k at its failing return: (set of
    (version, value, sorted pending), size).  Computed once."""
    ops, off, init = packed(name)
    want, n = oracle.frontier(ops[off[k]:off[k + 1]], int(jitc(name)["fail_op"][k]),
                              max_configs=4096, init_value=init)
    return frozenset((v, x, tuple(sorted(p))) for v, x, p in want), n


def sub_batch(name, ks):
    ops, off, init = packed(name)
    sub_ops, sub_off = pack_keys([ops[off[k]:off[k + 1]].tolist() for k in ks])
    return sub_ops, sub_off, jitc(name)["fail_op"][ks], abi.default_opts(init_value=init)


def test_batches_a_b_are_as_the_issue_states():
    for name, ks in AB_INVALID.items():
        j = jitc(name)
        assert [k for k in range(len(j)) if j["verdict"][k] == 0] == ks
        sizes = [ab_frontier(name, k)[1] for k in ks]
        assert 126 <= min(sizes) and max(sizes) <= 1911
        below = [k for k in ks if all(len(p) < 64 for _, _, p in ab_frontier(name, k)[0])]
        assert below == AB_BELOW_64[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_batches_first_ten(gctx, name):
    ks = AB_INVALID[name]
    sub_ops, sub_off, stops, o = sub_batch(name, ks)
    cfgs, totals = gctx.check_frontiers_counted(sub_ops, sub_off, stops, 10, o)
    for j, k in enumerate(ks):
        want, n = ab_frontier(name, k)
        assert cfgs[j] is not None, k
        assert int(totals[j]) == n and len(cfgs[j]) == min(10, n), (k, int(totals[j]), n)
        assert len(set(cfgs[j])) == len(cfgs[j]), k
        by_state = collections.defaultdict(list)
        for v, x, p in want:
            by_state[(v, x)].append(p)
        for c in cfgs[j]:
            assert matches_an_oracle_configuration(c, by_state), (k, c)
        check_invariants(sub_ops[sub_off[j]:sub_off[j + 1]].tolist(), int(stops[j]), cfgs[j])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_batches_whole_frontier(gctx, name):
    ks = AB_INVALID[name]
    sub_ops, sub_off, stops, o = sub_batch(name, ks)
    cfgs, totals = gctx.check_frontiers_counted(sub_ops, sub_off, stops, 2048, o)
    for j, k in enumerate(ks):
        want, n = ab_frontier(name, k)
        assert cfgs[j] is not None and int(totals[j]) == n == len(cfgs[j]), k
        if k in AB_BELOW_64[name]:
            assert set(cfgs[j]) == want, k
        else:
            cut = lambda cs: collections.Counter((v, x, min(len(p), 64)) for v, x, p in cs)
            assert cut(cfgs[j]) == cut(want), k
        check_invariants(sub_ops[sub_off[j]:sub_off[j + 1]].tolist(), int(stops[j]), cfgs[j])


def matches_an_oracle_configuration(cfg, by_state):
    """Equal to an oracle configuration of fewer than 64 pending ops, or a
    superset of one the oracle cut at 64."""
    v, x, p = cfg
    return any(q == p if len(q) < 64 else (len(q) == 64 and set(q) <= set(p))
               for q in by_state.get((v, x), ()))


@pytest.mark.gpu
def test_next_capacity_and_no_op_return(gctx):
    """Batch B's key 7 (valid) passes through a frontier of 30,895
    configurations, more than the first set capacity holds: its search is
    retried at the next.  At the return of record 557 the frontier holds
    11,148 configurations; record 560's return is a no-op (n = total = 0)."""
    ops, off, init = packed("B")
    assert int(jitc("B")["max_frontier"][7]) == 30895
    recs = ops[off[7]:off[8]]
    want, n = oracle.frontier(recs, 557, max_configs=16384, init_value=init)
    assert n == 11148 == len(want)
    assert oracle.frontier(recs, 560, max_configs=16, init_value=init)[1] == 0
    by_state = collections.defaultdict(list)
    for v, x, p in want:
        by_state[(v, x)].append(tuple(sorted(p)))
    sub_ops, sub_off = pack_keys([recs.tolist(), recs.tolist()])
    cfgs, totals = gctx.check_frontiers_counted(sub_ops, sub_off, [557, 560], 10,
                                                abi.default_opts(init_value=init))
    assert totals.tolist() == [11148, 0]
    assert cfgs[1] == [] and len(cfgs[0]) == 10 == len(set(cfgs[0]))
    for c in cfgs[0]:
        assert matches_an_oracle_configuration(c, by_state), c
    check_invariants(recs.tolist(), 557, cfgs[0])


@functools.lru_cache(maxsize=None)
def small_keys():
    rng = random.Random(0xF108)
    keys = [crashy(rng, rng.randrange(100, 200), 0.25, [R, R, W, C], p_perturb=1.0)
            for _ in range(24)]
    ops, off = pack_keys(keys)
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8, max_configs=1 << 22)
    inv = [k for k in range(len(keys)) if j["verdict"][k] == 0]
    want = []
    for k in inv:
        w, n = oracle.frontier(ops[off[k]:off[k + 1]], int(j["fail_op"][k]), max_configs=4096)
        assert n == len(w)
        want.append(frozenset((v, x, tuple(sorted(p))) for v, x, p in w))
    return keys, inv, [int(j["fail_op"][k]) for k in inv], want


def test_small_keys_are_as_the_issue_states():
    keys, inv, _, want = small_keys()
    assert len(inv) == 17
    crashed = [sum(1 for r in keys[k] if r[5] == INF) for k in inv]
    assert (min(crashed), max(crashed)) == (8, 29)
    assert max(len(w) for w in want) == 252
    assert max(len(p) for w in want for _, _, p in w) == 26


@pytest.mark.gpu
def test_same_answers_as_the_slot_search(gctx):
    keys, inv, stops, want = small_keys()
    ops, off = pack_keys([keys[k] for k in inv])
    cfgs, totals = gctx.check_frontiers_counted(ops, off, stops, 512)
    slot = gctx.check_frontiers(ops, off, stops, 512)
    assert sum(s is not None for s in slot) >= 1
    for j, k in enumerate(inv):
        assert cfgs[j] is not None, k
        assert set(cfgs[j]) == want[j] and int(totals[j]) == len(want[j]), k
        assert len(cfgs[j]) == len(want[j]), k
        if slot[j] is not None:
            assert set(slot[j]) == set(cfgs[j]), k
        check_invariants(keys[k], stops[j], cfgs[j])


@pytest.mark.gpu
def test_keys_the_search_cannot_reach(gctx):
    ops_a, off_a, init = packed("A")
    a14 = ops_a[off_a[14]:off_a[15]].tolist()
    a14_stop = int(jitc("A")["fail_op"][14])
    many = _crashed_writes([4] * 17)
    t = len(many)
    many += [[W, 1, N, N, t, t + 1], [R, 1, N, N, t + 2, t + 3]]
    assert not layout_ref(many)["fits"]
    two = [[W, 1, N, N, 0, 1], [R, 2, N, N, 2, 3], [R, 1, N, N, 4, 5]]  # fails at record 1
    good = _crashed_writes([3, 3]) + [[W, 5, N, N, 6, 7], [R, 0, N, N, 8, 9]]
    keys = [good, many, _crashed_writes([2]) + [[R, N, N, N, 2, 3]], two, good, a14, good]
    stops = [7, len(many) - 1, 0, 2, 7, a14_stop, 7]
    ops, off = pack_keys(keys)
    want, n = oracle.frontier(np.array(good), 7, max_configs=64)
    want = {(v, x, tuple(sorted(p))) for v, x, p in want}
    cfgs, totals = gctx.check_frontiers_counted(ops, off, stops, 64)
    assert [c is None for c in cfgs] == [False, True, True, True, False, False, False]
    assert totals.tolist()[1:4] == [-1, -1, -1]
    for j in (0, 4, 6):  # the other keys of the same call are unaffected
        assert set(cfgs[j]) == want and int(totals[j]) == n
    assert int(totals[5]) == ab_frontier("A", 14)[1]
    # the configuration budget
    cfgs, totals = gctx.check_frontiers_counted(ops, off, stops, 64,
                                                abi.default_opts(max_configs_per_key=1000))
    assert [c is None for c in cfgs] == [False, True, True, True, False, True, False]
    assert int(totals[5]) == -1 and set(cfgs[6]) == want
    # pending_cap one short
    import ctypes
    n_keys, mx = len(keys), 4
    cfg = np.zeros(n_keys * mx, dtype=abi.COUNTED_CONFIG_DTYPE)
    pend = np.zeros(mx * len(ops), dtype=np.int64)
    n_out = np.zeros(n_keys, dtype=np.int32)
    tot = np.zeros(n_keys, dtype=np.int64)
    st = np.array(stops, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    o = abi.default_opts()
    call = lambda cap: abi.lib().lc_check_frontiers_counted(
        gctx._h, p(ops), p(off), n_keys, p(st), ctypes.byref(o), p(cfg), mx, p(n_out), p(tot),
        p(pend), cap)
    assert call(mx * len(ops) - 1) == -22
    assert "pending_cap" in gctx.last_error()
    assert call(mx * len(ops)) == 0
    assert n_out.tolist() == [min(mx, n), -1, -1, -1, min(mx, n), mx, min(mx, n)]


def k1_history():
    h = [{"type": "invoke", "f": "acquire", "process": i, "value": None} for i in range(70)]
    for p in (70, 71):
        h.append({"type": "invoke", "f": "acquire", "process": p, "value": None})
        h.append({"type": "ok", "f": "acquire", "process": p, "value": None})
    return h


def test_k1_history_packs_to_k1():
    from jepsen.etcd_amd import history as H
    _, ops, off, _ = H.pack(k1_history(), model="mutex", independent=False)
    assert ops.tolist() == k1() and off.tolist() == [0, 72]


@pytest.mark.gpu
def test_drop_in_reports_71_pending_invokes():
    from jepsen.etcd_amd import checker
    seen = []
    for _ in range(2):  # two contexts open in turn
        ck = checker.RegisterChecker(model=checker.Mutex(), independent=False, device_mask=1)
        try:
            res = ck.check({}, k1_history())
            assert ck._fx is None  # the frontier exchange was never opened
        finally:
            ck.close()
        assert res["valid?"] is False
        assert "configs-error" not in res
        assert len(res["configs"]) == 1
        pend = res["configs"][0]["pending"]
        assert len(pend) == 71 and all(op["type"] == "invoke" for op in pend)
        assert sorted(op["process"] for op in pend) == list(range(70)) + [71]
        seen.append(res)
    assert seen[0] == seen[1]
