"""LC_FLAG_COUNTED_WITNESS: linearization orders for the keys the counted
tier decides (include/lincheck.h; the device search: the counted stage of
csrc/witness_search.hip).  The first witness stage gives every open op a
window slot, so a key with more than 64 ops open — 70 crashed acquires — gets
no order from it; the counted stage counts the crashed writes/CAS per class.

tests/counted_order_ref.py restates the search with the device's order of
trial, so the device's step counts are compared with it.  Every order the
device returns is certified from the records alone by tests/order_ref.py and
by jepsen/etcd_amd/witness.py, which must agree.  Every GPU run also makes the
same call with LC_FLAG_SEARCH_WITNESS alone: results, the kinds and witnesses
that call gave, and lc_last_witness_stats must not move."""
import functools
import os
import random
import re

import numpy as np
import pytest

import counted_order_ref as cref
import oracle
from helpers import FREE, HELD, INF, C, N, R, W, pack_keys
from jepsen.etcd_amd import abi, checker
from test_counted import _crashed_writes, batch, crashy, jitc, packed
from test_counted_frontiers import k1, k2
from test_search_witness import MODELS, both, searched

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = abi.LC_FLAG_COUNTED_CLASSES
SW = abi.LC_FLAG_SEARCH_WITNESS
CW = getattr(abi, "LC_FLAG_COUNTED_WITNESS", 0)
FULL, PREFIX = 3, 4
ACQ, REL = [C, HELD, FREE, N], [C, FREE, HELD, N]
MAX_STEPS, MAX_STORED = 4096, 2048  # a sixteenth of kWitnessNodeCap; a tenth of the cache


# ------------------------------------------------------------------ the keys

def overflow70():
    """The key of test_search_witness.py::test_window_overflow."""
    recs = [ACQ + [t, INF] for t in range(70)]
    return recs + [ACQ + [70, 71], REL + [72, 73], REL + [74, 75]]


def dead_end_with_counts():
    """test_hand_cases' cas-register key (its first candidate is a dead end)
    65 events later, behind 65 crashed writes of a value nobody reads."""
    casreg = [[W, 0, N, N, 0, 3], [C, 2, N, N, 1, 5], [W, 1, N, N, 2, 6], [C, 0, 1, N, 4, 8],
              [R, 0, N, N, 7, 9]]
    return [[W, 7, N, N, t, INF] for t in range(65)] + \
        [r[:4] + [r[4] + 65, r[5] + 65] for r in casreg]


def width_edge(m, extra=False):
    """m crashed acquires, then m sequential :ok releases (each needs one of
    them); with `extra` one release more, which none is left for."""
    recs = [ACQ + [t, INF] for t in range(m)]
    recs += [REL + [m + 2 * j, m + 2 * j + 1] for j in range(m + (1 if extra else 0))]
    return recs


@functools.lru_cache(maxsize=None)
def astride_key():
    """A 2-valued register key of 70+ records with 65+ crashed writes, a class
    with members on both sides of record 64 and :ok ops open across its call."""
    for seed in range(1000):
        rng = random.Random(seed)
        recs = crashy(rng, 110, 0.85, [R, W, W], p_perturb=0.0)
        if len(recs) < 70:
            continue
        crashed = [i for i, r in enumerate(recs) if r[0] == W and r[5] == INF]
        t = recs[64][4]
        across = sum(1 for r in recs[:64] if r[5] != INF and r[5] > t)
        sides = any(recs[a][:4] == recs[b][:4] for a in crashed if a < 64 for b in crashed if b >= 64)
        if len(crashed) >= 65 and across >= 2 and sides:
            return tuple(map(tuple, recs))
    raise AssertionError("no key with a class astride the chunk boundary")


def budget_key():
    recs, t = overflow70(), 76
    for _ in range(20):
        recs += [ACQ + [t, t + 1], REL + [t + 2, t + 3]]
        t += 4
    return recs


def read_budget_key():
    """70 crashed CAS from a value that never occurs, a write, 12 sequential
    reads of it: the tiers take the reads in their read closure (as in
    test_search_witness.py::test_budget), ranking them takes a step each."""
    recs = [[C, 5, 9, N, t, INF] for t in range(70)] + [[W, 1, N, N, 70, 71]]
    return recs + [[R, 1, N, N, 72 + 2 * i, 73 + 2 * i] for i in range(12)]


def many_classes_key():
    """60 crashed CAS of 17 classes, each from a value that never occurs (so
    the tiers' search does not branch on them), an :ok write without a version
    (the search tiers' key), six [nil nil] reads open at once (the tiers give
    those no slot): 66 ops open for the first stage, 17 classes."""
    recs = [[C, r[1], 100 + r[1], N, r[4], INF] for r in _crashed_writes([4] * 9 + [3] * 8)]
    recs.append([W, 50, N, N, 60, 61])
    return recs + [[R, N, N, N, 62 + i, 70 + i] for i in range(6)]


def many_open_key():
    """70 crashed writes of one value (a 7-bit field: 57 slots), an :ok write
    without a version and 58 [nil nil] reads open at once."""
    recs = [[W, 1, N, N, t, INF] for t in range(70)] + [[W, 2, N, N, 70, 71]]
    return recs + [[R, N, N, N, 72 + i, 200 + i] for i in range(58)]


HAND = {"overflow70": (overflow70, FREE), "k1": (k1, FREE), "k2": (k2, FREE),
        "dead-end": (dead_end_with_counts, N), "astride": (astride_key, N)}
for _m in (63, 64, 65, 127, 128):
    HAND["width-%d" % _m] = (functools.partial(width_edge, _m), FREE)
    HAND["width-%d+1" % _m] = (functools.partial(width_edge, _m, True), FREE)


@functools.lru_cache(maxsize=None)
def hand_ref(name):
    """(records, init, cut, restatement's Result) of a hand key; the cut is
    the oracle's (None: valid)."""
    make, init = HAND[name]
    recs = [list(r) for r in make()]
    ops, off = pack_keys([recs])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=1, max_configs=1 << 22, init_value=init)
    assert j["verdict"][0] != -1
    cut = None if j["verdict"][0] == 1 else int(j["fail_prefix_end"][0]) - 1
    return recs, init, cut, cref.search(recs, cut, (0, init))


@functools.lru_cache(maxsize=None)
def batch_ref(name):
    """Per key of batch A / B / C the restatement's Result at the oracle's cut."""
    keys, init = batch(name)
    j = jitc(name)
    out = []
    for k, recs in enumerate(keys):
        cut = None if j["verdict"][k] == 1 else int(j["fail_prefix_end"][k]) - 1
        out.append(cref.search(recs, cut, (0, init)))
    return out


# ------------------------------------------------------------------ CPU tests

def test_symbols_and_constants():
    L = abi.lib()
    assert L.lc_last_counted_witness_stats is not None  # (the feature's marker)
    assert L.lc_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "lincheck.h")).read()
    m = re.search(r"#define\s+LC_FLAG_COUNTED_WITNESS\s+(\d+)", hdr)
    assert m and int(m.group(1)) == abi.LC_FLAG_COUNTED_WITNESS == 128
    hdr = open(os.path.join(ROOT, "include", "lincheck_witness.h")).read()
    for name, cls in (("lc_counted_witness_stats", abi.LcCountedWitnessStats),
                      ("lc_witness_stats", abi.LcWitnessStats)):
        fields = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        assert re.findall(r"(?:int64_t|double)\s+(\w+);", fields) == [f for f, _ in cls._fields_]
    assert [f for f, _ in abi.LcCountedWitnessStats._fields_] == \
        ["n_keys", "n_found", "n_budget", "n_unfit", "nodes", "cache_hits", "kernel_ms"]
    assert [f for f, _ in abi.LcWitnessStats._fields_] == \
        ["n_keys", "n_found", "n_budget", "n_window", "nodes", "cache_hits", "kernel_ms"]


@pytest.mark.parametrize("model", list(MODELS))
def test_restatement_against_the_definition(model):
    """An order exactly when the exhaustive search has one; at the failing
    prefix one for the cut and none at the failing return."""
    init = MODELS[model][1]
    kinds, classes = set(), set()
    for recs, kind, cut, _ in searched(model):
        whole = cref.search(recs, None, (0, init))
        assert (whole.status == "found") == (kind == FULL), recs
        r = whole
        if kind == PREFIX:
            assert whole.status == "none", (recs, whole)
            r = cref.search(recs, cut, (0, init))
            assert cref.search(recs, cut + 1, (0, init)).status == "none", recs
        assert r.status == "found", (recs, cut)
        assert both(recs, r.ranks, kind, cut, init), (recs, r.ranks, kind, cut)
        kinds.add(kind)
        members = {}
        for x in recs:
            if x[0] in (W, C) and x[5] == INF:
                members[tuple(x[:4])] = members.get(tuple(x[:4]), 0) + 1
        classes.update(members.values())
    assert kinds == {FULL, PREFIX} and {1, 2} <= classes


def test_inputs_stay_inside_the_cap():
    """Every key the GPU tests demand a witness for: at most 4,096 steps in
    the restatement (a sixteenth of the device's cap) and fewer than 2,048
    dead ends stored (the cache holds 20,480)."""
    worst = {}
    for name in HAND:
        r = hand_ref(name)[3]
        assert r.status == "found" and r.steps <= MAX_STEPS and r.stored < MAX_STORED, (name, r[2:])
        worst[name] = r.steps
    for name in "ABC":
        rs = batch_ref(name)
        for k, r in enumerate(rs):
            assert r.status == "found" and r.steps <= MAX_STEPS and r.stored < MAX_STORED, (name, k, r[2:])
        worst[name] = max(r.steps for r in rs)
    print("steps at most:", worst)
    n_invalid = {name: int((jitc(name)["verdict"] == 0).sum()) for name in "ABC"}
    assert n_invalid["A"] > 0 and n_invalid["B"] > 0  # both verdicts occur
    # what the hand keys are there for
    assert hand_ref("overflow70")[3].steps == 4
    d = hand_ref("dead-end")[3]
    assert d.steps > 5 and d.hits > 0 and sum(1 for x in d.ranks if x >= 0) == 5
    assert any(r.hits > 0 for r in batch_ref("A"))


def test_checker_passes_the_flag():
    flag = lambda **kw: checker.RegisterChecker(**kw)._flags() & abi.LC_FLAG_COUNTED_WITNESS
    assert flag(search_witness=True) == 128
    assert flag(search_witness=True, counted_witness=True) == 128
    assert flag(search_witness=False) == 0 and flag() == 0
    assert flag(search_witness=True, counted_witness=False) == 0
    assert flag(search_witness=False, counted_witness=True) == 0


def overflow70_history():
    h = [{"type": "invoke", "f": "acquire", "process": i, "value": None} for i in range(70)]
    for p, f in ((70, "acquire"), (71, "release"), (72, "release")):
        h.append({"type": "invoke", "f": f, "process": p, "value": None})
        h.append({"type": "ok", "f": f, "process": p, "value": None})
    return h


def test_history_packs_to_the_key():
    from jepsen.etcd_amd import history as H
    _, ops, off, _ = H.pack(overflow70_history(), model="mutex", independent=False)
    assert ops.tolist() == overflow70() and off.tolist() == [0, 73]


# ------------------------------------------------------------------ GPU tests

class Run:
    """A batch checked with LC_FLAG_SEARCH_WITNESS alone (res0 / wit0 / kind0
    / st0) and with LC_FLAG_COUNTED_WITNESS too (res / wit / kind / st / cst)."""


def stats_of(st):
    return {k: v for k, v in st.items() if k != "kernel_ms"}


def run(ctx, keys, init, flags=CC, timed=False, **kw):
    """Both calls; the new flag must move nothing the first call gave.  (With
    `timed` the calls run under a time budget: which keys the tiers and the
    first stage finish then depends on the clock, in either call, so only
    the keys both calls decided are compared, and each call's own counts.)"""
    r = Run()
    r.init = init
    r.ops, r.off = pack_keys([list(map(list, k)) for k in keys])
    _, r.res0, r.wit0, r.kind0 = ctx.check(
        r.ops, r.off, abi.default_opts(init_value=init, flags=flags | SW, **kw), witness=True)
    r.st0 = ctx.last_witness_stats()
    assert not any(ctx.last_counted_witness_stats().values())  # (all zero without the flag)
    _, r.res, r.wit, r.kind = ctx.check(
        r.ops, r.off, abi.default_opts(init_value=init, flags=flags | SW | CW, **kw), witness=True)
    r.st, r.cst = ctx.last_witness_stats(), ctx.last_counted_witness_stats()
    assert r.cst["n_keys"] == r.cst["n_found"] + r.cst["n_budget"] + r.cst["n_unfit"]
    assert r.cst["n_keys"] == r.st["n_window"]
    assert r.st["n_keys"] == r.st["n_found"] + r.st["n_budget"] + r.st["n_window"]
    if timed:
        both_decided = (r.res["verdict"] != -1) & (r.res0["verdict"] != -1)
        assert r.res[both_decided].tobytes() == r.res0[both_decided].tobytes()
    else:
        assert r.res.tobytes() == r.res0.tobytes()
        assert stats_of(r.st) == stats_of(r.st0)
        for k in np.nonzero(r.kind0)[0]:
            assert r.kind[k] == r.kind0[k], k
            assert r.wit[r.off[k]:r.off[k + 1]].tobytes() == r.wit0[r.off[k]:r.off[k + 1]].tobytes(), k
    return r


def certify(r, k):
    """Key k's kind matches its verdict and its order is certified at its cut
    by both certifiers.  Returns the key's ranks."""
    v, kind = int(r.res["verdict"][k]), int(r.kind[k])
    assert kind == (FULL if v == 1 else PREFIX), (k, v, kind)
    recs, w = r.ops[r.off[k]:r.off[k + 1]], r.wit[r.off[k]:r.off[k + 1]]
    assert both(recs, w, kind, int(r.res["fail_prefix_end"][k]) - 1, r.init), (k, recs.tolist(), w.tolist())
    return w


def untouched(r):
    assert (r.kind == r.kind0).all() and r.wit.tobytes() == r.wit0.tobytes()


def hand(ctx, name):
    """A hand key alone in its call; the device's step count is the
    restatement's (the new stage's, or the first stage's when that found it)."""
    recs, init, cut, ref = hand_ref(name)
    r = run(ctx, [recs], init)
    assert int(r.res["verdict"][0]) == (1 if cut is None else 0), name
    if cut is not None:
        assert int(r.res["fail_prefix_end"][0]) - 1 == cut, name
    w = certify(r, 0)
    ranked = sorted((i for i in range(len(w)) if w[i] >= 0), key=lambda i: w[i])
    return r, recs, ranked, ref


@pytest.mark.gpu
def test_window_overflow_key_gets_its_order(ctx):
    """The assertion that fails without the feature: the key of
    test_search_witness.py::test_window_overflow ends with kind FULL."""
    r, recs, ranked, ref = hand(ctx, "overflow70")
    assert r.kind.tolist() == [FULL] and r.kind0.tolist() == [0]
    assert (r.st0["n_keys"], r.st0["n_found"], r.st0["n_window"]) == (1, 0, 1)
    assert (r.cst["n_keys"], r.cst["n_found"], r.cst["nodes"]) == (1, 1, 4) and ref.steps == 4
    assert len(ranked) == 4 and sorted(ranked) == [0, 70, 71, 72]  # the first acquire called
    assert r.cst["kernel_ms"] > 0


@pytest.mark.gpu
def test_invalid_hand_keys(ctx):
    for name, n_ranked in (("k1", 1), ("k2", 6)):
        r, recs, ranked, ref = hand(ctx, name)
        assert r.kind.tolist() == [PREFIX] and len(ranked) == n_ranked, (name, ranked)
        assert (r.cst["n_found"], r.cst["nodes"]) == (1, ref.steps), (name, r.cst, ref[2:])
        crashed = [i for i in ranked if recs[i][5] == INF]
        for i in crashed:  # the first called of their class
            earlier = [j for j in range(i) if recs[j][:4] == recs[i][:4] and recs[j][5] == INF]
            assert all(j in crashed for j in earlier), (name, i)
        assert len(crashed) == (0 if name == "k1" else 3)  # (k1: the :ok acquire alone)


@pytest.mark.gpu
def test_dead_end_with_counts(ctx):
    r, recs, ranked, ref = hand(ctx, "dead-end")
    print("dead end with counts:", r.cst, ref[2:])
    assert r.kind.tolist() == [FULL] and len(ranked) == 5
    assert r.cst["nodes"] > 5 and r.cst["cache_hits"] > 0
    assert (r.cst["nodes"], r.cst["cache_hits"]) == (ref.steps, ref.hits)


@pytest.mark.gpu
@pytest.mark.parametrize("m", [63, 64, 65, 127, 128])
def test_field_width_edges(ctx, m):
    for extra in (False, True):
        r, recs, ranked, ref = hand(ctx, "width-%d%s" % (m, "+1" if extra else ""))
        assert r.kind.tolist() == [PREFIX if extra else FULL] and len(ranked) == 2 * m
        crashed = [i for i in ranked if i < m]
        assert crashed == list(range(m))  # in call order
        if m == 63:  # 63 crashed ops and one release open: the first stage's
            assert r.cst["n_keys"] == 0 and r.kind0.tolist() == r.kind.tolist()
            assert r.st["nodes"] == ref.steps
        else:
            assert r.kind0.tolist() == [0]
            assert (r.cst["n_keys"], r.cst["n_found"], r.cst["nodes"]) == (1, 1, ref.steps)


@pytest.mark.gpu
def test_class_astride_the_chunk_boundary(ctx):
    r, recs, ranked, ref = hand(ctx, "astride")
    assert (r.cst["n_keys"], r.cst["n_found"], r.cst["nodes"]) == (1, 1, ref.steps)
    assert len(recs) >= 70 and any(i >= 64 and recs[i][5] == INF for i in ranked)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_batches(ctx, name):
    keys, init = batch(name)
    r = run(ctx, keys, init)
    ref = batch_ref(name)
    assert (r.res["verdict"] != -1).all()
    for k in range(len(keys)):
        certify(r, k)
    took = [k for k in range(len(keys)) if r.kind0[k] == 0]  # (every key is decided)
    print("batch", name, r.st, r.cst)
    assert r.cst["n_keys"] == len(took) == r.st["n_window"] >= 1
    assert (r.cst["n_found"], r.cst["n_budget"], r.cst["n_unfit"]) == (len(took), 0, 0)
    assert r.cst["nodes"] == sum(ref[k].steps for k in took)
    assert r.cst["cache_hits"] == sum(ref[k].hits for k in took)


@pytest.mark.gpu
def test_keys_that_do_not_fit_stay_as_they_were(ctx):
    """Batch D (21-26 classes per key), a decided key of 17 classes, and one
    with more :ok ops open than its layout has slots."""
    keys, init = batch("D")
    r = run(ctx, keys, init)
    assert r.cst["n_unfit"] == r.cst["n_keys"] and r.cst["n_found"] == 0
    untouched(r)
    for make in (many_classes_key, many_open_key):
        r = run(ctx, [make()], N)
        print(make.__name__, r.res.tolist(), r.kind0.tolist(), r.st, r.cst)
        assert r.res["verdict"][0] == 1, make.__name__
        assert (r.st["n_window"], r.cst["n_keys"], r.cst["n_unfit"]) == (1, 1, 1), make.__name__
        assert r.cst["nodes"] == 0
        untouched(r)


@pytest.mark.gpu
def test_flag_is_inert_alone(ctx):
    ops, off, init = packed("C")
    _, a, wa, ka = ctx.check(ops, off, abi.default_opts(init_value=init, flags=CC), witness=True)
    _, b, wb, kb = ctx.check(ops, off, abi.default_opts(init_value=init, flags=CC | CW), witness=True)
    assert a.tobytes() == b.tobytes() and wa.tobytes() == wb.tobytes() and ka.tobytes() == kb.tobytes()
    assert not any(ctx.last_counted_witness_stats().values())
    assert not any(stats_of(ctx.last_witness_stats()).values())


@pytest.mark.gpu
def test_budgets(ctx):
    """max_configs_per_key bounds the counted stage's steps too.  The 70-acquire
    key with 20 :ok acquire/release pairs appended never reaches a witness
    stage under max_configs_per_key=8: every mutex op linearized is a
    configuration of the tiers' search as well, so the counted tier itself
    stops at the budget (configs_explored 9, :unknown) — the call returns 0,
    the key keeps kind 0 and no stage counts it.  A key the tiers do decide
    within 8 configurations while its order needs more steps has reads, which
    the tiers take in their read closure: read_budget_key, n_budget == 1."""
    r = run(ctx, [budget_key()], FREE, max_configs_per_key=8)
    print("budget 8:", r.res.tolist(), r.st, r.cst)
    assert r.res["verdict"][0] == -1 and r.res["reason"][0] == abi.LC_REASON_CONFIG_BUDGET
    assert r.kind.tolist() == [0] and r.cst["n_keys"] == 0
    untouched(r)
    r = run(ctx, [read_budget_key()], N, max_configs_per_key=8)
    print("budget 8, reads:", r.res.tolist(), r.st, r.cst)
    assert r.res["verdict"][0] == 1
    assert (r.cst["n_keys"], r.cst["n_budget"], r.cst["n_found"]) == (1, 1, 0)
    assert r.kind.tolist() == [0]
    untouched(r)
    r = run(ctx, [read_budget_key()], N, max_configs_per_key=16)  # 13 steps
    assert (r.cst["n_found"], r.cst["nodes"]) == (1, 13) and r.kind.tolist() == [FULL]
    certify(r, 0)
    # under a time budget the call still returns 0 and counts every key
    keys, init = batch("A")
    r = run(ctx, keys, init, timed=True, time_budget_ms=1)
    print("time budget 1 ms:", r.st, r.cst)
    for k in range(len(keys)):
        if r.kind[k] in (FULL, PREFIX):
            certify(r, k)


@pytest.mark.gpu
def test_device_resident(ctx):
    import torch
    keys, init = batch("C")
    r = run(ctx, keys, init)
    dev = torch.device("cuda:0")
    n = len(r.off) - 1
    d_ops, d_off = torch.from_numpy(r.ops).to(dev), torch.from_numpy(r.off).to(dev)
    d_out = torch.zeros(n * abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_wit = torch.full((len(r.ops),), -3, dtype=torch.int32, device=dev)
    d_kind = torch.full((n,), -3, dtype=torch.int32, device=dev)
    ctx.check_device(d_ops.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(),
                     opts=abi.default_opts(init_value=init, flags=CC | SW | CW),
                     d_witness=d_wit.data_ptr(), d_witness_kind=d_kind.data_ptr())
    torch.cuda.synchronize()
    cst = ctx.last_counted_witness_stats()
    assert d_out.cpu().numpy().tobytes() == r.res.tobytes()
    assert (d_kind.cpu().numpy() == r.kind).all() and (d_wit.cpu().numpy() == r.wit).all()
    assert stats_of(cst) == stats_of(r.cst) and cst["n_found"] >= 8


@pytest.mark.gpu
def test_two_device_contexts_on_one_gpu(ctx, monkeypatch):
    keys, init = batch("C")
    one = run(ctx, keys, init)
    monkeypatch.setenv("LC_VIRTUAL_DEVICES", "2")
    with abi.Context(1) as two_ctx:
        two = run(two_ctx, keys, init)
        assert two_ctx.stats()["n_devices"] == 2
        shares = [d["key_end"] - d["key_begin"] for d in two_ctx.device_stats()]
    assert min(shares) >= 1
    assert two.res.tobytes() == one.res.tobytes() and (two.kind == one.kind).all()
    assert stats_of(two.cst) == stats_of(one.cst)  # summed over the devices
    for a, b in zip(np.cumsum([0] + shares)[:-1], np.cumsum(shares)):  # both ranges witnessed
        assert ((two.kind[a:b] >= FULL) & (two.kind0[a:b] == 0)).sum() > 0
    for k in range(len(keys)):
        certify(two, k)


@pytest.mark.gpu
def test_checker():
    cs = [checker.linearizable(checker.Mutex(), device_mask=1, search_witness=True),
          checker.linearizable(checker.Mutex(), device_mask=1, search_witness=True, counted_witness=False)]
    try:
        on, off = (c.check({}, overflow70_history()) for c in cs)
    finally:
        for c in cs:
            c.close()
    assert on["valid?"] is True and off["valid?"] is True
    assert len(on["linearization"]) == 4 and on["witness-certified"] is True
    assert "linearization" not in off and "witness-certified" not in off
    extra = {"linearization", "witness-certified"}
    assert {k: v for k, v in on.items() if k not in extra} == off
