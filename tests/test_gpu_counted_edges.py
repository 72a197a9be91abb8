"""The three counted kernels — counted_tier_kernel (LC_FLAG_COUNTED_CLASSES),
counted_frontier_kernel (lc_check_frontiers_counted) and
witness_counted_kernel (LC_FLAG_COUNTED_WITNESS) — on tests/planted_counted.py's
keys: member counts on either side of every field width, a full field beside a
stepped one, 1 .. 17 classes, 63 / 64 field bits, exactly `slots` ops open,
classes astride the 64-record chunks, a pending :ok member of a class's tuple,
counts carried between the lone configuration and the frontier, sets on either
side of the first capacity's 2^14, value ids around the legality table.

Every key of every batch, no mask: the six result fields equal the CPU
oracle's JITC search, the frontiers equal tests/counted_ref.py's with every
pending list whole, the orders are certified and counted_order_ref's steps
are the device's.  Routing is asserted from the references, never from the
device's own output (tests/test_planted_counted.py pins the references, the
plants and the oracle to each other)."""
import ctypes
import functools

import numpy as np
import pytest

import counted_ref as cr
import planted_counted as pc
from helpers import INF, N, pack_keys
from jepsen.etcd_amd import abi
from test_planted_counted import frontier_at, order_of, reference, stops_of
from test_search_witness import both

pytestmark = pytest.mark.gpu

FIELDS = ("verdict", "reason", "fail_op", "fail_prefix_end", "configs_explored", "max_frontier")
CC, SW, CW = abi.LC_FLAG_COUNTED_CLASSES, abi.LC_FLAG_SEARCH_WITNESS, abi.LC_FLAG_COUNTED_WITNESS
OVERFLOW, BUDGET = abi.LC_REASON_WINDOW_OVERFLOW, abi.LC_REASON_CONFIG_BUDGET
FULL, PREFIX = 3, 4
BATCHES = ("small+direct", "ladders", "rung")


@functools.lru_cache(maxsize=None)
def batch(name):
    """(plants, ops, key_off, expected rows where the counted search decides,
    decided, routed) of one batch: `routed` — the slot tiers' window
    overflows — and `decided` come from counted_ref and search_ref."""
    refs = [reference(part) for part in name.split("+")]
    pls = [pl for ref in refs for pl in ref.plants]
    counted = [c for ref in refs for c in ref.counted]
    search = [s for ref in refs for s in ref.search]
    jitc = np.concatenate([ref.jitc for ref in refs])
    ops, off = pack_keys([pl.recs for pl in pls])
    want = np.zeros(len(pls), dtype=[(f, np.int64) for f in FIELDS])
    for f in FIELDS:
        if f != "reason":
            want[f] = jitc[f]
    want["reason"] = np.where(jitc["verdict"] == 1, 0, abi.LC_REASON_NONLINEARIZABLE)
    routed = np.array([bool(c.window64 or s.overflow) for c, s in zip(counted, search)])
    decided = np.array([c.verdict != cr.UNKNOWN for c in counted])
    return pls, ops, off, want, decided, routed


def assert_rows(pls, got, want, keys, what):
    for f in FIELDS:
        bad = [k for k in keys if int(got[f][k]) != int(want[f][k])]
        assert not bad, (what, f, [(pls[k].tag, int(got[f][k]), int(want[f][k])) for k in bad[:8]])


@pytest.mark.parametrize("by_value", ["1", "0"])
@pytest.mark.parametrize("name", BATCHES)
def test_lc_check_equals_the_oracle(ctx, monkeypatch, name, by_value):
    pls, ops, off, want, decided, routed = batch(name)
    monkeypatch.setenv("LC_COUNTED_BY_VALUE", by_value)
    every = range(len(pls))
    _, plain = ctx.check(ops, off)
    assert ctx.counted_stats()["n_keys"] == 0
    # without the flag: the routed keys are :unknown, the others decided
    bad = [pls[k].tag for k in every
           if ((plain["verdict"][k], plain["reason"][k]) == (abi.LC_UNKNOWN, OVERFLOW)) != routed[k]]
    assert not bad, bad[:8]
    assert_rows(pls, plain, want, np.nonzero(~routed)[0], (name, "plain"))
    _, got = ctx.check(ops, off, abi.default_opts(flags=CC))
    st = ctx.counted_stats()
    assert_rows(pls, got, want, np.nonzero(decided | ~routed)[0], (name, "counted"))
    # a key beyond the layout, or with more ops open than slots: as the tiers left it
    left = np.nonzero(routed & ~decided)[0]
    assert_rows(pls, got, plain, left, (name, "left"))
    assert (st["n_keys"], st["n_decided"], st["n_unfit"]) == \
        (int(routed.sum()), int((routed & decided).sum()), len(left)), st
    if name != "rung":
        assert len(left) >= 2
    # the same keys as 24-byte records
    o32, base = abi.pack32(ops, off)
    _, got32 = ctx.check32(o32, off, base, abi.default_opts(flags=CC))
    assert_rows(pls, got32, got, every, (name, "lc_check32"))
    assert {k: v for k, v in ctx.counted_stats().items() if k != "kernel_ms"} == \
        {k: v for k, v in st.items() if k != "kernel_ms"}


def crashed_record(pl):
    return next(i for i, r in enumerate(pl.recs) if r[5] == INF)


@functools.lru_cache(maxsize=None)
def stop_batches(name):
    """Three stop arrays over one group: per plant its fail op, the :ok
    return that expands its largest set, one no-op return — and where a plant
    lacks one, a crashed record (not an :ok return: -1).  With each the
    frontiers counted_ref expects."""
    ref = reference(name)
    out = []
    for i in range(3):
        stops, want = [], []
        for k, (pl, c) in enumerate(zip(ref.plants, ref.counted)):
            ss = stops_of(pl, c) if c.verdict != cr.UNKNOWN else []
            if c.verdict == cr.UNKNOWN and i == 0:
                ss = [max(j for j, r in enumerate(pl.recs) if r[5] != INF)]
            if i < len(ss):
                stops.append(ss[i])
                want.append(frontier_at(name, k, ss[i]))
            else:
                stops.append(crashed_record(pl))
                want.append(None)
        out.append((np.array(stops, dtype=np.int64), want))
    return ref, out


@pytest.mark.parametrize("name", ["small", "direct", "noslot", "ladders", "rung"])
def test_frontiers_equal_the_reference(ctx, name):
    ref, batches = stop_batches(name)
    n_whole = n_beyond_64 = n_none = 0
    for stops, want in batches:
        sizes = [len(w) for w in want if w is not None]
        # (the rung fans' frontiers are compared whole one key per call: test_rung_frontiers_whole)
        rooms = (1, 10) if name == "rung" else (1, 10, max(sizes + [1]))
        for room in rooms:
            cfgs, totals = ctx.check_frontiers_counted(ref.ops, ref.off, stops, room)
            for k, pl in enumerate(ref.plants):
                what = (pl.tag, int(stops[k]), room)
                if want[k] is None:
                    assert cfgs[k] is None and int(totals[k]) == -1, what
                    n_none += 1
                    continue
                assert cfgs[k] is not None, what
                assert int(totals[k]) == len(want[k]), what + (int(totals[k]), len(want[k]))
                assert len(cfgs[k]) == min(room, len(want[k])) == len(set(cfgs[k])), what
                assert set(cfgs[k]) <= set(want[k]), what
                if room >= len(want[k]):
                    assert set(cfgs[k]) == set(want[k]), what
                    n_whole += 1
                    n_beyond_64 += any(len(p) > 64 for _, _, p in want[k])
    assert n_whole >= {"rung": 0, "noslot": 3}.get(name, 10) and n_none >= 1
    if name in ("small", "ladders"):
        assert n_beyond_64 >= 10  # pending lists the oracle cuts at 64, compared whole


N_RUNG = 2 * len(pc.RUNG_R + pc.RUNG_W)


@pytest.mark.parametrize("k", range(N_RUNG))
def test_rung_frontiers_whole(ctx, k):
    """One rung fan per call, room for its whole frontier: the frontier the
    read after the large return is entered with — (a + 1)(b + 1)
    configurations, 16,256 .. 16,512 of them around the first capacity, every
    one with its whole pending list — equals counted_ref's as a set.  The
    search that gets there holds a W set of 16,381 .. 32,768 configurations:
    on the first capacity, exactly filling it, and on the next."""
    ref = reference("rung")
    assert len(ref.plants) == N_RUNG
    pl, c = ref.plants[k], ref.counted[k]
    ops, off = pack_keys([pl.recs])
    stops = sorted(set(stops_of(pl, c)))
    assert stops
    largest = 0
    for stop in stops:
        want = frontier_at("rung", k, stop)
        assert want is not None
        cfgs, totals = ctx.check_frontiers_counted(ops, off, [stop], max(len(want), 1))
        assert int(totals[0]) == len(want) == len(cfgs[0]), (pl.tag, stop, int(totals[0]), len(want))
        assert len(set(cfgs[0])) == len(cfgs[0]) and set(cfgs[0]) == set(want), (pl.tag, stop)
        largest = max(largest, len(want))
    a, b = (int(x) for x in pl.tag.split("c=(")[1].split(")")[0].split(","))
    assert largest == (a + 1) * (b + 1), pl.tag  # |R| of the large return, whole


def test_frontier_buffers_stay_untouched_where_the_answer_is_minus_one(ctx):
    """Unfit plants, slot-overflow plants and stops that are no :ok return:
    n_out = -1, and neither the key's configurations nor the pending buffer
    beyond what the other keys' lists take are written."""
    pls = [pc.ladder(4, True, anchor=False), pc.class_count(17, False, anchor=False), pc.slots(58),
           pc.one_slot(2), pc.ladder(3, anchor=False), pc.nine_classes(128), pc.ladder(4, True, anchor=False)]
    stops = [len(pl.recs) - 1 for pl in pls]
    stops[4] = 0  # a crashed record
    ops, off = pack_keys([pl.recs for pl in pls])
    mx, n_keys = 8, len(pls)
    cfg = np.zeros(n_keys * mx, dtype=abi.COUNTED_CONFIG_DTYPE)
    cfg.view(np.uint8)[:] = 0x5A
    pend = np.full(mx * len(ops), -7, dtype=np.int64)
    n_out = np.zeros(n_keys, dtype=np.int32)
    tot = np.zeros(n_keys, dtype=np.int64)
    st = np.array(stops, dtype=np.int64)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    o = abi.default_opts()
    rc = abi.lib().lc_check_frontiers_counted(ctx._h, p(ops), p(off), n_keys, p(st), ctypes.byref(o),
                                              p(cfg), mx, p(n_out), p(tot), p(pend), len(pend))
    assert rc == 0, ctx.last_error()
    want = cr.check(pls[0].recs, stop=stops[0]).frontier
    assert n_out.tolist() == [len(want), -1, -1, -1, -1, -1, len(want)] and len(want) <= mx
    assert tot.tolist() == [len(want), -1, -1, -1, -1, -1, len(want)]
    raw = cfg.view(np.uint8).reshape(n_keys, -1)
    for k in range(1, 6):
        assert (raw[k] == 0x5A).all(), k
    used = sum(len(pd) for _, _, pd in want) * 2
    assert (pend != -7).sum() == used and used > 0


@pytest.mark.parametrize("name", ["small", "ladders", "rung"])
def test_counted_witness_orders(ctx, name):
    ref = reference(name)
    pls = list(ref.plants)
    if name == "small":
        pls.append(pc.witness_unfit())
    ops, off = pack_keys([pl.recs for pl in pls])
    n = len(ref.plants)
    decided = [c.verdict != cr.UNKNOWN for c in ref.counted] + [True] * (len(pls) - n)
    _, res, wit, kind = ctx.check(ops, off, abi.default_opts(flags=CC | SW | CW), witness=True)
    cst = ctx.last_counted_witness_stats()
    steps = hits = 0
    for k, pl in enumerate(pls):
        if k >= n or not decided[k]:  # beyond the layout: no order, kind NONE
            assert kind[k] == 0, pl.tag
            assert int(res["verdict"][k]) == (1 if k >= n else abi.LC_UNKNOWN), pl.tag
            continue
        v = int(res["verdict"][k])
        assert v == pl.verdict and kind[k] == (FULL if v == 1 else PREFIX), (pl.tag, v, int(kind[k]))
        recs, w = ops[off[k]:off[k + 1]], wit[off[k]:off[k + 1]]
        assert both(recs, w, int(kind[k]), int(res["fail_prefix_end"][k]) - 1, N), pl.tag
        cut, r = order_of(name, k)
        assert cut == (None if v == 1 else int(res["fail_prefix_end"][k]) - 1), pl.tag
        steps += r.steps
        hits += r.hits
    # every decided plant holds 65 crashed mutations open: the first stage's
    # window overflows, the counted stage takes it
    n_unfit = len(pls) - n
    assert (cst["n_keys"], cst["n_found"], cst["n_budget"], cst["n_unfit"]) == \
        (sum(decided), sum(decided) - n_unfit, 0, n_unfit), cst
    assert (cst["nodes"], cst["cache_hits"]) == (steps, hits), (cst, steps, hits)


@pytest.mark.parametrize("name", ["small", "ladders", "rung"])
def test_counted_witness_steps_key_for_key(ctx, name):
    """Every decided plant alone in its call (the stage's counts are per
    call): steps and cache hits are counted_order_ref's for that key, the
    cut is the one the reference searched at."""
    ref = reference(name)
    n_alone = 0
    for k, (pl, c) in enumerate(zip(ref.plants, ref.counted)):
        if c.verdict == cr.UNKNOWN:
            continue
        ops, off = pack_keys([pl.recs])
        _, res, wit, kind = ctx.check(ops, off, abi.default_opts(flags=CC | SW | CW), witness=True)
        cst = ctx.last_counted_witness_stats()
        cut, r = order_of(name, k)
        assert int(res["verdict"][0]) == pl.verdict, pl.tag
        assert cut == (None if pl.verdict else int(res["fail_prefix_end"][0]) - 1), pl.tag
        assert kind[0] == (FULL if pl.verdict else PREFIX), pl.tag
        assert (cst["n_keys"], cst["n_found"], cst["nodes"], cst["cache_hits"]) == \
            (1, 1, r.steps, r.hits), (pl.tag, cst, r.steps, r.hits)
        assert both(ops, wit, int(kind[0]), int(res["fail_prefix_end"][0]) - 1, N), pl.tag
        n_alone += 1
    assert n_alone == sum(c.verdict != cr.UNKNOWN for c in ref.counted) >= 10


def test_budget_at_the_references_count(ctx):
    """max_configs_per_key = E, one plant's configs_explored by counted_ref,
    decides it; E - 1 ends it LC_REASON_CONFIG_BUDGET and moves nothing else
    of the batch (one wavefront counts every configuration)."""
    pls = [pc.slots(57), pc.ladder(16), pc.pending_ok("after"), pc.ladder(8, True), pc.slots(58)]
    refs = [cr.check(pl.recs) for pl in pls]
    e = refs[1].configs_explored
    assert e == max(r.configs_explored for r in refs) and e > 100
    ops, off = pack_keys([pl.recs for pl in pls])
    _, free = ctx.check(ops, off, abi.default_opts(flags=CC))
    for k, r in enumerate(refs[:4]):
        assert tuple(int(free[f][k]) for f in FIELDS) == \
            (r.verdict, r.reason, r.fail_op, r.fail_prefix_end, r.configs_explored, r.max_frontier)
    assert (free["verdict"][4], free["reason"][4]) == (abi.LC_UNKNOWN, OVERFLOW)
    _, at = ctx.check(ops, off, abi.default_opts(flags=CC, max_configs_per_key=e))
    assert at.tobytes() == free.tobytes()
    _, below = ctx.check(ops, off, abi.default_opts(flags=CC, max_configs_per_key=e - 1))
    assert (below["verdict"][1], below["reason"][1]) == (abi.LC_UNKNOWN, BUDGET)
    others = [0, 2, 3, 4]
    assert below[others].tobytes() == free[others].tobytes()
