"""tests/search_ref.py (the frontier search restated from its specification)
and tests/planted_search.py (deterministic keys on the search tiers' edges),
pinned on the CPU:

* search_ref equals the oracle's JITC search in all five result fields on
  every plant and on random histories, and plain JIT's verdicts and fail ops
  wherever plain JIT finishes;
* the oracle decides every plant, with the verdict and the fail op the
  builders claim by construction;
* every edge is hit exactly: the quantities search_ref reports (set sizes per
  general-path return, window slots, general-path returns, record counts)
  are the ones planted_search's tables name — E - 1, E and E + 1.

tests/test_gpu_search_edges.py runs the same groups through every search
path of the device and takes its expectations from reference() below."""
import functools
import random

import numpy as np
import pytest

import oracle
import planted_search as ps
import search_ref
from helpers import INF, N, R, W, pack_keys, random_casreg, random_tiny

FIELDS = ("verdict", "fail_op", "fail_prefix_end", "configs_explored", "max_frontier")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(plants, ops, key_off, oracle JITC results, search_ref results) of one
    group, long and short keys alternating; computed once, left unchanged."""
    pls = ps.group(name)
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8)
    return pls, ops, off, j, tuple(search_ref.check(pl.recs) for pl in pls)


def _five(res):
    return tuple(int(v) for v in res[:5])


@pytest.mark.parametrize("name", ps.GROUPS)
def test_reference_equals_oracle_on_every_plant(name):
    pls, ops, off, j, refs = reference(name)
    assert len({pl.tag for pl in pls}) == len(pls)
    for k, (pl, r) in enumerate(zip(pls, refs)):
        assert j["verdict"][k] != -1, pl.tag  # the oracle decides every plant
        assert _five(r) == tuple(int(j[f][k]) for f in FIELDS), pl.tag
        assert (r.verdict, r.fail_op) == (pl.verdict, pl.fail_op), pl.tag
        assert all(rec[3] == N for rec in pl.recs), pl.tag  # version-less


@pytest.mark.parametrize("name", ps.GROUPS)
def test_verdicts_equal_plain_jit_where_it_finishes(name):
    """knossos.linear without any reduction, under a budget: the fans' 2^k
    subsets of crashed writes end most large plants :unknown there."""
    pls, ops, off, j, _ = reference(name)
    _, plain = oracle.check(ops, off, algo=oracle.JIT, n_threads=8, max_configs=100000)
    done = plain["verdict"] != -1
    assert (plain["verdict"][done] == j["verdict"][done]).all()
    assert (plain["fail_op"][done] == j["fail_op"][done]).all()
    if name in ("small", "epochs", "values"):
        assert done.sum() >= len(pls) // 2, (name, int(done.sum()), len(pls))


def test_reference_equals_oracle_on_random_histories():
    rng = random.Random(20250)
    keys = []
    while len(keys) < 2400:
        n = rng.randrange(1, 14)
        recs = random_tiny(rng, n) if len(keys) % 2 else random_casreg(rng, n, p_info=0.4)
        if recs:
            keys.append(recs)
    ops, off = pack_keys(keys)
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8)
    _, plain = oracle.check(ops, off, algo=oracle.JIT, n_threads=8)
    assert (plain["verdict"] != -1).all()
    n_general = 0
    for k, recs in enumerate(keys):
        r = search_ref.check(recs)
        assert _five(r) == tuple(int(j[f][k]) for f in FIELDS), (k, recs)
        assert (r.verdict, r.fail_op) == (plain["verdict"][k], plain["fail_op"][k]), (k, recs)
        n_general += bool(r.returns)
    assert (j["verdict"] == 0).sum() > 200 and n_general > 300, n_general


def _ref_of(name, tag):
    pls, _, _, _, refs = reference(name)
    return next(r for pl, r in zip(pls, refs) if pl.tag == tag)


@pytest.mark.parametrize("name,table,which", [
    ("lds", "LDS_EDGE", 0), ("pool", "POOL_EDGE", 1), ("rung", "RUNG_EDGE", 0),
    ("pool", "POOL_NF", 2), ("dump", "DUMP_FANS", 2)])
def test_fans_hit_their_sizes_exactly(name, table, which):
    """which: 0 largest max(|W|, |R|), 1 largest |R| + |W|, 2 largest |F|
    entering a general-path return — of search_ref, for every row.  (POOL_NF:
    the second fan's X is entered with exactly that many; the read after it
    with twice as many.)"""
    rows = getattr(ps, table)
    for row in rows:
        q, pl = row[0], ps.build(row)
        ref = _ref_of(name, pl.tag)
        if table == "POOL_NF":
            assert [n_f for n_f, _, _ in ref.returns] == [1, q, 2 * q], (table, pl.tag)
        else:
            assert search_ref.sizes(ref)[which] == q, (table, pl.tag)
    assert set(ps.EDGES[table]) <= {row[0] for row in rows}, table


def test_pure_fan_formulas():
    """|R| = prod(c_i + 1), |W| = 1 + sum c_i prod_{j != i}(c_j + 1), and the
    largest frontiers the design records for four fans."""
    for classes, mf in (((7, 8), 72), ((5, 11), 72), ((1, 4, 5), 60), ((8, 8), 81), ((2, 3, 4), 60)):
        r = search_ref.check(ps.fan(classes).recs)
        n_r = int(np.prod([c + 1 for c in classes]))
        n_w = 1 + sum(c * n_r // (c + 1) for c in classes)
        assert r.returns[0] == (1, n_w, n_r) and r.max_frontier == n_r == mf
        x = search_ref.check(ps.fan(classes, closer="x").recs)
        assert x.returns == [(1, n_w, 0)] and x.verdict == 0
        rd = search_ref.check(ps.fan(classes, closer="read").recs)
        assert rd.returns[0] == (1, n_w, n_r) and rd.returns[1][0] == n_r and rd.returns[1][2] == 0


def test_frontier_one_two_one():
    for classes, sizes in (((1,), [2, 1]), ((1, 1), [4, 2, 1])):
        for good in (True, False):
            r = _ref_of("small", ps.one_two_one(classes, good).tag)
            # the lone configuration branches, the reads collapse the frontier
            assert [n_r for _, _, n_r in r.returns] == sizes and r.returns[0][0] == 1
            # nothing is on the general path after the collapse: the last
            # reads and the write run on the lone configuration
            assert r.max_frontier == sizes[0] and r.slots_max == len(classes) + 1


def test_epoch_plants_general_returns():
    pls, _, _, _, refs = reference("epochs")
    counts = sorted(len(r.returns) for r in refs)
    assert sorted(set(counts)) == [254, 255, 256, 257, 511], counts
    for pl, r in zip(pls, refs):
        assert r.max_frontier == 4 and all(n_f <= 4 for n_f, _, _ in r.returns), pl.tag
    assert {pl.verdict for pl in pls} == {0, 1}


def test_window_plants_slots():
    want = {("plain", 63): 63, ("plain", 64): 64, ("reads", 64): 64, ("reuse", 64): 64}
    for (variant, slots), occ in want.items():
        r = _ref_of("small", ps.window(slots, variant).tag)
        assert r.slots_max == occ and not r.overflow, (variant, slots)
    pls, _, _, _, refs = reference("window65")
    assert len(pls) >= 2
    for pl, r in zip(pls, refs):
        assert r.slots_max == 65 and r.overflow, pl.tag
    # "reads": no return is on the general path, the reads on top of the full
    # window take no slot; "reuse": the slot of the retired write is taken again
    assert _ref_of("small", ps.window(64, "reads").tag).returns == []
    recs = ps.window(64, "reuse").recs
    y = next(i for i, rec in enumerate(recs) if rec[0] == W and rec[1] == 2)
    rd = next(i for i, rec in enumerate(recs) if rec[0] == R and rec[1] == 2)
    assert recs[rd][5] < recs[y][5] != INF  # retired by the read's return, before its own


def test_chunked_layout():
    seen = set()
    pls, _, _, _, refs = reference("small")
    for pl, r in zip(pls, refs):
        if pl.family != "chunked":
            continue
        n = len(pl.recs)
        seen.add(n)
        for b in range(64, n + 1, 64):
            recs = pl.recs
            # the fan is open from record b-6 on; X returns as record b-2; the
            # read called as record b-1 is open across the reload
            assert all(recs[i][5] == INF and recs[i][0] == W for i in range(b - 6, b - 2))
            x, r1 = recs[b - 2], recs[b - 1]
            assert x[0] == W and x[5] == x[4] + 1 and r1[0] == R
            assert r1[5] == r1[4] + (2 if " cf=1 " in pl.tag else 1)
            if n > b:  # the first event after the reload: r1's return, or record b's call
                assert (recs[b][4] < r1[5]) == (" cf=1 " in pl.tag)
            if pl.verdict == 0 and b == n // 64 * 64:
                assert r.fail_op == b - 1
        # the frontier is in a region across every reload: 9 configurations
        assert r.max_frontier == 9
    assert seen == set(ps.CHUNKED_N)


def test_value_plants_straddle_the_table():
    pls, _, _, _, refs = reference("small")
    sets = set()
    for pl, r in zip(pls, refs):
        if pl.family != "values":
            continue
        ids = {rec[1] for rec in pl.recs if rec[0] != R and rec[5] == INF}
        sets.add(tuple(sorted(ids)))
        assert search_ref.sizes(r)[0] <= 200, pl.tag
    for want in ps.VALUE_SETS:
        assert tuple(sorted(want)) in sets
    mixed = [s for s in sets if len(s) >= 4 and min(s) < 15 <= max(s)]
    assert mixed
    # one 64-configuration batch of the mixed fan holds both kinds of lane
    r = _ref_of("small", ps.values(*ps.MIXED_VALUES).tag)
    assert search_ref.sizes(r)[0] >= 64
