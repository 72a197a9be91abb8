"""tests/counted_ref.py (the counted-class search restated from its
specification) and tests/planted_counted.py (deterministic keys on the counted
kernels' edges), pinned on the CPU:

* counted_ref equals search_ref and the oracle's JITC search in verdict, fail
  op, prefix end, configurations explored and largest frontier on every plant
  it decides — the counts <-> slot-sets bijection DESIGN.md §4 claims — and
  its general-path returns have search_ref's set sizes;
* abi.counted_plan (the host planner the device shares counted.h with) equals
  counted_ref's layout in every field;
* every edge is hit exactly, by what counted_ref / search_ref report;
* every mutant of the rule differs from the rule on a plant of the family
  aimed at it;
* counted_ref's frontiers equal oracle.frontier as sets where the oracle
  lists pending sets whole (fewer than 64 ops);
* counted_order_ref finds an order on every fitting plant, order_ref
  certifies it.

tests/test_gpu_counted_edges.py runs the same groups through the three
counted kernels and takes its expectations from reference() below."""
import collections
import functools

import numpy as np
import pytest

import counted_order_ref
import counted_ref as cr
import oracle
import order_ref
import planted_counted as pc
import search_ref
from helpers import INF, C, N, R, W, pack_keys
from jepsen.etcd_amd import abi

FIVE = ("verdict", "fail_op", "fail_prefix_end", "configs_explored", "max_frontier")
Ref = collections.namedtuple("Ref", "plants ops off jitc counted search")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(plants, ops, key_off, oracle JITC results, counted_ref results,
    search_ref results) of one group; computed once, left unchanged."""
    pls = pc.group(name)
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8, max_configs=1 << 22)
    j.setflags(write=False)
    return Ref(pls, ops, off, j, tuple(cr.check(pl.recs) for pl in pls),
               tuple(search_ref.check(pl.recs) for pl in pls))


def every_plant():
    for name in pc.ALL_GROUPS:
        ref = reference(name)
        for k, pl in enumerate(ref.plants):
            yield name, k, pl, ref.counted[k], ref.search[k]


def plants_of(family):
    return [(pl, c, s) for _, _, pl, c, s in every_plant() if pl.family == family]


def by_tag(tag):
    return next((pl, c, s) for _, _, pl, c, s in every_plant() if pl.tag == tag)


def five(res):
    return tuple(int(getattr(res, f)) for f in FIVE)


@pytest.mark.parametrize("name", pc.ALL_GROUPS)
def test_reference_equals_search_ref_and_the_oracle(name):
    ref = reference(name)
    assert len({pl.tag for pl in ref.plants}) == len(ref.plants)
    n_decided = 0
    for k, pl in enumerate(ref.plants):
        c, s = ref.counted[k], ref.search[k]
        want = tuple(int(ref.jitc[f][k]) for f in FIVE)
        assert want[0] != -1, pl.tag  # the oracle decides every plant
        assert want[:2] == (pl.verdict, pl.fail_op), pl.tag
        assert tuple(int(v) for v in s[:5]) == want, pl.tag
        if c.verdict == cr.UNKNOWN:
            assert c.reason == cr.REASON_WINDOW_OVERFLOW and c.fail_op == -1, pl.tag
            continue
        n_decided += 1
        assert five(c) == want, pl.tag
        assert c.reason == (cr.REASON_NONE if pl.verdict else cr.REASON_NONLINEARIZABLE), pl.tag
        assert c.returns == s.returns, pl.tag
        # what the slot-per-op tiers hold open, from the counts: their window
        # overflows exactly where search_ref's does
        assert c.window64 == s.overflow, pl.tag
        if name in pc.GROUPS:
            assert c.window64, pl.tag  # lc_check hands the key to the counted tier
        if "far_version" not in pl.tag:
            assert all(rec[3] == N for rec in pl.recs), pl.tag
    assert n_decided >= len(ref.plants) - 6


def test_undecided_plants_are_the_unfit_and_the_overflowing_ones():
    undecided = {pl.tag: c for _, _, pl, c, _ in every_plant() if c.verdict == cr.UNKNOWN}
    unfit = {t for t, c in undecided.items() if not c.layout["fits"]}
    assert unfit == {pc.class_count(17, x).tag for x in (False, True)} | \
        {pc.class_count(17, False, anchor=False).tag} | \
        {pc.nine_classes(128, x).tag for x in (False, True)}
    assert set(undecided) - unfit == {pc.slots(58).tag, pc.one_slot(2).tag}


@pytest.mark.parametrize("name", pc.ALL_GROUPS)
def test_host_plan_equals_the_layout(name):
    ref = reference(name)
    for pl, c in zip(ref.plants, ref.counted):
        got = abi.counted_plan(np.array(pl.recs, dtype=np.int64).reshape(-1, 6))
        assert got == c.layout, pl.tag
        lay = c.layout
        assert lay["field_bits"] == sum(x["width"] for x in lay["classes"]) or lay["n_classes"] > 16
        for x in lay["classes"]:
            assert 2 ** (x["width"] - 1) <= x["members"] < 2 ** x["width"], pl.tag


ANCHOR_END = pc.ANCHOR  # where the anchor's records come first: 0 .. 64


def _writes_of(lay, value):
    return next(x for x in lay["classes"] if x["f"] == W and x["value"] == value)


def test_ladders_hit_every_width_edge():
    """The class of m crashed writes of 1: m members, floor(log2 m) + 1 bits
    — a power of two is the first count of its width — and a configuration
    per count in the frontier."""
    widths = {}
    for pl, c, _ in plants_of("ladder"):
        x = _writes_of(c.layout, 1)
        widths.setdefault(x["members"], set()).add(x["width"])
        assert c.max_frontier == x["members"] + 1, pl.tag
        rounds = sum(1 for r in pl.recs if r[0] == R)
        assert rounds == x["members"] + (0 if pl.verdict else 1), pl.tag
        if not pl.verdict:
            assert c.fail_op == len(pl.recs) - 1, pl.tag
    assert widths == {1: {1}, 2: {2}, 3: {2}, 4: {3}, 7: {3}, 8: {4}, 15: {4}, 16: {5}, 31: {5},
                      32: {6}, 63: {6}, 64: {7}, 65: {7}, 127: {7}, 128: {8}, 255: {8}, 256: {9}}
    assert set(widths) == set(pc.LADDER_M)
    direct = {_writes_of(c.layout, 1)["members"] for pl, c, _ in plants_of("ladder")
              if " anchor=0 " in pl.tag and c.layout["n_classes"] == 1 and len(pl.recs) < 65}
    assert direct == set(pc.DIRECT_M)


def test_neighbours_saturate_a_field_beside_a_stepped_one():
    """Driven field all ones (3 of 3, 7 of 7) or its top bit alone (4, 8);
    the stepped class of 4 right below it; first: the driven field ends at
    bit 63; last: the stepped field borders the slots.  At the last read's
    return every configuration holds both classes full."""
    seen = set()
    for pl, c, _ in plants_of("neighbours"):
        lay = c.layout
        d, s, b = (_writes_of(lay, v) for v in (1, 2, 3))
        assert (s["members"], s["width"], b["members"]) == (4, 3, 3), pl.tag
        assert d["shift"] == s["shift"] + s["width"], pl.tag  # the stepped field right below
        pos = pl.tag.split("pos=")[1].split()[0]
        if pos == "first":
            assert d["shift"] + d["width"] == 64, pl.tag
        elif pos == "last":
            assert s["shift"] == lay["slots"] == 64 - lay["field_bits"], pl.tag
        else:
            assert d["shift"] + d["width"] < 64 and s["shift"] > lay["slots"], pl.tag
        seen.add((d["members"], pos, pl.verdict))
        if pl.verdict:
            last = cr.check(pl.recs, stop=len(pl.recs) - 1)
            members = lambda v: [i for i, r in enumerate(pl.recs) if r[0] == W and r[1] == v and r[5] == INF]
            for _, _, pend in last.frontier:
                # one member of the stepped class left at the last read, none of the driven one
                assert len(set(pend) & set(members(2))) <= 1 and not set(pend) & set(members(1)), pl.tag
    assert seen == {(m, pos, v) for m in pc.NEIGHBOUR_M for pos in pc.NEIGHBOUR_POS for v in (0, 1)}
    assert {m + 1 & m for m in pc.NEIGHBOUR_M} == {0, 4, 8}  # all ones twice, a power of two twice


def test_class_counts_and_field_bits():
    n_classes, nine = set(), {}
    for pl, c, _ in plants_of("class_count"):
        lay = c.layout
        if "nine=" in pl.tag:
            nine[lay["field_bits"]] = (lay["n_classes"], lay["slots"], lay["fits"])
        else:
            n_classes.add((lay["n_classes"], lay["fits"]))
            if " anchor=0 " in pl.tag and lay["n_classes"] == 16:
                assert all(x["members"] == 1 for x in lay["classes"]), pl.tag
                assert (lay["field_bits"], lay["slots"]) == (16, 48), pl.tag
    assert n_classes == {(1, 1), (2, 1), (15, 1), (16, 1), (17, 0)}
    assert nine == {63: (9, 1, 1), 64: (9, 0, 0)}


def test_slot_plants_fill_the_window_exactly():
    got = {}
    for pl, c, _ in plants_of("slots"):
        got[pl.tag] = (c.layout["slots"], c.slots_used_max, c.verdict, c.reason)
    assert got[pc.slots(56).tag] == (57, 56, 1, 0)
    assert got[pc.slots(57).tag] == (57, 57, 1, 0)
    assert got[pc.slots(57, good=False).tag] == (57, 57, 0, 1)
    assert got[pc.slots(58).tag] == (57, 57, -1, cr.REASON_WINDOW_OVERFLOW)
    assert got[pc.one_slot(0).tag] == (1, 0, 1, 0)
    assert got[pc.one_slot(1).tag] == (1, 1, 1, 0)
    assert got[pc.one_slot(2).tag] == (1, 1, -1, cr.REASON_WINDOW_OVERFLOW)
    # reuse: 58 ops pass through 57 slots — the write of 3 is called with the
    # window full but for the slot the retired first write left
    for good in (True, False):
        pl = pc.slot_reuse(good)
        assert got[pl.tag][:2] == (57, 57) and got[pl.tag][2] == int(good)
        y = next(i for i, r in enumerate(pl.recs) if r[0] == W and r[1] == 3)
        first = next(i for i, r in enumerate(pl.recs) if r[0] == W and r[1] == 2)
        open_at_y = [i for i, r in enumerate(pl.recs)
                     if r[5] != INF and r[4] < pl.recs[y][4] < r[5]]
        assert len(open_at_y) == 56 and pl.recs[first][5] < pl.recs[y][4]
        # at y's return every write of 2 is retired: y is pending or linearized
        fr = cr.check(pl.recs, stop=y).frontier
        anchor = tuple(range(ANCHOR_END))
        assert sorted(p for _, _, p in fr) == [anchor, anchor + (y,)]


def test_chunk_plants_sit_on_the_reloads():
    firsts, astride, chunk_last, key_last = set(), set(), 0, 0
    for pl, c, _ in plants_of("chunks"):
        x = _writes_of(c.layout, 1)
        idx = [i for i, r in enumerate(pl.recs) if r[0] == W and r[1] == 1 and r[5] == INF]
        assert len(idx) == x["members"], pl.tag
        firsts.add(idx[0])
        astride |= {b for b in (64, 128) if b - 1 in idx and b in idx}
        chunk_last += any(i % 64 == 63 for i in idx)
        key_last += idx[-1] == len(pl.recs) - 1
        assert c.window64 and c.layout["n_classes"] == 2, pl.tag
        # a frontier of several configurations stands across every reload
        assert c.max_frontier >= 3, pl.tag
    assert {63, 64, 65} <= firsts and astride == {64, 128}
    assert chunk_last >= 6 and key_last >= 4


def test_pending_ok_member_return_times():
    whens = set()
    for pl, c, _ in plants_of("pending_ok"):
        y = next(i for i, r in enumerate(pl.recs) if r[0] == W and r[1] == 1 and r[5] != INF)
        crashed = [i for i, r in enumerate(pl.recs) if r[0] == W and r[1] == 1 and r[5] == INF]
        assert len(crashed) == 2 and y < crashed[0], pl.tag
        ret, calls = pl.recs[y][5], [pl.recs[i][4] for i in crashed]
        first_read = next(r for r in pl.recs if r[0] == R)
        when = ("before" if ret < calls[0] else "between" if ret < calls[1]
                else "after" if ret < first_read[4] else "late")
        assert " when=%s" % when in pl.tag, pl.tag
        whens.add(when)
        if when == "late":
            # deadline order puts Y before the crashed members, so the first
            # read of 1 puts Y into every configuration: retired before it returns
            assert y in c.noops and cr.check(pl.recs, stop=y).frontier == [], pl.tag
        else:
            assert y not in c.noops, pl.tag
    assert whens == set(pc.PENDING_WHEN)


def test_cas_plants_drive_each_class_to_its_count():
    tags = [pl.tag for pl, _, _ in plants_of("cas")]
    assert len(tags) == 12
    for n in (1, 2, 3, 4):
        pl, c, _ = by_tag(pc.cas_pair(n).tag)
        cas = [x for x in c.layout["classes"] if x["f"] == C and x["expected"] in (0, 1)]
        assert [(x["expected"], x["value"], x["members"]) for x in cas] == [(0, 1, n), (1, 0, n)]
        # at the last read (of 0) one CAS 1 -> 0 is left, and no CAS 0 -> 1
        last = cr.check(pl.recs, stop=len(pl.recs) - 1).frontier
        assert len(last) == 1
        left = [tuple(pl.recs[i][1:3]) for i in last[0][2] if pl.recs[i][2] in (0, 1)]
        assert left == [(0, 1)], (pl.tag, left)
    _, c, _ = by_tag(pc.cas_and_write().tag)
    assert [(x["f"], x["value"], x["members"]) for x in c.layout["classes"][1:]] == [(W, 1, 2), (C, 1, 2)]
    _, c, _ = by_tag(pc.cas_expected().tag)
    assert [(x["f"], x["value"], x["expected"]) for x in c.layout["classes"][1:]] == [(C, 1, 0), (C, 1, 2)]


def test_single_to_several_and_back_with_counts():
    for good in (True, False):
        pl, c, _ = by_tag(pc.single_several(good).tag)
        x = _writes_of(c.layout, 1)
        assert x["members"] == 4
        # the first general-path return is entered with one configuration —
        # whose count is 1: one member of the class is no longer pending
        assert c.returns[0][0] == 1
        members = [i for i, r in enumerate(pl.recs) if r[0] == W and r[1] == 1 and r[5] == INF]
        at = cr.check(pl.recs, stop=c.return_ops[0]).frontier
        assert len(at) == 1 and set(at[0][2]) & set(members) == set(members[1:3])
        # the third read's return leaves one configuration again, count 3:
        # at the next return it stands alone, version 5, no member pending
        reads = [i for i, r in enumerate(pl.recs) if r[0] == R]
        assert c.returns[c.return_ops.index(reads[2])][2] == 1
        w0 = next(i for i in range(reads[2] + 1, len(pl.recs)) if pl.recs[i][5] != INF)
        at = cr.check(pl.recs, stop=w0).frontier
        assert len(at) == 1 and at[0][:2] == (5, 1), at
        assert set(at[0][2]) & set(members) == (set(members[3:]) if good else set())
        # the last read: with the fourth member called it is served, else nothing is
        at = cr.check(pl.recs, stop=reads[-1]).frontier
        assert {frozenset(p) & frozenset(members) for _, _, p in at} == \
            ({frozenset(members[3:]), frozenset()} if good else {frozenset()}), at
        assert (c.verdict, c.fail_op) == ((1, -1) if good else (0, reads[-1]))
        assert (pl.recs[members[3]][4] < pl.recs[reads[-1]][4]) == good


def test_rung_fans_hit_the_first_capacity_exactly():
    """|R| = (a + 1)(b + 1) and |W| = 1 + a (b + 1) + b (a + 1) of the large
    return; a set of exactly 2^14 fits the first capacity (HbmStore::lim is
    cap with the full table, and counted_return_try gives up above it)."""
    for table, which in ((pc.RUNG_R, 2), (pc.RUNG_W, 1)):
        sizes = []
        for (a, b), q in table:
            for closer in ("valid", "read"):
                pl, c, s = by_tag(pc.rung((a, b), closer).tag)
                assert c.returns[0] == s.returns[0] == \
                    (1, 1 + a * (b + 1) + b * (a + 1), (a + 1) * (b + 1)), pl.tag
                assert c.returns[0][which] == q, pl.tag
                if closer == "valid" and which == 1:
                    assert cr.sizes(c)[0] == q, pl.tag  # |W|, the larger set, is the key's largest
                assert c.window64 and a + b >= 65, pl.tag
            sizes.append(q)
        assert sizes[0] < pc.RUNG_CAP == sizes[1] < sizes[2], sizes
    assert pc.RUNG_W[2][1] == pc.RUNG_CAP + 1


def test_extremes():
    pl, c, _ = by_tag(pc.values().tag)
    assert [x["value"] for x in c.layout["classes"][1:]] == list(pc.VALUE_IDS) == [0, 14, 15, 16]
    assert c.max_frontier >= 64  # one batch of configurations holds ids on both sides of 15
    for extra in (False, True):
        pl, c, _ = by_tag(pc.far_version(extra).tag)
        vers = [r[3] for r in pl.recs if r[3] != N]
        assert vers == list(pc.BAD_VERSIONS) and all(v < -1 or v > 2 ** 31 - 2 for v in vers)
        assert [(x["value"], x["version"], x["members"]) for x in c.layout["classes"][1:]] == \
            [(5, N, 1), (5, 2 ** 31 - 2, 2)]
        assert c.verdict == int(not extra)


def last_ok(pl):
    return max(i for i, r in enumerate(pl.recs) if r[5] != INF)


def _differs(pl, true, mutant):
    m = cr.check(pl.recs, mutant=mutant, budget=4000)
    if tuple(m[:6]) != tuple(true[:6]):
        return True
    stop = last_ok(pl)
    return cr.check(pl.recs, stop=stop, mutant=mutant, budget=4000).frontier != cr.check(pl.recs, stop=stop).frontier


@pytest.mark.parametrize("mutant", cr.MUTANTS)
def test_every_mutant_is_caught_by_its_family(mutant):
    assert set(pc.MUTANT_FAMILY) == set(cr.MUTANTS)
    family = pc.MUTANT_FAMILY[mutant]
    caught = [pl.tag for pl, c, _ in plants_of(family)
              if len(pl.recs) < 400 and _differs(pl, c, mutant)]
    print(mutant, "caught by", len(caught), "plants of", family, caught[:4])
    assert caught, mutant


def test_mutants_named_plants():
    """The plant each mutant was written against, by name."""
    for mutant, pl in (("width_short", pc.ladder(4, True)), ("width_short", pc.ladder(64, True)),
                       ("width_short", pc.neighbours(8, "middle", "driven")),
                       ("tuple_no_expected", pc.cas_expected(True)),
                       ("tuple_no_version", pc.far_version(True)),
                       ("no_pbit", pc.pending_ok("after")), ("no_pbit", pc.pending_ok("late")),
                       ("called_at_start", pc.single_several(False)),
                       ("called_at_start", pc.chunks((10, 63, 191), True, True)),
                       ("retire_fields", pc.single_several(False)),
                       ("slots_plus_one", pc.slots(58)), ("slots_plus_one", pc.one_slot(2))):
        true = by_tag(pl.tag)[1]
        m = cr.check(pl.recs, mutant=mutant, budget=4000)
        assert tuple(m[:6]) != tuple(true[:6]), (mutant, pl.tag)


def stops_of(pl, c, read_noops=True):
    """The stop ops of one plant: its fail op, the :ok return entered with
    the largest frontier, one return that is a no-op — where it has them.  (A read
    that was legal in the lone configuration at its call took no slot: a
    no-op here and on the device; the oracle lists that configuration.)"""
    out = []
    if c.fail_op >= 0:
        out.append(c.fail_op)
    if c.returns:
        big = max(range(len(c.returns)), key=lambda i: (c.returns[i][0], max(c.returns[i][1:])))
        out.append(c.return_ops[big])
    noops = [x for x in c.noops if read_noops or pl.recs[x][0] != R]
    if noops:
        out.append(noops[len(noops) // 2])
    return out


@functools.lru_cache(maxsize=None)
def frontier_at(name, k, stop):
    """counted_ref's frontier of plant k of a group at a stop op: computed
    once, shared with the GPU tests."""
    fr = cr.check(reference(name).plants[k].recs, stop=stop).frontier
    return None if fr is None else tuple(fr)


@pytest.mark.parametrize("name", ["small", "direct", "ladders"])
def test_frontiers_equal_the_oracles_below_64_pending(name):
    ref = reference(name)
    n_compared = n_beyond = 0
    for k, (pl, c) in enumerate(zip(ref.plants, ref.counted)):
        if c.verdict == cr.UNKNOWN:
            assert frontier_at(name, k, last_ok(pl)) is None, pl.tag
            continue
        for stop in stops_of(pl, c, read_noops=False):
            mine = frontier_at(name, k, stop)
            assert mine is not None and len(set(mine)) == len(mine), (pl.tag, stop)
            want, n = oracle.frontier(ref.ops[ref.off[k]:ref.off[k + 1]], stop, max_configs=1 << 12)
            assert n == len(mine), (pl.tag, stop, n, len(mine))
            if n > 1 << 12:
                continue
            if all(len(p) < 64 for _, _, p in want):
                assert {(v, x, tuple(sorted(p))) for v, x, p in want} == set(mine), (pl.tag, stop)
                n_compared += 1
            else:  # the oracle lists 64 of them: a subset of the whole list
                by_state = collections.defaultdict(list)
                for v, x, p in mine:
                    by_state[(v, x)].append(set(p))
                for v, x, p in want:
                    assert any(set(p) <= q for q in by_state[(v, x)]), (pl.tag, stop)
                n_beyond += 1
    print(name, "compared whole:", n_compared, "beyond 64 pending:", n_beyond)
    assert n_compared >= 20 if name == "direct" else n_beyond >= 10


def test_stops_that_are_not_ok_returns():
    pl, c, _ = by_tag(pc.ladder(4).tag)
    assert cr.check(pl.recs, stop=0).frontier is None            # a crashed op
    assert cr.check(pl.recs, stop=len(pl.recs)).frontier is None  # no record
    assert cr.check(pl.recs, stop=-1).frontier is None
    pl, c, _ = by_tag(pc.ladder(4, True).tag)
    assert cr.check(pl.recs, stop=c.fail_op).frontier not in (None, [])
    pl, c, _ = by_tag(pc.one_slot(0).tag)
    assert cr.check(pl.recs, stop=last_ok(pl)).frontier == []    # a [nil nil] read: a no-op return


@functools.lru_cache(maxsize=None)
def order_of(name, k):
    """counted_order_ref's Result of plant k at the oracle's cut."""
    ref = reference(name)
    cut = None if ref.jitc["verdict"][k] == 1 else int(ref.jitc["fail_prefix_end"][k]) - 1
    return cut, counted_order_ref.search(ref.plants[k].recs, cut, (0, N))


@pytest.mark.parametrize("name", pc.ALL_GROUPS)
def test_an_order_exists_on_every_fitting_plant(name):
    ref = reference(name)
    for k, (pl, c) in enumerate(zip(ref.plants, ref.counted)):
        cut, r = order_of(name, k)
        if c.verdict == cr.UNKNOWN:
            assert r.status == "unfit", (pl.tag, r.status)
            continue
        assert r.status == "found", (pl.tag, r.status, r.steps)
        assert order_ref.certify(pl.recs, r.ranks, cut, (0, N)), pl.tag
