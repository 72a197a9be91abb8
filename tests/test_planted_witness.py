"""tests/search_order_ref.py (the first witness stage's depth-first search
restated decision for decision, its dead-end cache bucket for bucket) and
tests/planted_witness.py (deterministic keys on that search's edges), pinned
on the CPU:

* search_order_ref finds an order exactly where the exhaustive search of
  order_ref finds one, and both certifiers accept every order it returns;
* its cache spills a sixth node aimed at one bucket, drops a 41st aimed at one
  probe run and misses a node that lies behind a bucket with a free entry;
* the oracle's JITC search decides every plant, with the verdict and the fail
  op the builders claim by construction;
* every edge planted_witness names is hit, by what search_order_ref reports.

tests/test_gpu_witness_edges.py runs the same plants through
witness_search_kernel and takes its expectations from reference() and
order_of() below."""
import collections
import functools

import numpy as np
import pytest

import counted_order_ref
import oracle
import order_ref
import planted_witness as pw
import search_order_ref as so
import search_ref
from helpers import INF, N, R, W, pack_keys
from planted_search import NOBODY
from test_search_witness import FULL, MODELS, PREFIX, both, searched, tiny_keys

Ref = collections.namedtuple("Ref", "plants ops off jitc")


@functools.lru_cache(maxsize=None)
def reference():
    """(hand plants, ops, key_off, oracle JITC results); computed once, left
    unchanged."""
    pls = pw.plants()
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8)
    j.setflags(write=False)
    return Ref(pls, ops, off, j)


@functools.lru_cache(maxsize=None)
def order_of(tag):
    """(cut, search_order_ref's Result) of one hand plant at the oracle's cut:
    computed once, shared with the GPU tests."""
    ref = reference()
    k = next(i for i, pl in enumerate(ref.plants) if pl.tag == tag)
    cut = None if ref.jitc["verdict"][k] == 1 else int(ref.jitc["fail_prefix_end"][k]) - 1
    return cut, so.search(ref.plants[k].recs, cut, (0, N))


def order_at(recs, verdict, fail_prefix_end, init=N):
    """search_order_ref's Result of any key a search tier decided."""
    return so.search(recs, None if verdict == 1 else int(fail_prefix_end) - 1, (0, init))


def ranked(r):
    """The records of a found order, in rank order."""
    return sorted((i for i, x in enumerate(r.ranks) if x >= 0), key=lambda i: r.ranks[i])


# ------------------------------------------------- the restatement itself

@pytest.mark.parametrize("model", list(MODELS))
def test_restatement_finds_an_order_iff_one_exists(model):
    init = MODELS[model][1]
    n = collections.Counter()
    for recs in tiny_keys(model, 300, 7, 0x5117):
        r = so.search(recs, None, (0, init))
        whole = order_ref.find_order(recs, None, (0, init)) is not None
        assert r.status == ("found" if whole else "none"), recs
        if whole:
            assert both(recs, r.ranks, FULL, None, init), (recs, r.ranks)
        n[r.status] += 1
        n["backtracked"] += r.stored > 0
    for recs, kind, cut, _ in searched(model):
        if kind != PREFIX:
            continue
        r = so.search(recs, cut, (0, init))
        assert r.status == "found", (recs, cut)
        assert both(recs, r.ranks, PREFIX, cut, init), (recs, cut, r.ranks)
        # with the failing return inside, every order is tried and none is found
        assert so.search(recs, cut + 1, (0, init)).status == "none", (recs, cut)
        n["prefix"] += 1
    assert n["found"] > 100 and n["none"] == n["prefix"] > 10, n
    if model != "mutex":  # (a mutex history never backtracks: test_search_witness.test_hand_cases)
        assert n["backtracked"] > 10, n


def test_hash_is_the_kernels():
    """ws_hash by hand on the nodes whose products are plain: all zeros, and
    one field at a time equal to 1 (each constant alone, then the finalizer)."""
    m64 = (1 << 64) - 1

    def fin(h):
        h ^= h >> 29
        return ((h * 0xBF58476D1CE4E5B9) & m64) >> 32

    assert so.ws_hash(0, 0, 0, 0) == 0
    assert so.ws_hash(0, 1, 0, 0) == fin(0x9E3779B97F4A7C15)
    assert so.ws_hash(0, 0, 1, 0) == fin(0xC2B2AE3D27D4EB4F)
    assert so.ws_hash(1, 0, 0, 0) == fin((0xC2B2AE3D27D4EB4F << 32) & m64)
    assert so.ws_hash(0, 0, 0, 1) == fin(0x165667B19E3779F9)
    # nil is the 32-bit pattern of -1, in the value and in the version
    assert so.ws_hash(0, 0, 0, -1) == fin((0xFFFFFFFF * 0x165667B19E3779F9) & m64)
    assert so.ws_hash(0, 0, -1, 0) == fin((0xFFFFFFFF * 0xC2B2AE3D27D4EB4F) & m64)


def _aimed(bucket, count, start=0):
    """`count` nodes whose probe run starts at `bucket`."""
    out, mask = [], start
    while len(out) < count:
        mask += 1
        if so.ws_hash(3, mask, 7, 2) & (so.BUCKETS - 1) == bucket:
            out.append((3, mask, 7, 2))
    return out


def test_cache_spills_drops_and_stops_at_a_free_entry():
    c = so.Cache()
    nodes = _aimed(4090, so.ENTRIES * so.PROBES + 1)  # (the run wraps: 4090 .. 4095, 0, 1)
    for i, node in enumerate(nodes[:-1]):
        assert not c.lookup(node)
        assert c.insert(node) is False
        assert c.lookup(node)
        assert (c.stored, c.spilled, c.dropped) == (i + 1, max(0, i + 1 - so.ENTRIES), 0), i
    # the sixth went to the next bucket, the 40th to the eighth — across the wrap
    assert nodes[5] in c.buckets[4091] and nodes[39] in c.buckets[1]
    assert sorted(c.buckets) == [0, 1, 4090, 4091, 4092, 4093, 4094, 4095]
    # the 41st meets 8 full buckets: not stored, and not found afterwards
    assert c.insert(nodes[-1]) is False
    assert (c.stored, c.spilled, c.dropped) == (40, 35, 1) and not c.lookup(nodes[-1])
    assert c.insert(nodes[0]) is True and c.stored == 40  # there already: nothing stored
    # a run that starts in a full bucket of the other run goes on past it
    other = _aimed(4095, 1, start=10 ** 6)[0]
    assert c.insert(other) is False and other in c.buckets[2] and c.spilled == 36
    # a lookup stops at the first bucket with a free entry: a node lying
    # behind one (nothing puts it there — nothing is ever removed) is missed
    c = so.Cache()
    a, b = _aimed(100, 2)
    c.insert(a)
    c.buckets[101] = [b]
    assert c.lookup(a) and not c.lookup(b)
    c.buckets[100] = [a] + _aimed(100, 4, start=10 ** 6)  # bucket 100 full: the lookup goes on
    assert c.lookup(b)


# ------------------------------------------------- the plants

def test_the_oracle_decides_every_plant():
    ref = reference()
    assert len({pl.tag for pl in ref.plants}) == len(ref.plants)
    assert {pl.family for pl in ref.plants} == set(pw.FAMILIES)
    for k, pl in enumerate(ref.plants):
        # (the default max_configs_per_key: none needs more)
        assert ref.jitc["verdict"][k] != -1, pl.tag
        assert (int(ref.jitc["verdict"][k]), int(ref.jitc["fail_op"][k])) == (pl.verdict, pl.fail_op), pl.tag
        assert all(rec[3] == N for rec in pl.recs), pl.tag  # version-less
        calls = [rec[4] for rec in pl.recs]
        times = calls + [rec[5] for rec in pl.recs if rec[5] != INF]
        assert calls == sorted(calls) and len(set(times)) == len(times), pl.tag
        if not pl.verdict:
            assert int(ref.jitc["fail_prefix_end"][k]) == pl.recs[pl.fail_op][5], pl.tag


def test_every_found_order_is_certified_and_the_set_stays_small():
    status = collections.Counter()
    heavy = []
    for pl in pw.plants():
        cut, r = order_of(pl.tag)
        status[r.status] += 1
        if r.status == "found":
            assert order_ref.certify(pl.recs, r.ranks, cut, (0, N)), pl.tag
            assert both(pl.recs, r.ranks, FULL if pl.verdict else PREFIX, cut, N), pl.tag
        else:
            assert r.ranks is None and r.status in ("budget", "window"), (pl.tag, r.status)
        if r.steps > 20000:
            heavy.append(pl.tag)
    assert len(heavy) <= 12, heavy
    assert status["budget"] == 2 and status["window"] == 1, status


def _fan_ranks(m):
    """The only order of a back-fan: W_m R_m W_m-1 R_m-1 .. (writes are
    records 0 .. m - 1, the read of v is record m + (m - v))."""
    ranks = [0] * (2 * m)
    for v in range(1, m + 1):
        ranks[v - 1] = 2 * (m - v)
        ranks[m + (m - v)] = 2 * (m - v) + 1
    return ranks


def test_backfans_backtrack_and_cache():
    prev = 0
    for m in pw.BACKFANS:
        pl = pw.backfan(m)
        _, r = order_of(pl.tag)
        assert r.status == "found" and r.ranks == _fan_ranks(m), pl.tag
        assert r.dropped == 0 and r.steps > prev, pl.tag
        prev = r.steps
        if m == 1:
            assert (r.steps, r.hits, r.stored) == (2, 0, 0)
        else:  # dead ends stored — the nodes without a candidate and the frames popped
            assert r.steps > 2 * m and r.stored >= 1, (pl.tag, r)
        if m >= 3:
            assert r.hits >= 1, (pl.tag, r)
    # no single bucket overflows below m = 9: the chains and the cap go past that
    assert order_of(pw.backfan(8).tag)[1].spilled == 0 < order_of(pw.backfan(9).tag)[1].spilled


def test_forced_crashed_reads_are_ranked_behind_their_value():
    for m, crs in pw.FORCED:
        pl = pw.backfan(m, crs)
        _, r = order_of(pl.tag)
        plain = order_of(pw.backfan(m).tag)[1]
        assert r.status == "found" and r.steps > plain.steps, pl.tag
        seq = ranked(r)
        for i, rec in enumerate(pl.recs):
            if rec[0] == R and rec[5] == INF:
                if rec[1] == 1:  # legal beside the key's last return only, which goes first and ends the search
                    assert r.ranks[i] == -1, (pl.tag, i)
                    continue
                # legal once its value is written: taken at once, so it stands
                # right behind the write or a read of that value
                before = pl.recs[seq[r.ranks[i] - 1]]
                assert before[1] == rec[1] and r.ranks[i] >= 1, (pl.tag, i)
        assert len(seq) == len(pl.recs) - (1 in crs), pl.tag


def test_chains_fill_buckets_then_probe_runs_then_the_cap():
    got = {ms: order_of(pw.chain(ms).tag)[1] for ms in pw.CHAINS}
    for ms, r in got.items():
        assert r.status == ("budget" if ms == (10, 10, 10) else "found"), ms
        if r.status == "found":
            want, at = [], 0
            for m in ms:  # fan after fan, each in its only order
                want += [at + x for x in _fan_ranks(m)]
                at += 2 * m
            assert r.ranks == want, ms
    # buckets overflow, no probe run does
    assert got[(10, 9)].spilled >= 1 and got[(10, 9)].dropped == 0
    # probe runs overflow: dead ends go unstored, are met again and searched
    # again — and the order is still found, within the cap
    for ms in ((10, 10), (10, 10, 8)):
        r = got[ms]
        assert r.dropped >= 1 and r.status == "found" and r.steps <= so.NODE_CAP, (ms, r)
    assert got[(10, 10)].steps > 2 * order_of(pw.backfan(10).tag)[1].steps  # (the price of the drops)
    assert got[(3, 4)].spilled == got[(5, 5, 5)].spilled == 0


def test_the_node_cap():
    for pl in [pw.backfan(m) for m in pw.CAPPED] + [pw.chain((10, 10, 10))]:
        _, r = order_of(pl.tag)
        assert (r.status, r.steps, r.ranks) == ("budget", so.NODE_CAP + 1, None), pl.tag
    # one step below the cap's test a key still ends found: write_reads below


def test_ahead_plants_put_the_chunk_edge_at_every_position_of_the_fan():
    fan = order_of(pw.backfan(9).tag)[1]
    edges = collections.defaultdict(set)
    for p in pw.AHEAD_P:
        pl = pw.ahead(p)
        cut, r = order_of(pl.tag)
        ev = so.events(pl.recs, cut)
        writes = [i for i, rec in enumerate(pl.recs) if rec[5] == INF]
        reads = [i for i, rec in enumerate(pl.recs) if rec[0] == R]
        assert writes == list(range(p, p + 9)) and reads == list(range(p + 9, p + 18)), pl.tag
        assert [ev.slots[i] for i in writes] == list(range(9)), pl.tag
        b = 64 if p <= 64 else 128
        assert p <= b <= p + 9 and max(reads) >= b  # the edge: before write b - p, or before the first read
        edges[b].add(b - p)
        assert r.status == "found" and r.ranks[p:] == [p + x for x in _fan_ranks(9)], pl.tag
        # the fan's search, one step per write ahead of it
        assert (r.steps, r.hits, r.stored) == (fan.steps + p, fan.hits, fan.stored), pl.tag
    assert edges == {64: set(range(10)), 128: set(range(10))}


def test_opened_plants_fill_the_window():
    want = {53: 63, 54: 64, 55: 65}
    assert set(want) == set(pw.OPENED_F)
    fan = order_of(pw.backfan(9).tag)[1]
    for f, n_open in want.items():
        pl = pw.opened(f)
        cut, r = order_of(pl.tag)
        ev = so.events(pl.recs, cut)
        assert ev.open_max == n_open, pl.tag
        # the tiers give the crashed reads no slot: they decide all three
        s = search_ref.check(pl.recs)
        assert not s.overflow and s.verdict == 1, pl.tag
        if n_open == 65:
            assert r.status == "window" and ev.slots is None
            # the second stage's layout: nine classes of one, the reads left out
            c = counted_order_ref.search(pl.recs, cut, (0, N))
            assert c.status == "found" and order_ref.certify(pl.recs, c.ranks, cut, (0, N))
            assert all(c.ranks[i] == -1 for i in range(f))
            continue
        first_read = f + 9
        assert ev.slots[first_read] == n_open - 1 and set(ev.slots[:first_read]) == set(range(n_open - 1))
        assert r.status == "found" and all(r.ranks[i] == -1 for i in range(f)), pl.tag
        assert r.ranks[f:] == _fan_ranks(9), pl.tag
        assert (r.steps, r.hits, r.stored) == (fan.steps, fan.hits, fan.stored), pl.tag
    assert so.events(pw.opened(54).recs).slots[54 + 9] == 63  # the last slot


def test_reuse_plants_sit_in_scattered_slots():
    for pl in pw.family("reuse"):
        cut, r = order_of(pl.tag)
        ev = so.events(pl.recs, cut)
        m = sum(1 for rec in pl.recs if rec[5] == INF)
        writes = {rec[1]: i for i, rec in enumerate(pl.recs) if rec[0] == W}
        reads = {rec[1]: i for i, rec in enumerate(pl.recs) if rec[0] == R and rec[1] not in (N, NOBODY)}
        l, a, b = 0, 1, 2
        assert [ev.slots[i] for i in (l, a, b)] == [0, 1, 2]
        ws = [ev.slots[writes[v]] for v in range(1, m + 1)]
        assert ws == [3, 1] + list(range(4, m + 2)), pl.tag  # not contiguous: B sits in slot 2
        # a freed low slot is retaken by a later call
        assert ev.slots[writes[2]] == ev.slots[a] < ev.slots[writes[1]]
        # L returns between the fan's second and third read; the third takes L's slot
        k_l = next(k for k, e in enumerate(ev.ev) if e[0] == l)
        assert [e[0] for e in ev.ev[k_l - 2:k_l + 3]] == [reads[m], reads[m - 1], l, reads[m - 2], b], pl.tag
        assert ev.slots[reads[m]] == ev.slots[reads[m - 1]] == m + 2
        assert ev.slots[reads[m - 2]] == ev.slots[reads[m - 3]] == ev.slots[l] == 0, pl.tag
        # L and B are forced ahead of the fan's writes, which are retried many
        # times: every rewind to a frame of the first two reads puts L back
        assert r.status == "found" and (r.ranks[a], r.ranks[l], r.ranks[b]) == (0, 1, 2), (pl.tag, r)
        assert r.hits > 100, (pl.tag, r)
        assert r.steps > 20 * len(pl.recs), pl.tag
    assert {pl.verdict for pl in pw.family("reuse")} == {0, 1}


def test_unwritten_plants_cut_an_open_fan():
    for m, done in pw.UNWRITTEN:
        pl = pw.unwritten(m, done)
        cut, r = order_of(pl.tag)
        assert pl.verdict == 0 and cut == pl.recs[pl.fail_op][5] - 1, pl.tag
        ev = so.events(pl.recs, cut)
        # the failing read is called by the cut and open at it, as the crashed writes are
        assert ev.slots[pl.fail_op] is not None and ev.slots[pl.fail_op + 1] is None, pl.tag
        assert len(ev.ev) == done and all(ev.slots[i] is not None for i in range(m)), pl.tag
        assert r.status == "found" and r.ranks[pl.fail_op] == r.ranks[-1] == -1, pl.tag
        if done == 0:  # no return by the cut: found, nothing ranked
            assert r.ranks == [-1] * len(pl.recs) and r.steps == 0
        if done == m:
            assert r.ranks[:2 * m] == _fan_ranks(m), pl.tag
            plain = order_of(pw.backfan(m).tag)[1]
            assert (r.steps, r.hits, r.stored) == (plain.steps, plain.hits, plain.stored), pl.tag
    assert {done for _, done in pw.UNWRITTEN} >= {0} and any(m == d for m, d in pw.UNWRITTEN)


def test_deadline_plant_takes_the_earliest_return_first():
    pl = pw.deadline()
    _, r = order_of(pl.tag)
    ev = so.events(pl.recs)
    crashed, a, b, x, rd = range(5)
    assert ev.slots == [0, 1, 2, 3, 1] and [e[0] for e in ev.ev] == [x, b, a, rd]
    assert pl.recs[x][5] < pl.recs[b][5] < pl.recs[a][5]
    # b (slot 2) before X, a after it, the crashed write of slot 0 never: no backtracking
    assert (r.status, r.ranks, r.steps, r.stored) == ("found", [-1, 2, 0, 1, 3], 4, 0), r
    # the lowest slot first would give another order, valid as well
    other = [0, 3, 2, 1, 4]
    assert order_ref.certify(pl.recs, other, None, (0, N)) and other != r.ranks


def test_write_reads_take_one_step_per_op_and_the_budget_edge():
    for n_reads in pw.WRITE_READS:
        pl = pw.write_reads(n_reads)
        _, r = order_of(pl.tag)
        assert (r.status, r.steps, r.hits, r.stored) == ("found", n_reads + 1, 0, 0), pl.tag
        assert r.ranks == list(range(n_reads + 1))
        # max_steps = r + 1 is enough; with r the test at the loop's top ends the key
        at = so.search(pl.recs, None, (0, N), max_steps=n_reads + 1)
        assert (at.status, at.steps) == ("found", n_reads + 1)
        below = so.search(pl.recs, None, (0, N), max_steps=n_reads)
        assert (below.status, below.steps, below.ranks) == ("budget", n_reads + 1, None)
    # the frontier search explores 2 configurations on these keys
    k = [pl.tag for pl in reference().plants].index(pw.write_reads(30).tag)
    assert int(reference().jitc["configs_explored"][k]) == 2


def test_length_plants_surround_the_carving_unit():
    assert sorted(len(pl.recs) for pl in pw.family("length")) == list(pw.LENGTHS) == \
        [127, 128, 129, 255, 256, 257]
    fan = order_of(pw.backfan(7).tag)[1]
    for pl in pw.family("length"):
        _, r = order_of(pl.tag)
        n = len(pl.recs)
        assert r.status == "found" and min(r.ranks) == 0 and sorted(r.ranks) == list(range(n)), pl.tag
        assert (r.steps, r.hits, r.stored) == (fan.steps + n - 14, fan.hits, fan.stored), pl.tag


def test_interleaved_batch_is_the_same_plants():
    pls = pw.interleaved()
    assert sorted(pl.tag for pl in pls) == sorted(pl.tag for pl in pw.plants())
    lens = [len(pl.recs) for pl in pls]
    assert lens[0] == max(lens) and lens[1] == min(lens)
    assert np.sign(np.diff(lens[:20])).tolist() == [-1, 1] * 9 + [-1]  # long, short, long, ..
