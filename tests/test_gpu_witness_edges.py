"""witness_search_kernel (LC_FLAG_SEARCH_WITNESS: ws_search and its helpers,
csrc/witness_search.hip) on tests/planted_witness.py's keys: dead ends cached
and met again, cache buckets and probe runs that overflow, the node cap,
backtracking across the 64-record chunks of the event pass, 63 / 64 / 65 ops
open, slots reused and restored by a rewind, invalid keys cut with a fan open,
key lengths round the 128-record carving unit, waves that serve several keys
with one cache, lists compacted across the ballot's 64 keys and the block's
256.

The search is deterministic — one wave per key, a fixed order of trial, a
cache private to the key — so every key has one right order and one right
step count: the witness array equals tests/search_order_ref.py's ranks
exactly, `nodes` its steps, `cache_hits` its hits, and the kind is what its
status says.  Expectations come from the restatement and the CPU oracle,
never from the device's own output (tests/test_planted_witness.py pins the
restatement, the plants and the oracle to each other).  Default options, no
time budget."""
import functools

import numpy as np
import pytest

import counted_order_ref
import planted
import planted_witness as pw
import search_order_ref as so
import test_planted_search
from helpers import N, W
from jepsen.etcd_amd import abi
from test_planted_witness import order_at, order_of
from test_search_witness import FULL, PREFIX, both, certify_all, run

pytestmark = pytest.mark.gpu

SW, CW = abi.LC_FLAG_SEARCH_WITNESS, abi.LC_FLAG_COUNTED_WITNESS
N_WAVES = 1024  # kWitnessWaves
COUNTS = ("n_found", "n_budget", "n_window")


def counts_of(status):
    """(n_found, n_budget, n_window) of one key that ends with `status`."""
    return {"found": (1, 0, 0), "none": (0, 1, 0), "budget": (0, 1, 0), "window": (0, 0, 1)}[status]


def assert_key(r, k, tag, verdict, want):
    """Key k of a run against the restatement's Result: kind, witness."""
    a, b = int(r.off[k]), int(r.off[k + 1])
    assert int(r.res["verdict"][k]) == verdict, tag
    assert r.kind0[k] == 0, tag  # decided by a search tier
    if want.status == "found":
        assert int(r.kind[k]) == (FULL if verdict == 1 else PREFIX), (tag, int(r.kind[k]))
        got = r.wit[a:b].tolist()
        assert got == want.ranks, (tag, [(i, x, y) for i, (x, y) in enumerate(zip(got, want.ranks)) if x != y][:8])
        assert both(r.ops[a:b], r.wit[a:b], int(r.kind[k]), int(r.res["fail_prefix_end"][k]) - 1, r.init), tag
    else:  # given up: kind NONE, nothing of the witness written
        assert int(r.kind[k]) == 0, (tag, int(r.kind[k]))
        assert r.wit[a:b].tobytes() == r.wit0[a:b].tobytes(), tag


def assert_sums(r, wants, what):
    st = r.st
    assert st["n_keys"] == len(wants), (what, st)
    assert tuple(st[c] for c in COUNTS) == tuple(map(sum, zip(*(counts_of(w.status) for w in wants)))), (what, st)
    assert (st["nodes"], st["cache_hits"]) == (sum(w.steps for w in wants), sum(w.hits for w in wants)), \
        (what, st, sum(w.steps for w in wants), sum(w.hits for w in wants))


def assert_plant(r, k, pl):
    cut, want = order_of(pl.tag)
    assert (int(r.res["verdict"][k]), int(r.res["fail_op"][k])) == (pl.verdict, pl.fail_op), pl.tag
    assert cut == (None if pl.verdict else int(r.res["fail_prefix_end"][k]) - 1), pl.tag
    assert_key(r, k, pl.tag, pl.verdict, want)
    return want


@pytest.mark.parametrize("family", pw.FAMILIES)
def test_key_for_key(ctx, family):
    """Every hand plant alone in its call (the stage's counts are per call)."""
    heaviest = (0, None, 0.0)
    for pl in pw.family(family):
        r = run(ctx, [pl.recs], N)
        want = assert_plant(r, 0, pl)
        st = r.st
        assert (st["n_keys"],) + tuple(st[c] for c in COUNTS) == (1,) + counts_of(want.status), (pl.tag, st)
        assert (st["nodes"], st["cache_hits"]) == (want.steps, want.hits), (pl.tag, st, want.steps, want.hits)
        assert certify_all(r, want_all=False) == (want.status == "found"), pl.tag
        heaviest = max(heaviest, (want.steps, pl.tag, st["kernel_ms"]))
    print("%s: heaviest key %s, %d steps, kernel_ms %.2f" % (family, heaviest[1], heaviest[0], heaviest[2]))


@functools.lru_cache(maxsize=None)
def hand_batch():
    pls = pw.interleaved()
    return pls, tuple(order_of(pl.tag)[1] for pl in pls)


def test_in_sum(ctx):
    """The same plants as one batch, long and short keys alternating: a wave's
    frames, events and slots are carved for the longest key of the launch."""
    pls, wants = hand_batch()
    r = run(ctx, [pl.recs for pl in pls], N)
    for k, pl in enumerate(pls):
        assert_plant(r, k, pl)
    assert_sums(r, wants, "hand plants")
    assert certify_all(r, want_all=False) == sum(w.status == "found" for w in wants)


def test_generation_stamps(ctx):
    """kWitnessWaves + 200 keys: eight back-fans of 5 .. 8, then a one-op key,
    over and over.  1,088 of the 1,224 keys use the cache and there are 1,024
    waves, so some wave serves two of them — whichever one it is, the second
    key meets the first one's entries, of the very nodes it looks up (a fan of
    m begins as a fan of m + 1 does), stale by their stamp alone.  Twice on one
    context: the workspace is zeroed by each launch."""
    cycle = [pw.backfan(m) for m in (5, 6, 7, 8)] * 2 + [planted.Plant("one", "one", [[W, 1, N, N, 0, 1]], 1, -1)]
    pls = [cycle[i % len(cycle)] for i in range(N_WAVES + 200)]
    wants = [order_of(pl.tag)[1] if pl.family != "one" else so.search(pl.recs) for pl in pls]
    assert sum(w.stored > 0 for w in wants) > N_WAVES and wants[8].steps == 1
    for _ in range(2):
        r = run(ctx, [pl.recs for pl in pls], N)
        for k, pl in enumerate(pls):
            assert_key(r, k, pl.tag, 1, wants[k])
        assert_sums(r, wants, "generation stamps")


@pytest.mark.parametrize("n_keys", [1, 63, 64, 65, 255, 256, 257])
def test_compacted_lists(ctx, n_keys):
    """witness_compact_kernel: back-fans (even keys) between version-pinned
    keys the version-order tier witnesses itself (kinds 1 and 2), batches on
    either side of the ballot's 64 keys and the block's 256."""
    fans = [pw.backfan(m) for m in (2, 3, 4, 5, 6)]
    pinned = [planted.base(5), planted.swap(9, 0, 3), planted.base(64, 3), planted.swap(65, 3, 20)]
    pls = [fans[(k // 2) % 5] if k % 2 == 0 else pinned[(k // 2) % 4] for k in range(n_keys)]
    r = run(ctx, [pl.recs for pl in pls], N)
    wants = []
    for k, pl in enumerate(pls):
        if k % 2:
            assert int(r.res["verdict"][k]) == pl.verdict and r.kind0[k] == (1 if pl.verdict else 2), pl.tag
        else:
            wants.append(assert_plant(r, k, pl))
    assert_sums(r, wants, n_keys)  # n_keys of the stats: the version-less keys
    # (certify_all: the tiers' kinds and witnesses are byte-identical with the flag)
    assert certify_all(r) == len(wants)


def test_budget_edge(ctx):
    """max_configs_per_key bounds the steps: the loop's test is `steps >
    budget`, at its top, and a key's last step is followed by one more
    iteration (the return) — so r + 1 is enough for the r + 1 ops of
    write_reads(r), and r is not.  (The frontier search explores 2
    configurations on that key: the tiers decide it either way.)"""
    n_reads = 30
    pl = pw.write_reads(n_reads)
    r = run(ctx, [pl.recs], N, max_configs_per_key=n_reads + 1)
    assert_plant(r, 0, pl)
    assert (r.st["n_found"], r.st["n_budget"], r.st["nodes"]) == (1, 0, n_reads + 1), r.st
    r = run(ctx, [pl.recs], N, max_configs_per_key=n_reads)
    assert int(r.res["verdict"][0]) == 1
    below = so.search(pl.recs, None, (0, N), max_steps=n_reads)
    assert_key(r, 0, pl.tag, 1, below)  # kind NONE, the witness as it was without the flag
    assert (r.st["n_found"], r.st["n_budget"], r.st["n_window"], r.st["nodes"]) == (0, 1, 0, below.steps), r.st
    # the cap itself: kWitnessNodeCap + 1 steps, and nothing of the witness written
    pl = pw.backfan(pw.CAPPED[0])
    r = run(ctx, [pl.recs], N)
    want = assert_plant(r, 0, pl)
    assert want.status == "budget" and r.kind.tolist() == [0] and r.wit.tobytes() == r.wit0.tobytes()
    assert (r.st["n_found"], r.st["n_budget"], r.st["nodes"]) == (0, 1, so.NODE_CAP + 1), r.st
    assert r.st["cache_hits"] == want.hits


def test_65_open_ops_go_to_the_counted_stage(ctx):
    """55 crashed reads beside a 9-fan: the tiers (no slot for a crashed read)
    decide the key, the first stage leaves it at its 65th open op, and the
    counted stage — crashed reads take no slot there either — finds the order
    counted_order_ref gives."""
    pl = pw.opened(55)
    r = run(ctx, [pl.recs], N, CW)
    cst = ctx.last_counted_witness_stats()
    assert order_of(pl.tag)[1].status == "window" and int(r.res["verdict"][0]) == 1
    assert (r.st["n_keys"], r.st["n_found"], r.st["n_budget"], r.st["n_window"]) == (1, 0, 0, 1), r.st
    assert (r.st["nodes"], r.st["cache_hits"]) == (0, 0)
    want = counted_order_ref.search(pl.recs, None, (0, N))
    assert want.status == "found"
    assert (cst["n_keys"], cst["n_found"], cst["nodes"], cst["cache_hits"]) == (1, 1, want.steps, want.hits), cst
    assert r.kind.tolist() == [FULL] and r.wit.tolist() == want.ranks
    assert both(r.ops, r.wit, FULL, -1, N)
    # without the second flag the key keeps kind NONE and its witness untouched
    r = run(ctx, [pl.recs], N)
    assert_key(r, 0, pl.tag, 1, order_of(pl.tag)[1])


@pytest.mark.parametrize("name", ["small+lds", "pool+epochs"])
def test_planted_search_batches(ctx, name):
    """tests/planted_search.py's keys — wide fans of equal values, full
    windows, 254 .. 511 general-path returns — with the flag: what the
    restatement says of each key, found, window or budget."""
    parts = [test_planted_search.reference(part) for part in name.split("+")]
    pls = [pl for part in parts for pl in part[0]]
    jitc = np.concatenate([part[3] for part in parts])
    wants = [order_at(pl.recs, int(jitc["verdict"][k]), jitc["fail_prefix_end"][k]) for k, pl in enumerate(pls)]
    r = run(ctx, [pl.recs for pl in pls], N)
    for k, pl in enumerate(pls):
        if not pl.verdict:  # the cut the restatement searched at
            assert int(r.res["fail_prefix_end"][k]) == int(jitc["fail_prefix_end"][k]), pl.tag
        assert_key(r, k, pl.tag, pl.verdict, wants[k])
    assert_sums(r, wants, name)
    seen = {w.status for w in wants}
    assert "found" in seen and (name != "pool+epochs" or "window" in seen), seen


def test_device_resident(ctx):
    """The interleaved hand batch through lc_check_device with d_witness /
    d_witness_kind: kinds and witnesses equal the host path's."""
    import torch
    pls, wants = hand_batch()
    r = run(ctx, [pl.recs for pl in pls], N)
    dev = torch.device("cuda:0")
    n = len(pls)
    d_ops, d_off = torch.from_numpy(r.ops).to(dev), torch.from_numpy(r.off).to(dev)
    d_out = torch.zeros(n * abi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_wit = torch.full((len(r.ops),), -3, dtype=torch.int32, device=dev)
    d_kind = torch.full((n,), -3, dtype=torch.int32, device=dev)
    ctx.check_device(d_ops.data_ptr(), d_off.data_ptr(), n, d_out.data_ptr(),
                     opts=abi.default_opts(flags=SW), d_witness=d_wit.data_ptr(),
                     d_witness_kind=d_kind.data_ptr())
    torch.cuda.synchronize()
    st = ctx.last_witness_stats()
    assert d_out.cpu().numpy().tobytes() == r.res.tobytes()
    kind, wit = d_kind.cpu().numpy(), d_wit.cpu().numpy()
    assert (kind == r.kind).all() and (wit == r.wit).all()
    for k, (pl, want) in enumerate(zip(pls, wants)):
        a, b = int(r.off[k]), int(r.off[k + 1])
        if want.status == "found":
            assert kind[k] == (FULL if pl.verdict else PREFIX) and wit[a:b].tolist() == want.ranks, pl.tag
        else:
            assert kind[k] == 0, pl.tag
    assert {c: st[c] for c in COUNTS + ("n_keys", "nodes", "cache_hits")} == \
        {c: r.st[c] for c in COUNTS + ("n_keys", "nodes", "cache_hits")}
