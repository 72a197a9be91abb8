"""The frontier-search tiers (lds_tier_kernel, hbm_tier_kernel, hbm_coop_kernel
at 4, 8 and 16 waves, the dump kernels behind lc_check_frontiers) on
tests/planted_search.py's keys: set sizes on either side of the LDS regions'
128 configurations, the cooperative pools' 1,688 / 3,456 entries and the first
HBM rung's 2^14; 63 / 64 / 65 window slots, slot reuse; 64-record chunk
reloads with the frontier in a region; 254 .. 511 general-path returns around
the 8-bit LDS epoch; value ids around the 16-entry legality table.

Every key of every batch, no mask, on every path: verdict, reason, fail op,
failing prefix end, configurations explored and largest frontier equal the
CPU oracle's JITC search (tests/test_planted_search.py pins the oracle, the
plants' construction and tests/search_ref.py to each other).  Routing is
asserted from search_ref's set sizes, never from the device's own output."""
import functools

import numpy as np
import pytest

import oracle
import planted_search as ps
import search_ref
from helpers import pack_keys
from jepsen.etcd_amd import abi
from test_planted_search import reference

pytestmark = pytest.mark.gpu

FIELDS = ("verdict", "reason", "fail_op", "fail_prefix_end", "configs_explored", "max_frontier")
LC_REASON_FRONTIER_LDS = 6  # include/lincheck.h (internal: only with LC_FLAG_NO_HBM_RETRY)
LDS_CAP = 128

# env knobs of one search path (lincheck.cpp search_tier / hbm_tiers)
PATHS = {
    "lds_first": {"LC_JIT_DIRECT": "0"},  # lds_tier_kernel, then the ladder for what outgrows it
    "default": {},                        # straight to the cooperative tier (8 waves here)
    "one_wave": {"LC_HBM_COOP": "0"},     # hbm_tier_kernel
    "coop4": {"LC_HBM_COOP": "4"},
    "coop8": {"LC_HBM_COOP": "8"},
    "coop16": {"LC_HBM_COOP": "16"},
}
ONE_WAVE = ("lds_first", "one_wave")
BATCHES = ("small+lds", "pool+epochs", "rung")


def use_path(monkeypatch, path):
    for k in ("LC_JIT_DIRECT", "LC_HBM_COOP"):
        monkeypatch.delenv(k, raising=False)
    for k, v in PATHS[path].items():
        monkeypatch.setenv(k, v)


def assert_equal(pls, got, want, what, fields=FIELDS):
    for f in fields:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (what, f, len(bad), [(pls[k].tag, int(got[f][k]), int(want[f][k]))
                                                   for k in bad[:8]])


def outgrows_lds(ref):
    return search_ref.sizes(ref)[0] > LDS_CAP


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", BATCHES)
def test_every_field_equals_the_oracle(ctx, monkeypatch, name, path):
    pls, ops, off, j, refs = reference(name)
    use_path(monkeypatch, path)
    _, r = ctx.check(ops, off)
    st = ctx.stats()
    assert_equal(pls, r, j, (name, path))
    # version-less keys with a [nil x] read: every one reaches the search
    assert st["n_jit_keys"] == len(pls)
    if path == "lds_first":
        assert st["n_hbm_keys"] == sum(outgrows_lds(ref) for ref in refs)
    else:
        assert st["n_hbm_keys"] == len(pls)


@pytest.mark.parametrize("name", BATCHES[:2])
def test_lds_tier_alone_leaves_exactly_the_keys_past_128(ctx, monkeypatch, name):
    """LC_FLAG_NO_HBM_RETRY: the plants whose largest W or R set, by
    search_ref, exceeds kLdsCap end LC_REASON_FRONTIER_LDS; every other one
    is decided by lds_tier_kernel."""
    pls, ops, off, j, refs = reference(name)
    use_path(monkeypatch, "default")
    _, r = ctx.check(ops, off, abi.default_opts(flags=abi.LC_FLAG_NO_HBM_RETRY))
    big = np.array([outgrows_lds(ref) for ref in refs])
    assert big.any() and not big.all()
    bad = np.nonzero((r["reason"] == LC_REASON_FRONTIER_LDS) != big)[0]
    assert len(bad) == 0, [(pls[k].tag, int(r["reason"][k]), search_ref.sizes(refs[k])) for k in bad]
    assert (r["verdict"][big] == abi.LC_UNKNOWN).all()
    keep = np.nonzero(~big)[0]
    assert_equal([pls[k] for k in keep], r[keep], j[keep], name)


@functools.lru_cache(maxsize=None)
def budget_keys():
    pls = (ps.fan((7, 8)), ps.fan((5, 11), closer="read"), ps.chunked(129, good=False),
           ps.chunked(193, call_first=True, good=False))
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC)
    assert (j["verdict"] != -1).all() and (j["configs_explored"] > 100).all()
    return pls, j


@pytest.mark.parametrize("path", list(PATHS))
def test_budget_at_the_oracles_count(ctx, monkeypatch, path):
    """max_configs_per_key = E, the oracle's configs_explored, decides the
    key; E - 1 is LC_REASON_CONFIG_BUDGET where one wavefront counts every
    configuration (the cooperative paths count per batch: E // 2 is)."""
    pls, j = budget_keys()
    use_path(monkeypatch, path)
    for k, pl in enumerate(pls):
        ops, off = pack_keys([pl.recs])
        e = int(j["configs_explored"][k])
        _, r = ctx.check(ops, off, abi.default_opts(max_configs_per_key=e))
        assert_equal([pl], r, j[k:k + 1], (pl.tag, path, e))
        less = e - 1 if path in ONE_WAVE else e // 2
        _, r = ctx.check(ops, off, abi.default_opts(max_configs_per_key=less))
        assert (r["verdict"][0], r["reason"][0]) == (abi.LC_UNKNOWN, abi.LC_REASON_CONFIG_BUDGET), \
            (pl.tag, path, less, int(r["verdict"][0]), int(r["reason"][0]))


@pytest.mark.parametrize("path", ["lds_first", "default", "one_wave", "coop4"])
def test_window_of_65_is_unknown_and_counted_decides(ctx, monkeypatch, path):
    pls, ops, off, j, refs = reference("window65")
    assert all(ref.overflow for ref in refs)
    use_path(monkeypatch, path)
    _, r = ctx.check(ops, off)
    assert (r["verdict"] == abi.LC_UNKNOWN).all(), r["verdict"]
    assert (r["reason"] == abi.LC_REASON_WINDOW_OVERFLOW).all(), r["reason"]
    _, r = ctx.check(ops, off, abi.default_opts(flags=abi.LC_FLAG_COUNTED_CLASSES))
    assert_equal(pls, r, j, ("window65 counted", path))


@functools.lru_cache(maxsize=None)
def copies(n):
    """n keys cycling through the small group's plants, and the oracle's
    results tiled the same way."""
    pls, _, _, j, _ = reference("small")
    idx = np.arange(n) % len(pls)
    ops, off = pack_keys([pls[i].recs for i in idx])
    return [pls[i] for i in idx], ops, off, j[idx]


@pytest.mark.parametrize("n", [512, 513, 1024, 1025])
def test_batch_sizes_around_the_routing_thresholds(ctx, monkeypatch, n):
    """kHbmCoop8MaxKeys = 512 (8-wave workgroups up to it, 4-wave beyond) and
    kJitDirectMaxKeys = 1,024 (straight to the cooperative tier up to it, the
    LDS tier first beyond)."""
    pls, ops, off, j = copies(n)
    use_path(monkeypatch, "default")
    _, r = ctx.check(ops, off)
    st = ctx.stats()
    assert_equal(pls, r, j, n)
    assert st["n_jit_keys"] == n
    if n <= 1024:
        assert st["n_hbm_keys"] == n
    else:
        _, _, _, _, refs = reference("small")
        per = [outgrows_lds(ref) for ref in refs]
        assert st["n_hbm_keys"] == sum(per[i % len(per)] for i in range(n))


def test_frontier_dumps_equal_the_oracles_sets(ctx, monkeypatch):
    """lc_check_frontiers at the failing read of fans whose frontier there
    holds 127, 128, 129 and 4,000 configurations (by search_ref): with room
    for all of them, exactly oracle.frontier's set — the LDS dump up to 128,
    its HBM retry (launch_frontier_dump_hbm) beyond.  None is not accepted."""
    pls, ops, off, j, refs = reference("dump")
    use_path(monkeypatch, "default")
    sizes = [search_ref.sizes(ref)[2] for ref in refs]
    assert {127, 128, 129} <= set(sizes) and max(sizes) >= 4000
    stops = np.array([pl.fail_op for pl in pls])
    assert (stops >= 0).all() and (j["fail_op"] == stops).all()
    room = max(sizes) + 100
    got = ctx.check_frontiers(ops, off, stops, room)
    for k, pl in enumerate(pls):
        want, n_want = oracle.frontier(ops[off[k]:off[k + 1]], int(stops[k]))
        assert n_want == sizes[k] == len(want), pl.tag
        assert got[k] is not None, pl.tag
        assert len(got[k]) == n_want, (pl.tag, len(got[k]), n_want)
        assert set(got[k]) == want, pl.tag  # same count and same set: none duplicated
    # and cut off below the frontier's size: that many, distinct, all members
    got = ctx.check_frontiers(ops, off, stops, 100)
    for k, pl in enumerate(pls):
        want, _ = oracle.frontier(ops[off[k]:off[k + 1]], int(stops[k]))
        assert got[k] is not None and len(got[k]) == 100 == len(set(got[k])), pl.tag
        assert set(got[k]) <= want, pl.tag


@pytest.mark.parametrize("path", ["default", "coop4", "coop16"])
def test_pool_and_epoch_batches_repeat(ctx, monkeypatch, path):
    """Four runs in one context: the cooperative tier's work queue and table
    claims are where a race would show."""
    pls, ops, off, j, _ = reference("pool+epochs")
    use_path(monkeypatch, path)
    for i in range(4):
        _, r = ctx.check(ops, off)
        assert_equal(pls, r, j, (path, i))
