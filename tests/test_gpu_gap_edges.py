"""The gap matching (gapmatch.h) at every chunk, class, LDS and probe edge:
tests/planted_gap.py's keys — augmenting paths of exactly L + 1 ops around
the 64-op chunks and the 64 levels of the flip, class mode from 128 optional
ops and up to 64 classes, forced branches on either side of the violation
scan's 64-gap step, pinned optional ops in the probed prefixes, and the
smallest shapes on either side of fast_gap's limits and of the matching's
LDS reserve — through fast_gap (short keys), the gap tier proper (behind a
ladder past 1,024 records), one-wave, 256- and 512-thread workgroups,
in-place bisection and multisection rounds.

Every key, no mask: verdict, fail op and failing prefix end equal the CPU
oracle's JITC search (tests/test_planted_gap.py pins the oracle's answers to
the plants' construction).

lc_stats has no field for the workgroup shape, the counterexample search's
mode, GD_RETRY or the matching's mode, so that a batch takes the path it is
built for rests on these constants; when one moves, move the batch with it:
  lincheck.cpp  kGapWaveMaxLen = 256, kGapWaveMinKeys = 1,024 (one-wave
                workgroups: test_one_wave_workgroups);
                kGapWideMaxKeys = 64, kGapWideMinLen = 2,048 (512 threads:
                the group "longer");
                kGapProbeMinLen = 1,024 and 2 * keys <= wg_cap (multisection
                rounds: "longer", "mid"; wg_cap = min(kGapMaxWG = 1,024,
                kGapWsBytes / one workgroup's workspace) is 1,024 for keys
                this long; every other batch bisects in place);
                kGapSkelLdsMax = 78 KB, the LDS of 68 B per record of the
                longest key + 8 KB (test_matching_at_the_lds_reserve).
  gap_tier.hip  kMatchReserve = 8 KB, kSkelLdsBytes = 68 (GD_RETRY).
  gapmatch.h    kClsMinOps = 128, kMaxCls = 64, match_lds_bytes.
  kernels.h / check_kernel.hip  kFastMaxRecords = 1,024, kFgMaxGaps = 48,
                kFgMaxOps = 96, kFgStash = 32 (the handoff).
planted_gap.py holds copies (K_*, match_lds_bytes, lds_room), and
test_planted_gap.py checks the plants' shapes against them."""
import functools

import numpy as np
import pytest

import oracle
import planted_gap as pg
from helpers import pack_keys
from jepsen.etcd_amd import abi
from test_gpu_single_pass import both_paths
from test_gpu_witness import certify

pytestmark = pytest.mark.gpu

SHORT = tuple(f + v for f in pg.FAMILIES for v in ("-short", "-shift")) + ("limits",)
LONG = tuple(f + "-long" for f in pg.FAMILIES) + ("limits-long",)
ALL_FIELDS = ("verdict", "reason", "fail_op", "fail_prefix_end", "configs_explored", "max_frontier")


def plants(name):
    fam, _, var = name.partition("-")
    if name == "longer":
        return pg.longer_plants()
    if name == "mid":
        # longest key between 1,025 and 2,047 records, few keys: 256 threads,
        # multisection rounds
        return tuple(pg.lengthen(pl, 1500) for pl in plants("pending-long")[:12]) + \
            plants("chain-long")[:12]
    if name.startswith("lim:"):
        return tuple(pg.limit_plants()[name[4:]])
    if fam == "limits":
        pls = pg.all_limit_plants()
        return pls if not var else tuple(pg.lengthen(pl, pg.LONG) for pl in pls)
    return pg.family_plants(fam, {"short": 0, "shift": pg.SHIFT, "long": pg.LONG}[var])


@functools.lru_cache(maxsize=None)
def batch(name):
    """(plants, ops, key_off, oracle results) of one group, computed once and
    left unchanged; long and short keys alternating."""
    pls = pg.interleave(plants(name))
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=16, max_configs=1 << 20)
    assert (j["verdict"] == [pl.verdict for pl in pls]).all()
    assert (j["fail_op"] == [pl.fail_op for pl in pls]).all()
    return pls, ops, off, j


def same_as_oracle(name, r, fields=("verdict", "fail_op", "fail_prefix_end")):
    pls, _, _, j = batch(name)
    for f in fields:
        bad = np.nonzero(r[f] != j[f])[0]
        assert len(bad) == 0, (f, len(bad), [(pls[k].tag, int(r[f][k]), int(j[f][k]))
                                             for k in bad[:8]])


def same_fields(pls, got, want, fields=ALL_FIELDS):
    for f in fields:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, len(bad), [(pls[k].tag, int(got[f][k]), int(want[f][k]))
                                             for k in bad[:8]])


@pytest.mark.parametrize("name", SHORT + LONG)
def test_check_two_pass_and_fused(ctx, monkeypatch, name):
    """lc_check with LC_FUSED=0 and 1: equal results, witnesses and kinds, the
    oracle's answers, every witness certified, and a linearization of every
    valid key (FULL) and of the prefix before every failing return (PREFIX)."""
    _, ops, off, _ = batch(name)
    r, wit, kind = both_paths(ctx, monkeypatch, ops, off)
    same_as_oracle(name, r)
    certify(ops, off, r, wit, kind)
    assert (kind == np.where(r["verdict"] == 1, abi.LC_WITNESS_FULL, abi.LC_WITNESS_PREFIX)).all()


@pytest.mark.parametrize("path", ["check32-0", "check32-1", "check16"])
@pytest.mark.parametrize("name", SHORT)
def test_check32_and_check16(ctx, monkeypatch, name, path):
    """The same batches as 24-byte records (both fused settings) and as
    16-byte records."""
    _, ops, off, _ = batch(name)
    fn, _, fused = path.partition("-")
    if fn == "check32":
        monkeypatch.setenv("LC_FUSED", fused)
        o32, base = abi.pack32(ops, off)
        _, r = ctx.check32(o32, off, base)
    else:
        o16, base = abi.pack16(ops, off)
        _, r = ctx.check16(o16, off, base)
    same_as_oracle(name, r)


@pytest.mark.parametrize("name", LONG)
def test_gap_tier_proper(ctx, monkeypatch, name):
    """Behind a ladder past 1,024 records the gap tier proper decides every
    plant.  gap_tier_kernel reports the gap count of the whole key's decision
    as max_frontier and its matching passes as configs_explored (for an
    invalid key, with the probes' added): the planted gap count on every key;
    one pass on a valid chain (the augmenting path repairs first-fit within
    the one matching), at least two on a valid coupled key (a branch
    happened).  The matching in the HBM workspace (LC_GAP_LDS=0) gives the
    same in every field; so does the plain-order rerun
    (LC_GAP_PREF_BUDGET=1) in every field but configs_explored: the rerun's
    matching passes are counted there and it branches in another order
    (measured: equal on every chain and pending plant, which never branch;
    on coupled G=65 ats=63 2 passes against 67, on its val@100 twin of G=129
    2,563 against 1,965)."""
    pls, ops, off, _ = batch(name)
    for v in ("LC_GAP_LDS", "LC_GAP_PREF_BUDGET"):
        monkeypatch.delenv(v, raising=False)
    _, r = ctx.check(ops, off)
    st = ctx.stats()
    same_as_oracle(name, r)
    assert st["n_jit_keys"] == 0 and st["n_hbm_keys"] == 0
    for k, pl in enumerate(pls):
        if " dup=1" in pl.tag:
            continue  # two :ok writes of one version: the skeleton fails before any gap is counted
        assert r["max_frontier"][k] == pg.shape(pl.recs)[0], (pl.tag, int(r["max_frontier"][k]))
        if pl.verdict == 1 and pl.family == "coupled" and "ats= " not in pl.tag:
            assert r["configs_explored"][k] >= 2, (pl.tag, int(r["configs_explored"][k]))
        if pl.verdict == 1 and pl.family == "chain":
            assert r["configs_explored"][k] == 1, (pl.tag, int(r["configs_explored"][k]))
    monkeypatch.setenv("LC_GAP_LDS", "0")
    _, hbm = ctx.check(ops, off)
    monkeypatch.delenv("LC_GAP_LDS")
    same_fields(pls, hbm, r)
    monkeypatch.setenv("LC_GAP_PREF_BUDGET", "1")
    _, plain = ctx.check(ops, off)
    monkeypatch.delenv("LC_GAP_PREF_BUDGET")
    same_fields(pls, plain, r, [f for f in ALL_FIELDS if f != "configs_explored"])


def test_one_wave_workgroups(ctx, monkeypatch):
    """More than 1,024 keys for the gap tier, none longer than 256 records:
    one-wave workgroups.  The short plants past fast_gap's limits (those are
    handed over), repeated; every copy gets the answer of the 256-thread run
    of one copy each."""
    monkeypatch.setenv("LC_FUSED", "0")
    pls = [pl for name in SHORT for pl in plants(name) if len(pl.recs) <= 256
           and (pg.shape(pl.recs)[0] > pg.K_FG_MAX_GAPS or pg.shape(pl.recs)[1] > pg.K_FG_MAX_OPS)]
    assert len(pls) >= 40 and any(pl.verdict == 0 for pl in pls)
    ops, off = pack_keys([pl.recs for pl in pls])
    _, one = ctx.check(ops, off)
    assert (one["verdict"] == [pl.verdict for pl in pls]).all()
    assert (one["fail_op"] == [pl.fail_op for pl in pls]).all()
    reps = 1100 // len(pls) + 1
    ops, off = pack_keys([pl.recs for pl in pls] * reps)
    _, r = ctx.check(ops, off)
    assert len(r) > 1024 and ctx.stats()["n_jit_keys"] == 0
    for i in range(reps):
        same_fields(pls, r[i * len(pls):(i + 1) * len(pls)], one)


@pytest.mark.parametrize("name", ["longer", "mid"])
def test_wide_workgroups_and_multisection(ctx, monkeypatch, name):
    """The group "longer": at most 64 keys, all of 2,048 records or more:
    512-thread workgroups and multisection rounds, with pending's invalid
    plants among them — the failing return the key's first (no witness
    pass), second, a middle one and the last.  The group "mid": the longest
    key between 1,025 and 2,047 records: 256 threads, multisection rounds."""
    pls, ops, off, _ = batch(name)
    longest = max(len(pl.recs) for pl in pls)
    if name == "longer":
        assert len(pls) <= 64 and min(len(pl.recs) for pl in pls) >= 2048
    else:
        assert len(pls) <= 64 and 1025 <= longest <= 2047
    r, wit, kind = both_paths(ctx, monkeypatch, ops, off)
    same_as_oracle(name, r)
    certify(ops, off, r, wit, kind)
    assert (kind == np.where(r["verdict"] == 1, abi.LC_WITNESS_FULL, abi.LC_WITNESS_PREFIX)).all()


@pytest.mark.parametrize("limit", ["gaps", "ops", "stash", "stash wave3"])
def test_handoff_at_the_crash_light_limits(ctx, monkeypatch, limit):
    """The valid plants within a limit of fast_gap are decided where the
    version order ran (the fused run spends no time in the gap tier); the
    valid plants just past it are handed over (it does).  The answers are
    right on both sides, for the invalid twins too."""
    monkeypatch.setenv("LC_FUSED", "1")
    for side in ("in", "past"):
        name = "lim:%s %s" % (side, limit)
        pls, ops, off, _ = batch(name)
        _, r = ctx.check(ops, off)
        same_as_oracle(name, r)
        valid = [pl for pl in pls if pl.verdict == 1]
        assert valid
        vops, voff = pack_keys([pl.recs for pl in valid])
        _, rv = ctx.check(vops, voff)
        st = ctx.stats()
        assert (rv["verdict"] == 1).all()
        assert st["n_jit_keys"] == 0 and st["n_hbm_keys"] == 0
        assert (st["gap_kernel_ms"] == 0) == (side == "in"), (name, st["gap_kernel_ms"])


@pytest.mark.parametrize("where", ["longest-fits", "longest-retry", "shorter", "mgr"])
def test_matching_at_the_lds_reserve(ctx, monkeypatch, where):
    """G = n_opt on either side of match_lds_bytes(G, n_opt) = kMatchReserve
    (89: 8,160 B fits; 90: 8,240 B does not).  Each pair (a valid key and its
    invalid twin, equally long) as the longest keys of a batch of their own:
    the skeleton is in LDS with exactly the reserve left, so the 89-gap
    matching runs in the last 8,192 B of the allocation and the 90-gap one
    retries with the skeleton in HBM.  "shorter": all four beside a longer
    key, which sizes the LDS: both matchings fit (no retry).  "mgr": two
    class-mode keys (n_opt >= 128) beside a key of pg.MGR_LONGEST records,
    one with room in LDS for the per-op copies of matched gap records
    (mgr_room) and one without; as a batch's longest key no class-mode key
    has that room (planted_gap.limit_plants), so mgr_room has no such edge."""
    monkeypatch.setenv("LC_FUSED", "0")
    pls = list(pg.limit_plants()["mgr" if where == "mgr" else "reserve"])
    if where.startswith("longest"):
        fit = pg.RESERVE_FIT + (where == "longest-retry")
        pls = [pl for pl in pls if pg.shape(pl.recs) == (fit, fit)]
        n = len(pls[0].recs)
        assert len(pls) == 2 and all(len(pl.recs) == n for pl in pls)
        assert (pg.match_lds_bytes(fit, fit) <= pg.lds_room(n, n) == pg.K_MATCH_RESERVE) == \
            (where == "longest-fits")
    elif where == "shorter":
        pls = pls + [pg.chain(3, 2, 600, 1)]
        longest = len(pls[-1].recs)
        assert longest > 600 and all(pg.match_lds_bytes(*pg.shape(pl.recs)) <=
                                     pg.lds_room(len(pl.recs), longest) for pl in pls)
    else:
        pls = pls + [pg.chain(3, 2, pg.MGR_LONGEST - 9, 1)]
        assert len(pls[-1].recs) == pg.MGR_LONGEST
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=16)
    assert (j["verdict"] == [pl.verdict for pl in pls]).all()
    _, r, wit, kind = ctx.check(ops, off, witness=True)
    same_fields(pls, r, j, ("verdict", "fail_op", "fail_prefix_end"))
    certify(ops, off, r, wit, kind)


@pytest.mark.parametrize("name", SHORT + LONG + ("longer",))
def test_certificates(ctx, name):
    """One call with certificates per batch: oracle/cert.c accepts every
    invalid key's, and every valid key carries none."""
    _, ops, off, _ = batch(name)
    _, r, _, _, cert, cset = ctx.check(ops, off, witness=True, certificate=True)
    same_as_oracle(name, r)
    st = oracle.check_certificate(ops, off, cert.reshape(-1), cset, r, n_threads=16)
    assert (st == np.where(r["verdict"] == 0, oracle.CERT_OK, oracle.CERT_NONE)).all(), \
        [(batch(name)[0][k].tag, int(st[k]), cert[k].tolist()) for k in
         np.nonzero(st != np.where(r["verdict"] == 0, oracle.CERT_OK, oracle.CERT_NONE))[0][:5]]
