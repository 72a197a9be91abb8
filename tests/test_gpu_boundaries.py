"""The version-order decision (check_kernel.hip, fast_key) at every lane, row,
wave and chunk edge: tests/planted.py's keys — one violation each, between
adjacent positions that straddle a thread (4), row (64) or wave (256)
boundary of timing_fails' prefix maximum, at the last positions below M, at
the record counts around the LDS clear's guard — through every kernel that
instantiates fast_key (fast_tier_kernel, gap_light_kernel, the fused kernels,
the 24-byte kernels, the resident grid), and past 1,024 records through the
gap tier proper.  Each batch mixes lengths, long and short keys alternating.

Every key, no mask: verdict, fail op and failing prefix end equal the CPU
oracle's JITC search (tests/test_planted.py pins the oracle's answers to the
plants' construction).  The search alone (LC_FLAG_NO_FAST_PATH) is a second
GPU opinion."""
import functools

import numpy as np
import pytest

import oracle
import planted
from helpers import INF, pack_keys
from jepsen.etcd_amd import abi
from test_gpu_single_pass import both_paths
from test_gpu_witness import certify
from test_planted_cert import existing_certs
from test_resident import FIELDS, _dev, _launched, _run

pytestmark = pytest.mark.gpu

GROUPS = planted.FAMILIES + tuple("long%d" % n for n in planted.LONG_LENGTHS)


@functools.lru_cache(maxsize=None)
def batch(name):
    """(plants, ops, key_off, oracle results) of one group, computed once and
    left unchanged: a family's plants and the valid ladders of every length,
    long and short keys alternating."""
    if name.startswith("long"):
        pls = planted.long_plants(int(name[4:]))
    else:
        pls = planted.family_plants(name) + planted.base_plants()
    pls = planted.interleave(pls)
    ops, off = pack_keys([pl.recs for pl in pls])
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=16)
    assert (j["verdict"] == [pl.verdict for pl in pls]).all()
    assert (j["fail_op"] == [pl.fail_op for pl in pls]).all()
    return pls, ops, off, j


def same_as_oracle(name, r, fields=("verdict", "fail_op", "fail_prefix_end")):
    pls, _, _, j = batch(name)
    for f in fields:
        bad = np.nonzero(r[f] != j[f])[0]
        assert len(bad) == 0, (f, len(bad), [(pls[k].tag, int(r[f][k]), int(j[f][k]))
                                             for k in bad[:8]])


@pytest.mark.parametrize("name", GROUPS)
def test_check_two_pass_and_fused(ctx, monkeypatch, name):
    """lc_check with LC_FUSED=0 (fast_tier_kernel, then gap_light_kernel with
    first_failure) and LC_FUSED=1 (the fused pass): equal results, witnesses
    and kinds, the oracle's answers, and every witness certified."""
    pls, ops, off, _ = batch(name)
    r, wit, kind = both_paths(ctx, monkeypatch, ops, off)
    same_as_oracle(name, r)
    certify(ops, off, r, wit, kind)
    # version-pinned keys: a linearization of every valid key, of the prefix
    # before the failing return of every invalid one
    assert (kind == np.where(r["verdict"] == 1, abi.LC_WITNESS_FULL, abi.LC_WITNESS_PREFIX)).all()


@pytest.mark.parametrize("path", ["check-0", "check-1", "check32-0", "check32-1", "check16"])
@pytest.mark.parametrize("name", GROUPS)
def test_certificates_equal_the_restatement(ctx, monkeypatch, name, path):
    """Certificates asked for on the same batches, through lc_check,
    lc_check32 (LC_FUSED=0 and 1 each) and lc_check16: every invalid plant's
    (kind, a, b, c) is the one tests/cert_ref.py finds at the plant's failing
    return (none of these kinds carries a set), oracle/cert.c accepts it, and
    every valid key carries LC_CERT_NONE."""
    pls, ops, off, _ = batch(name)
    inv, certs = existing_certs(name)
    want = {pl.tag: c for pl, (_, c) in zip(inv, sorted(certs.items()))}
    fn, _, fused = path.partition("-")
    if fused:
        monkeypatch.setenv("LC_FUSED", fused)
    if fn == "check":
        _, r, _, _, cert, cset = ctx.check(ops, off, witness=True, certificate=True)
    elif fn == "check32":
        o32, base = abi.pack32(ops, off)
        _, r, _, _, cert, cset = ctx.check32(o32, off, base, certificate=True)
    else:
        o16, base = abi.pack16(ops, off)
        _, r, _, _, cert, cset = ctx.check16(o16, off, base, certificate=True)
    same_as_oracle(name, r)
    for k, pl in enumerate(pls):
        w = want[pl.tag] if pl.verdict == 0 else (abi.LC_CERT_NONE, -1, -1, 0, [])
        assert tuple(int(x) for x in cert[k]) == tuple(w[:4]) and not w[4], (pl.tag, cert[k], w)
    st = oracle.check_certificate(ops, off, cert.reshape(-1), cset, r, n_threads=16)
    assert (st == np.where(r["verdict"] == 0, oracle.CERT_OK, oracle.CERT_NONE)).all()


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("name", GROUPS)
def test_check32(ctx, monkeypatch, name, fused):
    """24-byte records: fast_tier32_kernel / fused_tier32_kernel."""
    _, ops, off, _ = batch(name)
    o32, base = abi.pack32(ops, off)
    monkeypatch.setenv("LC_FUSED", fused)
    _, r = ctx.check32(o32, off, base)
    same_as_oracle(name, r)


@pytest.mark.parametrize("name", GROUPS)
def test_check16(ctx, name):
    _, ops, off, _ = batch(name)
    o16, base = abi.pack16(ops, off)
    _, r = ctx.check16(o16, off, base)
    same_as_oracle(name, r)


@pytest.mark.parametrize("name", GROUPS)
def test_check_device_launched_and_resident(ctx, monkeypatch, name):
    """lc_check_device launched, then four consecutive calls on the same
    buffers with the resident grid allowed (fast_resident_kernel): every call
    equals the launched one in every result field."""
    pls, ops, off, _ = batch(name)
    monkeypatch.setenv("LC_FUSED", "0")
    d_ops, d_off = _dev(ops), _dev(off)
    want = _launched(ctx, d_ops, d_off, len(pls), monkeypatch)
    same_as_oracle(name, want)
    monkeypatch.setenv("LC_RESIDENT_IDLE_US", "200000")
    for i in range(4):
        got = _run(ctx, d_ops, d_off, len(pls))
        for f in FIELDS:
            bad = np.nonzero(got[f] != want[f])[0]
            assert len(bad) == 0, (i, f, [(pls[k].tag, int(got[f][k]), int(want[f][k]))
                                          for k in bad[:8]])


@pytest.mark.parametrize("name", GROUPS)
def test_search_alone(ctx, name):
    """LC_FLAG_NO_FAST_PATH: the frontier search decides every key."""
    _, ops, off, _ = batch(name)
    _, r = ctx.check(ops, off, abi.default_opts(flags=abi.LC_FLAG_NO_FAST_PATH))
    same_as_oracle(name, r, fields=("verdict", "fail_op"))


@functools.lru_cache(maxsize=None)
def valid_twins(crashed):
    """Every valid plant of at most 1,024 records, with (crash's twins) or
    without crashed writes, as a batch of its own."""
    pls = [pl for fam in planted.FAMILIES for pl in planted.family_plants(fam)]
    pls = [pl for pl in pls + list(planted.base_plants())
           if pl.verdict == 1 and any(r[5] == INF for r in pl.recs) == crashed]
    return (len(pls),) + pack_keys([pl.recs for pl in planted.interleave(pls)])


@pytest.mark.parametrize("fused", ["0", "1"])
def test_valid_twins_decided_by_the_version_order(ctx, monkeypatch, fused):
    """The valid crash-free twins never leave the version-order pass: no key
    is handed to the crash-light pass, the gap tier or the search."""
    n, ops, off = valid_twins(False)
    assert n > 500
    monkeypatch.setenv("LC_FUSED", fused)
    _, r = ctx.check(ops, off)
    st = ctx.stats()
    assert (r["verdict"] == 1).all()
    assert st["n_gap_keys"] == 0 and st["n_jit_keys"] == 0 and st["n_hbm_keys"] == 0


@pytest.mark.parametrize("fused", ["0", "1"])
def test_valid_crash_twins_decided_in_place(ctx, monkeypatch, fused):
    """The valid twins with crashed writes are decided by fast_gap where the
    version order ran: n_gap_keys counts every one as taken by the crash-light
    decision, none goes on to the search.  lc_stats does not count the gap
    tier proper apart from that decision; that it stayed idle shows in the
    fused run, where no key is handed over at all: no time is spent past the
    first pass."""
    n, ops, off = valid_twins(True)
    assert n > 50
    monkeypatch.setenv("LC_FUSED", fused)
    _, r, wit, kind = ctx.check(ops, off, witness=True)
    st = ctx.stats()
    assert (r["verdict"] == 1).all() and (kind == abi.LC_WITNESS_FULL).all()
    assert st["n_gap_keys"] == n and st["n_jit_keys"] == 0 and st["n_hbm_keys"] == 0
    if fused == "1":
        assert st["gap_kernel_ms"] == 0 and st["jit_kernel_ms"] == 0
