"""The certificate finder (cert.hip, cert_kernel) at every edge of its stages:
tests/planted_cert.py's keys — one infeasibility each, built to be found by
one stage at one edge of that stage's ownership pattern — through lc_check
(two-pass and fused), lc_check32 and lc_check16 with certificates asked for.

Every key: the verdict, fail op and failing prefix end are the plant's; the
device's (kind, a, b, c) and the first c entries of its set equal the
certificate the plant was built to get and the one tests/cert_ref.py finds
(tests/test_planted_cert.py pins those two to each other and to the CPU
oracle); oracle/cert.c accepts it; valid twins carry LC_CERT_NONE.  Then the
layout: the same keys interleaved with valid, empty and odd-length ones get
what each gets in a call of its own, and a PROOF search never touches the
next key's arrays."""
import functools

import numpy as np
import pytest

import oracle
import planted_cert as pc
from helpers import N, R, W, pack_keys
from jepsen.etcd_amd import abi
from test_planted_cert import by_opts, found

pytestmark = pytest.mark.gpu


def sets_with_kind(c):
    """HALL and PROOF certificates carry c set entries."""
    return c[0] in (abi.LC_CERT_HALL, abi.LC_CERT_PROOF)


def same_certificates(pls, off, want, cert, cset, who=""):
    """cert (n, 4) / cset of one call against want: {plant index: (kind, a, b,
    c, set)} (the others: none)."""
    for i, pl in enumerate(pls):
        w = want.get(i, pc.NO_CERT + ((),))
        got = tuple(int(x) for x in cert[i])
        assert got == tuple(w[:4]), (who, pl.tag, got, w[:4])
        if sets_with_kind(got):
            s = [int(x) for x in cset[off[i]: off[i] + got[3]]]
            assert s == list(w[4]), (who, pl.tag, s[:8], list(w[4])[:8])


def planted_certs(pls):
    return {i: pl.cert + (pl.cset,) for i, pl in enumerate(pls) if pl.verdict == 0}


def same_results(pls, r, who=""):
    want_v = np.array([pl.verdict for pl in pls])
    want_f = np.array([pl.fail_op for pl in pls])
    want_e = np.array([pl.recs[pl.fail_op][5] if pl.verdict == 0 else 0 for pl in pls])
    bad = np.nonzero((r["verdict"] != want_v) | (r["fail_op"] != want_f) |
                     ((want_v == 0) & (r["fail_prefix_end"] != want_e)))[0]
    assert len(bad) == 0, (who, [(pls[k].tag, int(r["verdict"][k]), int(r["fail_op"][k]))
                                 for k in bad[:5]])


@functools.lru_cache(maxsize=None)
def packed(family):
    """Per (init_version, init_value) of the family: (plant indices, ops,
    key_off), computed once and left unchanged."""
    pls = pc.family_plants(family)
    return tuple((o, idx) + pack_keys([pls[i].recs for i in idx])
                 for o, idx in by_opts(pls).items())


def run_family(family, call, who):
    """call(ops, off, opts) -> (r, cert, cset): results and certificates of
    every plant equal the planted ones, cert_ref's, and pass the checker."""
    pls_all = pc.family_plants(family)
    ref = found(family)
    for (v0, init), idx, ops, off in packed(family):
        pls = [pls_all[i] for i in idx]
        r, cert, cset = call(ops, off, abi.default_opts(init_version=v0, init_value=init))
        same_results(pls, r, who)
        same_certificates(pls, off, planted_certs(pls), cert, cset, who)
        same_certificates(pls, off, {n: ref[i] for n, i in enumerate(idx) if i in ref},
                          cert, cset, who + " cert_ref")
        st = oracle.check_certificate(ops, off, cert.reshape(-1), cset, r, init_version=v0,
                                      init_value=init, n_threads=16)
        want = np.array([oracle.CERT_OK if pl.cert != pc.NO_CERT else oracle.CERT_NONE
                         for pl in pls])
        assert (st == want).all(), (who, [pls[k].tag for k in np.nonzero(st != want)[0][:5]])
        assert (cert[r["verdict"] != 0][:, 0] == abi.LC_CERT_NONE).all()


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_check_two_pass_and_fused(ctx, monkeypatch, family):
    """lc_check with LC_FUSED=0 and LC_FUSED=1: the planted certificates, and
    every witness certified."""
    for mode in ("0", "1"):
        monkeypatch.setenv("LC_FUSED", mode)

        def call(ops, off, opts):
            _, r, wit, kind, cert, cset = ctx.check(ops, off, opts, witness=True, certificate=True)
            st, _ = oracle.check_witness(ops, off, wit, kind, results=r, n_threads=16,
                                         init_version=opts.init_version,
                                         init_value=opts.init_value)
            bad = np.nonzero((kind != abi.LC_WITNESS_NONE) & (st != oracle.WIT_OK))[0]
            assert len(bad) == 0, bad[:5]
            assert (kind == np.where(r["verdict"] == 1, abi.LC_WITNESS_FULL,
                                     abi.LC_WITNESS_PREFIX)).all()
            return r, cert, cset

        run_family(family, call, "fused=" + mode)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("family", pc.FAMILIES)
def test_check32(ctx, monkeypatch, family, fused):
    monkeypatch.setenv("LC_FUSED", fused)

    def call(ops, off, opts):
        o32, base = abi.pack32(ops, off)
        _, r, _, _, cert, cset = ctx.check32(o32, off, base, opts, certificate=True)
        return r, cert, cset

    run_family(family, call, "check32 fused=" + fused)


@pytest.mark.parametrize("family", pc.FAMILIES)
def test_check16(ctx, family):
    """Every plant's values fit the 16-byte records."""
    def call(ops, off, opts):
        p16 = abi.pack16(ops, off)
        assert p16 is not None
        _, r, _, _, cert, cset = ctx.check16(p16[0], off, p16[1], opts, certificate=True)
        return r, cert, cset

    run_family(family, call, "check16")


# ---- layout -----------------------------------------------------------------
STALE = [[W, 1, N, 1, 0, 2], [R, N, N, 0, 4, 6]]  # a read of the initial version after w1
STALE_PLANT = pc.Plant("fill", "stale", STALE, 0, 1, (abi.LC_CERT_ORDER, 1, 0, 0), (), 0, 0, N)


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Plants of every family (first call 0, initial version 0) between
    valid, empty and odd-length keys: the keys' workspace offset rb + 2 key
    takes both parities.  A proof plant first and another last."""
    proofs = [pl for pl in pc.family_plants("proof") if pl.cert[0] == pc.PROOF]
    some = []
    for fam in pc.FAMILIES[:-1]:
        pls = pc.family_plants(fam)
        step = max(1, len(pls) // 24)
        some += pls[::step][:24] if fam != "proof" else list(pls)
    filler = [pc.Plant("fill", "empty", [], 1, -1, pc.NO_CERT, (), 0, 0, N),
              STALE_PLANT,
              pc.Plant("fill", "one", [[W, 1, N, 1, 0, 2]], 1, -1, pc.NO_CERT, (), 0, 0, N)]
    pls = [proofs[0]]
    for i, pl in enumerate(some):
        pls += [pl, filler[i % 3]]
    pls.append(proofs[-1])
    ops, off = pack_keys([pl.recs for pl in pls])
    parities = {int(off[k] + 2 * k) % 2 for k, pl in enumerate(pls) if pl.cert[0] == pc.PROOF}
    assert parities == {0, 1}
    return pls, ops, off


def test_interleaved_batch_equals_single_calls(ctx):
    """Each key's certificate and set are the planted ones, and what the
    same key gets in a call of its own."""
    pls, ops, off = mixed_batch()
    _, r, _, _, cert, cset = ctx.check(ops, off, certificate=True)
    same_results(pls, r)
    same_certificates(pls, off, planted_certs(pls), cert, cset, "batch")
    seen = {}
    for i, pl in enumerate(pls):
        if pl.verdict != 0 or pl.tag in seen:
            continue
        seen[pl.tag] = 1
        o1, f1 = pack_keys([pl.recs])
        _, r1, _, _, c1, s1 = ctx.check(o1, f1, certificate=True)
        assert all(r1[f][0] == r[f][i] for f in ("verdict", "fail_op", "fail_prefix_end"))
        assert (c1[0] == cert[i]).all(), (pl.tag, c1[0], cert[i])
        k = int(c1[0][3]) if sets_with_kind(c1[0]) else 0
        assert (s1[:k] == cset[off[i]: off[i] + k]).all(), pl.tag


def test_proof_search_stays_inside_its_key(ctx):
    """2,000 keys.  The depth-3 proof plant of 11 records fills every frame
    it has (n % 4 = 3: the size at which the frames of the old layout ran two
    ints past the key's region, onto the start of the next key's lower-bound
    array).  The first 1,000 keys alternate it with a key whose ORDER
    certificate is that lower bound of index 0: a stale read of the initial
    version.  In the other 1,000 the proof plant is followed by itself (the
    next key's search keeps its log of assumed positions in the same two
    ints, at the same moment) and then by the stale read.  Every key gets
    its certificate."""
    proof = pc.proof_key(2, 3)
    assert len(proof.recs) == 11 and pc.proof_depth(2, 3) == 3 == (11 + 2) // 4
    plants = [proof, STALE_PLANT] * 500 + [proof, proof, STALE_PLANT, proof] * 250
    ops, off = pack_keys([pl.recs for pl in plants])
    _, r, _, _, cert, cset = ctx.check(ops, off, certificate=True)
    same_results(plants, r)
    want = np.array([pl.cert for pl in plants], dtype=np.int32)
    bad = np.nonzero((cert != want).any(axis=1))[0]
    assert len(bad) == 0, (len(bad), [(int(k), cert[k].tolist()) for k in bad[:5]])
    at = off[:-1][[pl is proof for pl in plants]]
    toks = cset[np.add.outer(at, np.arange(len(proof.cset)))]
    assert (toks == np.array(proof.cset, dtype=np.int32)).all()
