"""tests/planted_cert.py pinned on the CPU, so that
tests/test_gpu_cert_edges.py cannot be vacuous: every plant gets its expected
verdict from both of the oracle's searches and its fail op and cut from JITC
(default budgets, no plant excluded); the finder's restatement
(tests/cert_ref.py) returns exactly the certificate the plant was built to
get — derived by hand in the builder — and oracle/cert.c accepts it; on the
valid twin and on the prefix just before the failing return the finder finds
nothing; and the plant list covers every edge it is meant to.  The invalid
plants of tests/planted.py are certified the same way."""
import functools

import numpy as np
import pytest

import cert_ref
import oracle
import planted
import planted_cert as pc
from helpers import INF, pack_keys

FAMILIES = pc.FAMILIES


def by_opts(pls):
    """{(init_version, init_value): indices} of the plants."""
    out = {}
    for i, pl in enumerate(pls):
        out.setdefault((pl.v0, pl.init), []).append(i)
    return out


@functools.lru_cache(maxsize=None)
def decided(family):
    """(plants, JITC results, WGL verdicts) of one family, computed once."""
    pls = pc.family_plants(family)
    j = np.zeros(len(pls), dtype=oracle.RESULT_DTYPE)
    w = np.zeros(len(pls), dtype=np.int64)
    for (v0, init), idx in by_opts(pls).items():
        ops, off = pack_keys([pls[i].recs for i in idx])
        _, a = oracle.check(ops, off, algo=oracle.JITC, n_threads=8, init_version=v0,
                            init_value=init)
        _, b = oracle.check(ops, off, algo=oracle.WGL, n_threads=8, init_version=v0,
                            init_value=init)
        j[idx] = a
        w[idx] = b["verdict"]
    return pls, j, w


@functools.lru_cache(maxsize=None)
def found(family):
    """cert_ref's certificate of every invalid plant at the oracle's cut."""
    pls, j, _ = decided(family)
    return {i: cert_ref.find([tuple(r) for r in pl.recs], int(j["fail_prefix_end"][i]),
                             pl.v0, pl.init)
            for i, pl in enumerate(pls) if pl.verdict == 0}


def pinned_key(recs):
    return not any(r[5] != INF and r[3] == -1 and (r[0] != 0 or r[1] != -1) for r in recs)


@pytest.mark.parametrize("family", FAMILIES)
def test_plants_are_well_formed(family):
    """Version-pinned keys, records in call order, distinct event times, and
    every invalid plant next to its twin, which differs in one record."""
    pls = pc.family_plants(family)
    assert len({pl.tag for pl in pls}) == len(pls)
    by_tag = {pl.tag: pl for pl in pls}
    n_twins = 0
    for pl in pls:
        assert pinned_key(pl.recs), pl.tag
        calls = [r[4] for r in pl.recs]
        assert calls == sorted(calls) and calls[0] == pl.t0, pl.tag
        ev = calls + [r[5] for r in pl.recs if r[5] != INF]
        assert len(set(ev)) == len(ev) and all(r[5] > r[4] for r in pl.recs), pl.tag
        assert (pl.verdict == 0) == (pl.fail_op >= 0)
        twin = by_tag.get(pl.tag.replace("good=0", "good=1"))
        if pl.verdict == 0 and twin is not None:
            assert twin.verdict == 1 and len(twin.recs) == len(pl.recs)
            assert sum(a != b for a, b in zip(pl.recs, twin.recs)) == 1, pl.tag
            n_twins += 1
    bad = [pl.tag for pl in pls if pl.verdict == 0]
    # no twin: the two-clash PAIR plants (two fields would differ)
    lone = [t for t in bad if t.replace("good=0", "good=1") not in by_tag]
    assert all("two=1" in t for t in lone), lone[:5]
    assert n_twins >= len(bad) - len(lone) and n_twins >= 3


@pytest.mark.parametrize("family", FAMILIES)
def test_oracle_agrees_with_every_plant(family):
    pls, j, w = decided(family)
    want_v = np.array([pl.verdict for pl in pls])
    want_f = np.array([pl.fail_op for pl in pls])
    bad = np.nonzero((j["verdict"] != want_v) | (w != want_v) | (j["fail_op"] != want_f))[0]
    assert len(bad) == 0, [(pls[k].tag, int(j["verdict"][k]), int(w[k]), int(j["fail_op"][k]))
                           for k in bad[:5]]
    # the fail op's return is the end of the failing prefix
    assert all(j["fail_prefix_end"][k] == pls[k].recs[pls[k].fail_op][5]
               for k in np.nonzero(want_v == 0)[0])


@pytest.mark.parametrize("family", FAMILIES)
def test_restatement_finds_the_planted_certificate(family):
    """cert_ref.find at the cut: the plant's hand-derived (kind, a, b, c) and
    set, entry for entry."""
    pls, _, _ = decided(family)
    for i, got in found(family).items():
        pl = pls[i]
        assert tuple(got[:4]) == pl.cert and tuple(got[4]) == pl.cset, \
            (pl.tag, got[:4], got[4][:8], pl.cert, pl.cset[:8])


def cert_arrays(pls, certs):
    """certs: {plant index: (kind, a, b, c, set)} -> the lc_aux arrays."""
    off = np.concatenate([[0], np.cumsum([len(pl.recs) for pl in pls])])
    cert = np.tile(np.array(pc.NO_CERT, dtype=np.int32), len(pls))
    cset = np.zeros(off[-1], dtype=np.int32)
    for i, (kind, a, b, c, ps) in certs.items():
        cert[4 * i: 4 * i + 4] = (kind, a, b, c)
        cset[off[i]: off[i] + len(ps)] = ps
    return cert, cset


@pytest.mark.parametrize("family", FAMILIES)
def test_checker_accepts_every_certificate(family):
    pls, j, _ = decided(family)
    certs = found(family)
    cert, cset = cert_arrays(pls, certs)
    off = np.concatenate([[0], np.cumsum([len(pl.recs) for pl in pls])])
    for (v0, init), idx in by_opts(pls).items():
        ops, koff = pack_keys([pls[i].recs for i in idx])
        c = np.concatenate([cert[4 * i: 4 * i + 4] for i in idx])
        s = np.concatenate([cset[off[i]: off[i + 1]] for i in idx])
        st = oracle.check_certificate(ops, koff, c, s, j[idx], init_version=v0, init_value=init)
        for n, i in enumerate(idx):
            want = oracle.CERT_OK if pls[i].cert != pc.NO_CERT else oracle.CERT_NONE
            assert st[n] == want, (pls[i].tag, int(st[n]), pls[i].cert)


@pytest.mark.parametrize("family", FAMILIES)
def test_nothing_found_on_linearizable_prefixes(family):
    """The valid twin's whole history, and the invalid plant's prefix just
    before its failing return: no certificate."""
    pls, j, _ = decided(family)
    n = 0
    for i, pl in enumerate(pls):
        recs = [tuple(r) for r in pl.recs]
        rets = sorted(r[5] for r in recs if r[5] != INF)
        if pl.verdict == 1:
            cut = max(recs[-1][4], rets[-1])
        else:
            earlier = [x for x in rets if x < j["fail_prefix_end"][i]]
            if not earlier:
                continue
            cut = earlier[-1]
        got = cert_ref.find(recs, cut, pl.v0, pl.init)
        assert got[0] == cert_ref.NONE, (pl.tag, cut, got[:4])
        n += 1
    # (an invalid plant that fails at its first return has no earlier prefix)
    assert n >= sum(pl.verdict == 1 for pl in pls) >= 3


def test_every_boundary_is_planted():
    """The plant list itself: every edge the families are meant to cover has
    a plant."""
    tags = {pl.tag: pl for pl in pc.all_plants() if pl.verdict == 0}
    has = lambda fam, rest: "%s %s good=0 t0=0 v0=0" % (fam, rest) in tags
    # ORDER between mutations: L = 256 .. 1,024 (per = 1, 2, 2, 3, 4); every
    # thread edge straddled; each side of every wave edge and of three thread
    # edges, for p and for p+d, at every distance
    assert [(L + 255) // 256 for L in pc.ORDER_L] == [1, 2, 2, 3, 4]
    for L in pc.ORDER_L:
        per, M = (L + 255) // 256, L - 1
        for t in range(1, 256):
            assert per * t + 1 >= M or has("order_mut", "L=%d p=%d d=1" % (L, per * t - 1))
        edges = pc.order_edges(L)
        assert set(edges) >= {64 * per * w for w in (1, 2, 3)} | {per, 255 * per}
        for e in edges:
            for d in (1, 2, 64 * per, 192 * per):
                for p in (e - 1, e, e - d - 1, e - d):
                    if p >= 0 and p + d < M:
                        assert has("order_mut", "L=%d p=%d d=%d" % (L, p, d)), (L, p, d)
        # the suffix minimum arrives from a later wave
        assert any(pl.family == "order_mut" and (" L=%d " % L) in pl.tag and
                   pl.cert[1] - pl.cert[2] >= 64 * per for pl in tags.values())
    # CLAIMS and PAIR: finders in different 256-strides
    for i1, i2 in pc.CLAIMS_AT:
        assert i1 // 256 != i2 // 256 and has("claims_far", "i1=%d i2=%d" % (i1, i2))
    assert {255, 256} <= {i for i, _ in pc.CLAIMS_AT} and {511, 512} <= {i for _, i in pc.CLAIMS_AT}
    for q in (1, 255, 256, 257):
        assert has("pair_far", "q=%d two=0" % q) and has("pair_far", "q=%d two=1" % q)
    assert has("pair_far", "q=0 at=0") and has("pair_far", "q=0 at=256")
    # the candidate list: every n, every n_u that fits, candidates from
    # record 0 and at the key's end
    for n in pc.ULIST_N:
        for nu in pc.ULIST_NU:
            if 2 * nu <= n:
                for lead in {0, n - 2 * nu}:
                    assert has("ulist", "m=%d inter lead=%d n=%d" % (nu, lead, n)), (n, nu, lead)
    for m in pc.HALL_ALL_M:
        assert any(pl.family == "hall_all" and pl.cert[3] == m for pl in tags.values()), m
    for p in pc.DEADLINE_P:
        for how in ("ulist", "pin", "ulist_ok", "pin_ok"):
            assert has("deadline", "p=%d %s" % (p, how))
    for g in pc.PINNED_G:
        for ops in (1, 2, 3):
            for cas in (0, 1):
                assert has("pinned", "g=%d ops=%d cas=%d" % (g, ops, cas))
    assert has("hall_one", "g=255") and has("hall_one", "lo=10 hi=300 top=310")
    for q in pc.PAIR_OPEN_Q:
        assert has("pair_open", "q=%d" % q)
    # PROOF: split depths 1..4 at both conflict sizes, every n % 4, the lanes
    # of the wave, the node cap from both sides, no token room (the frame cap
    # from both sides: proof_deep, below)
    proofs = [pl for pl in tags.values() if pl.family == "proof"]
    shape = lambda pl: tuple(int(x.split("=")[1]) for x in pl.tag.split()[1:5])  # k, c, chain, n
    for c in (3, 4):
        for depth in (1, 2, 3, 4):
            sizes = [shape(pl)[3] for pl in proofs
                     if shape(pl)[1] == c and pc.proof_depth(shape(pl)[0], c) == depth and
                     shape(pl)[2] == 0 and pl.cert[0] == pc.PROOF]
            if c == 4 and depth == 1:
                continue  # (a conflict of four positions splits twice)
            assert {n % 4 for n in sizes} == {0, 1, 2, 3}, (c, depth, sizes)
            # the frame cap equal to the depth wherever a key of 4 depth + 1
            # records holds the shape and its tokens, and one above it
            frames = {cert_ref.n_frames(n) - depth for n in sizes}
            kf = depth - (c - 2)
            fits = max(pc.proof_size(kf, c), len(pc.proof_tokens(0, kf, c))) <= 4 * depth + 1
            assert frames >= ({0, 1} if fits else {min(frames)}), (c, depth, frames)
            assert fits or (c, depth) in ((3, 1), (4, 2), (4, 4))
        for ng in pc.PROOF_OPEN:
            assert any(shape(pl)[1] == c and sum(shape(pl)[:3]) == ng for pl in proofs)
        lo, hi = pc.NODE_CAP_K[c]
        assert pc.proof_nodes(0, lo, c) <= pc.PROOF_NODES < pc.proof_nodes(0, hi, c)
        for kf, kind in ((lo, pc.PROOF), (hi, pc.NONE)):
            pl = [pl for pl in proofs if shape(pl)[:3] == (kf, c, 0)]
            assert len(pl) == 1 and pl[0].cert[0] == kind and len(pl[0].recs) >= \
                len(pc.proof_tokens(0, kf, c)) * (kind == pc.PROOF)
        assert any(shape(pl)[1] == c and pl.cert == pc.NO_CERT and
                   len(pl.recs) < len(pc.proof_tokens(0, shape(pl)[0], c)) for pl in proofs)
    # PROOF against the frame cap: split depth one above it (no certificate),
    # equal to it and one below it (a proof of depth tokens), each at every n % 4
    deep = [pl for pl in tags.values() if pl.family == "proof_deep" and pl.t0 == pl.v0 == 0]
    for over, kind in ((1, pc.NONE), (0, pc.PROOF), (-1, pc.PROOF)):
        at = [pl for pl in deep
              if int(pl.tag.split()[1][2:]) - cert_ref.n_frames(len(pl.recs)) == over]
        assert {len(pl.recs) % 4 for pl in at} == {0, 1, 2, 3}, (over, [pl.tag for pl in at])
        assert all(pl.cert[0] == kind for pl in at), over
        assert all(pl.cert[3] == int(pl.tag.split()[1][2:]) for pl in at if kind == pc.PROOF)
    # every certificate again on the other bases
    kinds = lambda pls: {(pl.family, pl.cert[0], pl.cert[3] > 1) for pl in pls}
    first = kinds(pl for pl in tags.values() if (pl.t0, pl.v0) == (0, 0))
    for t0, v0, init in pc.BASES:
        there = [pl for pl in tags.values() if (pl.t0, pl.v0, pl.init) == (t0, v0, init)]
        assert {k[:2] for k in kinds(there)} >= {k[:2] for k in first if k[1] != pc.NONE}, (t0, v0)
    assert cert_ref.PROOF_NODES == pc.PROOF_NODES


def test_search_counts_as_planted():
    """The restated search's node count, deepest frame stack and tokens are
    the builders' closed forms (planted_cert.proof_nodes / proof_depth /
    proof_tokens): 1,535 nodes at k_free = 8 and 3,071 at 9 (conflict = 3),
    1,087 at 6 and 2,175 at 7 (conflict = 4) — the node cap of 2,048 lies
    between."""
    assert [pc.proof_nodes(0, k, 3) for k in pc.NODE_CAP_K[3]] == [1535, 3071]
    assert [pc.proof_nodes(0, k, 4) for k in pc.NODE_CAP_K[4]] == [1087, 2175]
    for kf, c, chain in ((0, 3, 0), (2, 3, 0), (3, 3, 40), (1, 4, 0), (2, 4, 59), (8, 3, 0), (6, 4, 0)):
        pl = pc.proof_key(kf, c, chain=chain, pad=1100)
        st = {}
        got = cert_ref.find([tuple(r) for r in pl.recs], pl.recs[pl.fail_op][5], stats=st,
                            proof_budget=1 << 20)
        assert got[0] == cert_ref.PROOF
        assert st == {"nodes": pc.proof_nodes(chain, kf, c), "depth": pc.proof_depth(kf, c),
                      "tokens": len(pc.proof_tokens(chain, kf, c))}, (kf, c, chain, st)


# what the finder's stages make of tests/planted.py's invalid plants
EXISTING_KINDS = {
    "swap": {"unreach"}, "far": {"unreach"}, "hole": {"unreach"}, "read_past": {"unreach"},
    "read_future": {"unreach"}, "crash": {"unreach"}, "dup": {"dup"}, "cas_exp": {"pair"},
    "read_val": {"pair", "claims", "unreach"}, "read_stale": {"order"},
    "long1025": {"unreach", "pair", "dup", "order", "claims"}, "long3001": {"unreach", "pair"},
}


@functools.lru_cache(maxsize=None)
def existing_certs(name):
    """(invalid plants of one group of tests/planted.py, cert_ref's
    certificates at the plants' own cuts), computed once; the GPU tests
    compare the device's with them."""
    pls = planted.long_plants(int(name[4:])) if name.startswith("long") else \
        planted.family_plants(name)
    pls = [pl for pl in pls if pl.verdict == 0]
    return pls, {i: cert_ref.find([tuple(r) for r in pl.recs], pl.recs[pl.fail_op][5])
                 for i, pl in enumerate(pls)}


@pytest.mark.parametrize("name", sorted(EXISTING_KINDS))
def test_existing_plants_are_certified(name):
    pls, certs = existing_certs(name)
    kinds = {oracle.CERT_KINDS[c[0]] for c in certs.values()}
    assert not any(c[4] for c in certs.values())  # (no kind with a set)
    assert kinds == EXISTING_KINDS[name], kinds
    if name == "read_stale":  # always with a read as the lower bound's op
        assert all(pls[i].recs[c[1]][0] == 0 for i, c in certs.items())
    ops, off = pack_keys([pl.recs for pl in pls])
    res = np.zeros(len(pls), dtype=oracle.RESULT_DTYPE)
    res["fail_prefix_end"] = [pl.recs[pl.fail_op][5] for pl in pls]
    cert = np.array([c[:4] for _, c in sorted(certs.items())], dtype=np.int32).reshape(-1)
    st = oracle.check_certificate(ops, off, cert, np.zeros(len(ops), dtype=np.int32), res)
    assert (st == oracle.CERT_OK).all(), [pls[k].tag for k in np.nonzero(st != oracle.CERT_OK)[0][:5]]
