"""tests/planted.py pinned on the CPU, so that tests/test_gpu_boundaries.py
cannot be vacuous: every planted key gets its expected verdict from both of
the oracle's searches, its expected fail op from the one the GPU's search
tiers restate (JITC), and the same from the Python restatements of the
version-order decision (fastpath_ref) and of the gap matching (gapmatch_ref)
wherever they apply.  The oracle decides every key under its default
budgets: none is excluded."""
import numpy as np
import pytest

import fastpath_ref as fp
import gapmatch_ref as gm
import oracle
import planted
from helpers import INF, pack_keys

GROUPS = planted.FAMILIES + ("base",) + tuple("long%d" % n for n in planted.LONG_LENGTHS)


def group(name):
    if name == "base":
        return planted.base_plants()
    if name.startswith("long"):
        return planted.long_plants(int(name[4:]))
    return planted.family_plants(name)


def test_ladder_shape():
    recs = planted.ladder(9)
    assert recs == [[1, i % 7, -1, i + 1, 4 * i, 4 * i + 1] for i in range(9)]
    recs = planted.ladder(9, reads_every=3)
    assert [r[0] for r in recs] == [1, 1, 1, 0, 1, 1, 1, 0, 1]
    assert [r[4:] for r in recs] == [[4 * s, 4 * s + 1] for s in range(9)]
    assert recs[3][:4] == [0, 2, -1, 3] and recs[7][:4] == [0, 5 % 7, -1, 6]
    assert planted.n_positions(1024) == 1024 and planted.n_positions(1023, 3) == 768


def test_every_boundary_is_planted():
    """swap and far reach every listed position on both 1,000-record ladders
    (each side of every thread, row and wave boundary and the last two
    positions), and every length has its valid key and a violation in its
    last two positions."""
    swaps = {pl.tag for pl in planted.family_plants("swap")}
    fars = {pl.tag for pl in planted.family_plants("far")}
    for n, re in ((1024, 0), (1023, 3)):
        m = planted.n_positions(n, re)
        for p in planted.POSITIONS + (m - 2, m - 1):
            if p + 1 < m:
                assert "swap n=%d re=%d p=%d" % (n, re, p) in swaps
            for d in planted.FAR_D:  # p as the late holder and as the early returner
                for p0 in (p, p - d):
                    if p0 >= 0 and p0 + d < m:
                        assert "far n=%d re=%d d=%d good=0 p=%d" % (n, re, d, p0) in fars
    have = {(len(pl.recs), pl.verdict) for pl in planted.base_plants()}
    assert have == {(n, 1) for n in planted.LENGTHS}
    for fam in ("swap", "dup"):
        last = {len(pl.recs) for pl in planted.family_plants(fam)
                if pl.fail_op >= len(pl.recs) - 3}
        assert last >= {n for n in planted.LENGTHS if n >= 4}, fam
    # the lengths of the LDS clear's guard, by a read of the last version
    assert {len(pl.recs) for pl in planted.family_plants("read_past")} >= set(planted.LENGTHS)


def test_twins_differ_in_one_field():
    """An invalid plant built with good=False and its valid twin are the
    same records but for one field."""
    n_pairs = 0
    for fam in ("far", "read_val", "cas_exp", "read_stale", "read_future"):
        by_tag = {pl.tag: pl for pl in planted.family_plants(fam)}
        for tag, bad in by_tag.items():
            if "good=0" not in tag:
                continue
            good = by_tag[tag.replace("good=0", "good=1")]
            assert (bad.verdict, good.verdict) == (0, 1) and len(bad.recs) == len(good.recs)
            diff = sum(x != y for a, b in zip(bad.recs, good.recs) for x, y in zip(a, b))
            assert diff == 1, tag
            n_pairs += 1
    assert n_pairs > 400


@pytest.mark.parametrize("name", GROUPS)
def test_oracle_agrees_with_every_plant(name):
    pls = group(name)
    ops, off = pack_keys([pl.recs for pl in pls])
    want_v = np.array([pl.verdict for pl in pls])
    want_f = np.array([pl.fail_op for pl in pls])
    assert len(pls) >= 30 and (name == "base" or (want_v == 0).sum() >= 30)
    assert ((want_v == 0) == (want_f >= 0)).all()
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8)
    _, w = oracle.check(ops, off, algo=oracle.WGL, n_threads=8)
    bad = np.nonzero((j["verdict"] != want_v) | (w["verdict"] != want_v) |
                     (j["fail_op"] != want_f))[0]
    assert len(bad) == 0, [(pls[k].tag, int(j["verdict"][k]), int(w["verdict"][k]),
                            int(j["fail_op"][k])) for k in bad[:5]]
    # the fail op's return is the end of the failing prefix
    inv = np.nonzero(want_v == 0)[0]
    assert all(j["fail_prefix_end"][k] == pls[k].recs[pls[k].fail_op][5] for k in inv)


@pytest.mark.parametrize("name", GROUPS)
def test_restatements_agree_with_every_plant(name):
    """fastpath_ref decides every crash-free key (and only those) and names
    the fail op of every invalid one without declining; gapmatch_ref decides
    every key and bisects to the same fail op."""
    n_fp = 0
    for pl in group(name):
        crashed = any(r[5] == INF for r in pl.recs)
        d = fp.decide(pl.recs)
        assert d == (None if crashed else pl.verdict), pl.tag
        assert gm.decide(pl.recs) == pl.verdict, pl.tag
        if pl.verdict == 0:
            if not crashed:
                ff = fp.first_failure(pl.recs)
                assert ff is not None and ff[0] == pl.fail_op, (pl.tag, ff and ff[0])
                n_fp += 1
            assert gm.first_failure(pl.recs) == (pl.fail_op, pl.recs[pl.fail_op][5]), pl.tag
    assert name in ("base", "crash") or n_fp >= 30
