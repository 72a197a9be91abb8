"""tests/planted_gap.py pinned on the CPU, so that tests/test_gpu_gap_edges.py
cannot be vacuous: every planted key gets its constructed verdict from both
of the oracle's searches and its fail op from JITC, the same from the Python
restatement of the gap matching (gapmatch_ref), and the construction itself
is proved with a call-order first-fit written here (not the product's, not
the restatement's): what greedy leaves open on a chain, how long the shortest
augmenting path is, which pairs greedy violates on a coupled key.  No plant
is excluded or masked."""
import numpy as np
import pytest

import gapmatch_ref as gm
import oracle
import planted_gap as pg
from helpers import INF, C, N, R, pack_keys
from jepsen.etcd_amd import abi

GROUPS = tuple("%s-%s" % (f, v) for f in pg.FAMILIES for v in ("short", "shift", "long")) + \
    ("limits", "limits-long", "longer")


def group(name):
    fam, _, var = name.partition("-")
    if name == "longer":
        return pg.longer_plants()
    if fam == "limits":
        pls = pg.all_limit_plants()
        return pls if not var else tuple(pg.lengthen(pl, pg.LONG) for pl in pls)
    return pg.family_plants(fam, {"short": 0, "shift": pg.SHIFT, "long": pg.LONG}[var])


# ---------------------------------------------------------------------------
# the construction's own first-fit
def layout(recs, cut=None):
    """(gaps, ops, elig, before): the unpinned positions a required op needs,
    the optional mutations in call order (crashed ones; in the prefix at
    event `cut` also the :ok ones still open, pinned to their position),
    elig(g, o) by deadline, pinned position, claimed value and (where the
    value before the gap is known) CAS expectation."""
    if cut is not None:
        recs = [r[:5] + [r[5] if r[5] <= cut else INF] for r in recs if r[4] <= cut]
    recs = [r for r in recs if r[0] != R or r[5] != INF]
    pinned = {r[3] - 1: r for r in recs if r[0] != R and r[5] != INF}
    m = max(r[3] for r in recs if r[5] != INF)
    dl, claim = [INF] * (m + 1), {}
    for r in recs:
        if r[5] != INF and r[3] >= 1:
            dl[r[3] - 1] = min(dl[r[3] - 1], r[5])
            if r[0] == R and r[1] != N:
                claim[r[3] - 1] = r[1]
    for p in range(m - 1, -1, -1):
        dl[p] = min(dl[p], dl[p + 1])
    gaps = [p for p in range(m) if p not in pinned]
    ops = [r for r in recs if r[0] != R and r[5] == INF]

    def before(p):
        if p == 0:
            return N
        return pinned[p - 1][1] if p - 1 in pinned else claim.get(p - 1)

    def elig(p, o):
        if o[4] >= dl[p] or (p in claim and o[1] != claim[p]) or (o[3] != N and o[3] - 1 != p):
            return False
        return o[0] != C or before(p) is None or o[2] == before(p)

    return gaps, ops, elig, before


def first_fit(recs, cut=None):
    gaps, ops, elig, before = layout(recs, cut)
    op_of, gap_of = {}, {}
    for g in gaps:
        for i, o in enumerate(ops):
            if i not in gap_of and elig(g, o):
                op_of[g], gap_of[i] = i, g
                break
    return gaps, ops, elig, before, op_of, gap_of


def shortest_path(gaps, ops, elig, gap_of, g0, end=None):
    """Ops on the shortest augmenting path from the open gap g0 (0: none);
    end, a list, receives the free op the path ends at and the gap it was
    reached from."""
    seen, level, n = set(), [g0], 0
    while level:
        n += 1
        nxt = []
        for g in level:
            for i, o in enumerate(ops):
                if i in seen or not elig(g, o):
                    continue
                seen.add(i)
                if i not in gap_of:
                    if end is not None:
                        end[:] = [o, g]
                    return n
                nxt.append(gap_of[i])
        level = nxt
    return 0


def test_chain_needs_the_whole_path():
    """On every valid chain(L) call-order first-fit leaves exactly the last
    gap open and the shortest augmenting path from it has L + 1 ops; on the
    invalid twins (Hall, and the claim of a value nobody writes) it leaves the
    same gap open and no path exists."""
    n = 0
    for pre in (0, pg.LONG):
        for pl in pg.chain_plants(pre) + (pg.all_limit_plants() if pre == 0 else ()):
            if pl.family != "chain":
                continue
            L = pg._kw(pl)["L"]
            gaps, ops, elig, _, op_of, gap_of = first_fit(pl.recs)
            assert len(gaps) == L + 1 == pg.shape(pl.recs)[0], pl.tag
            assert [g for g in gaps if g not in op_of] == [gaps[-1]], pl.tag
            assert all(op_of[g] == j for j, g in enumerate(gaps[:-1])), pl.tag
            steps = shortest_path(gaps, ops, elig, gap_of, gaps[-1])
            assert steps == (L + 1 if pl.verdict else 0), (pl.tag, steps)
            n += 1
    assert n > 100


def test_coupled_greedy_violates_the_planted_pairs():
    n = 0
    for pre in (0, pg.LONG):
        for pl in pg.coupled_plants(pre) + (pg.all_limit_plants() if pre == 0 else ()):
            if pl.family != "coupled":
                continue
            k = pg._kw(pl)
            ats = [int(x) for x in str(k.get("ats", "")).split("+") if x]
            gaps, ops, elig, before, op_of, _ = first_fit(pl.recs)
            assert len(gaps) == k["G"] == len(op_of), pl.tag
            viol = [g - gaps[0] - 1 for g in gaps
                    if ops[op_of[g]][0] == C and before(g) is None
                    and ops[op_of[g - 1]][1] != ops[op_of[g]][2]]
            assert viol == ats, (pl.tag, viol)
            n += 1
    assert n > 60


def test_pending_ops_are_pending_at_the_failing_return():
    """Every pending plant holds npend (+1 with dup) :ok writes called before
    the failing read's return and returning after it ("last": after its
    call), and the failing return is the key's first / second / last where
    the tag says so."""
    n = 0
    for pl in pg.pending_plants(0) + pg.pending_plants(pg.LONG):
        k = pg._kw(pl)
        f2 = max((r for r in pl.recs if r[0] == R), key=lambda r: r[4])
        assert pl.verdict == 1 or pl.recs[pl.fail_op] is f2, pl.tag
        at = f2[4] if k["where"] == "last" else f2[5]
        pend = [r for r in pl.recs if r[0] != R and r[5] != INF and r[4] < at < r[5]]
        assert len(pend) == k["npend"] + k["dup"], pl.tag
        rets = sorted(r[5] for r in pl.recs if r[5] != INF)
        if k["where"] in ("first", "second"):
            assert rets.index(f2[5]) == WHERE_RANK[k["where"]], pl.tag
        elif k["where"] == "last" and not k["dup"]:
            assert rets[-1] == f2[5], pl.tag
        else:
            assert rets[0] < f2[5] < rets[-1], pl.tag
        n += 1
    assert n > 40


WHERE_RANK = {"first": 0, "second": 1}


def _probed(pl):
    """(F2, cut): the failing read (the twin's: the last read called) and the
    last event at which every X is still open: the one before F2's return
    ("middle": the counterexample search always decides that prefix, as its
    last valid probe and in the witness pass), or before the first X's
    ("last": the X return between F2's call and its return)."""
    f2 = max((r for r in pl.recs if r[0] == R), key=lambda r: r[4])
    xs = [r[5] for r in pl.recs if r[0] != R and r[5] != INF and r[5] > f2[4]]
    return f2, min(xs + [f2[5]]) - 1


def test_pending_via_ends_at_the_pinned_op_through_its_rival():
    """Every via plant, in the last prefix with every X open: first-fit
    gives X_1's gap to the rival (called first) and leaves the gap open that
    claims the rival's value; the shortest augmenting path from it
    has two ops and ends at the pinned, unmatched X_1, reached at X_1's own
    gap — not the search's root.  With L = 64 and npend = 65 that prefix has
    128 optional ops or more (class mode: the pinned lists), else fewer."""
    n_cls = n_scan = 0
    for pre in (0, pg.SHIFT, pg.LONG):
        for pl in pg.pending_plants(pre):
            if " via=1" not in pl.tag:
                continue
            _, cut = _probed(pl)
            gaps, ops, elig, _, op_of, gap_of = first_fit(pl.recs, cut)
            rival = [i for i, o in enumerate(ops) if o[1] == 7000]
            assert len(rival) == 1 and rival[0] in gap_of, pl.tag
            x1 = [i for i, o in enumerate(ops) if o[3] != N and o[3] - 1 == gap_of[rival[0]]]
            assert len(x1) == 1 and x1[0] not in gap_of and ops[x1[0]][4] > ops[rival[0]][4], pl.tag
            # (the chain's last gap is open too: its path ends at X_0, before these gaps)
            still_open = [g for g in gaps if g not in op_of]
            assert len(still_open) == 2 and still_open[0] < gap_of[rival[0]] < still_open[1], pl.tag
            end = []
            assert shortest_path(gaps, ops, elig, gap_of, still_open[1], end) == 2, pl.tag
            assert end[0] is ops[x1[0]] and end[1] == gap_of[rival[0]] != still_open[1], pl.tag
            big = len(ops) >= pg.K_CLS_MIN_OPS
            assert big == (pg._kw(pl)["npend"] == 65), (pl.tag, len(ops))
            n_cls, n_scan = n_cls + big, n_scan + (not big)
    assert n_cls >= 12 and n_scan >= 12


def test_pending_dup_puts_two_on_one_gaps_list():
    """Every dup plant, in the last prefix with every X open: two open :ok
    writes are pinned to one gap, one op to every other pinned gap; one of the
    plants has 128 optional ops or more there (class mode's aPH / aPN lists),
    the others fewer (the scans)."""
    sizes = []
    for pre in (0, pg.SHIFT, pg.LONG):
        for pl in pg.pending_plants(pre):
            if " dup=1" not in pl.tag:
                continue
            gaps, ops, _, _ = layout(pl.recs, _probed(pl)[1])
            per_gap = {}
            for o in ops:
                if o[3] != N and o[3] - 1 in gaps:  # (a position past the prefix's last is no gap)
                    per_gap[o[3] - 1] = per_gap.get(o[3] - 1, 0) + 1
            assert sorted(per_gap.values())[-2:] in ([2], [1, 2]), (pl.tag, per_gap)
            sizes.append(len(ops) >= pg.K_CLS_MIN_OPS)
    assert sizes.count(True) == 3 and sizes.count(False) == 6


def _one_field(a, b):
    """The records of a and b are the same but for one field of one record."""
    only_a = [r for r in a if r not in b]
    only_b = [r for r in b if r not in a]
    return len(a) == len(b) and len(only_a) == len(only_b) == 1 and \
        sum(x != y for x, y in zip(only_a[0], only_b[0])) == 1


def test_twins_differ_in_one_field():
    n = 0
    for name in GROUPS:
        by_tag = {pl.tag: pl for pl in group(name)}
        for tag, bad in by_tag.items():
            if bad.verdict == 1 or " dup=1" in tag:
                continue
            if bad.family == "pending":
                twin = tag.replace("good=0", "good=1")
            else:
                twin = " ".join(f for f in tag.split(" ") if not f.startswith("bad="))
            if name == "longer" and twin not in by_tag:
                continue  # (a handful: its twins are in the other groups)
            assert _one_field(bad.recs, by_tag[twin].recs) and by_tag[twin].verdict == 1, tag
            n += 1
    assert n > 200


def test_every_edge_is_planted():
    """Each edge the issue names is present by tag, short and behind the long
    ladder; dropping one fails here."""
    for pre in (0, pg.SHIFT, pg.LONG):
        tags = {pl.tag for fam in pg.FAMILIES for pl in pg.family_plants(fam, pre)}
        shapes = {pl.tag: pg.shape(pl.recs) for fam in pg.FAMILIES
                  for pl in pg.family_plants(fam, pre)}
        # chain: both sides of the flip's 64 levels, of the 64-op chunk, of class mode's 128 ops
        for L in (1, 2, 3, 62, 63, 64, 65, 126, 127, 128, 129, 191):
            for bad in (None, "late", "noval"):
                assert pg._tag("chain", L=L, ncls=2, pre=pre, pad=1, bad=bad) in tags
        for L in (1, 3, 63, 64, 65, 128, 129):
            for bad in ("early",):
                assert pg._tag("chain", L=L, ncls=2, pre=pre, pad=1, bad=bad) in tags
        # G == n_opt: the deadline's chunk ends the op list
        for L in (63, 64, 127):
            t = pg._tag("chain", L=L, ncls=2, pre=pre, pad=0)
            assert shapes[t] == (L + 1, L + 1)
        # n_opt on either side of kClsMinOps by the pads alone
        assert {shapes[pg._tag("chain", L=3, ncls=2, pre=pre, pad=p)][1] for p in (123, 124, 125)} \
            == {pg.K_CLS_MIN_OPS - 1, pg.K_CLS_MIN_OPS, pg.K_CLS_MIN_OPS + 1}
        # 63, 64 classes (class mode) and 65 (scan mode with n_opt >= 128)
        for ncls in (63, 64, 65):
            for L, pad in ((ncls - 1, 130), (130, 0), (191, 3)):
                t = pg._tag("chain", L=L, ncls=ncls, pre=pre, pad=pad)
                pl = [p for p in pg.chain_plants(pre) if p.tag == t][0]
                classes = {(r[1], r[2]) for r in pl.recs if r[0] != R and r[5] == INF}
                assert len(classes) == ncls and shapes[t][1] >= pg.K_CLS_MIN_OPS
        # coupled: pairs on either side of the 64-gap scan step and at the clamp G - 1
        for G in pg.COUPLED_G:
            for at in {0, 62, 63, G - 2} | ({64} if G > 65 else set()):
                for bad in (None, "val@%d" % at, "late@%d" % at):
                    assert pg._tag("coupled", G=G, ats=str(at), pre=pre, pad=1, bad=bad) in tags
            ev = pg._evens(G)  # a run of pairs at consecutive even gaps, to the last pair
            assert len(ev) == 12 and all(b - a == 2 for a, b in zip(ev, ev[1:]))
            assert ev[-1] in (G - 2, G - 3) or ev[0] < 64 < ev[-1]
            assert pg._tag("coupled", G=G, ats="+".join(map(str, ev)), pre=pre, pad=1) in tags
            assert any(t.startswith("coupled G=%d " % G) and t.endswith("second=3") for t in tags)
            assert len(pg.COUPLED_MANY[G]) >= 4
        assert any(t.startswith("coupled") and shapes[t][1] >= pg.K_CLS_MIN_OPS for t in tags)
        # pending: 1, 2 and 65 pinned optional ops; every place of the failing return
        for n in pg.PENDING_N:
            for where in pg.WHERE if pre == 0 else ("middle", "last"):
                for L in ((2, 64) if where in ("middle", "last") else (0,)):
                    assert pg._tag("pending", L=L, where=where, npend=n, pre=pre, pad=1,
                                   dup=0, good=0) in tags
        assert sum(" dup=1" in t for t in tags) == 3
        assert pg._tag("pending", L=64, where="middle", npend=65, pre=pre, pad=1, dup=1, good=0) in tags
        for L, n, where in ((2, 2, "middle"), (3, 3, "last"), (64, 65, "middle"), (64, 65, "last")):
            for good in (0, 1):
                assert pg._tag("pending", L=L, where=where, npend=n, pre=pre, pad=1, dup=0,
                               good=good, via=1) in tags
    # limits: each side of kFgMaxGaps, kFgMaxOps, kFgStash (first and fourth
    # wave), of the matching's LDS reserve, and class mode below 254 records
    lim = {name: [pg.shape(pl.recs) for pl in pls] for name, pls in pg.limit_plants().items()}
    assert {g for g, _ in lim["in gaps"]} == {47, 48} and {g for g, _ in lim["past gaps"]} == {49}
    assert all(n == g + 1 for g, n in lim["in gaps"] + lim["past gaps"])
    assert {n for _, n in lim["in ops"]} == {95, 96} and {n for _, n in lim["past ops"]} == {97}
    # ... and only that limit: within fast_gap's other two
    for name in ("in gaps", "past gaps", "in ops", "past ops"):
        for pl in pg.limit_plants()[name]:
            runs = [sum(r[0] != R and r[5] == INF for r in pl.recs[i:i + 64])
                    for i in range(0, len(pl.recs), 64)]
            assert max(runs) <= pg.K_FG_STASH and len(pl.recs) <= 256, (pl.tag, runs)
    assert all(n <= pg.K_FG_MAX_OPS for _, n in lim["in gaps"] + lim["past gaps"])
    assert all(g <= pg.K_FG_MAX_GAPS for g, _ in lim["in ops"] + lim["past ops"])
    for name in ("in stash", "past stash", "in stash wave3", "past stash wave3"):
        assert all(g <= pg.K_FG_MAX_GAPS and n <= pg.K_FG_MAX_OPS for g, n in lim[name])
    for w, first in (("", 0), (" wave3", 192)):
        for side, want in (("in", 32), ("past", 33)):
            for pl in pg.limit_plants()["%s stash%s" % (side, w)]:
                run = pl.recs[first:first + 64]
                assert len(pl.recs) == first + 64
                assert sum(r[5] == INF for r in run) == want == pg.K_FG_STASH + (side == "past")
    fit = pg.RESERVE_FIT
    assert pg.match_lds_bytes(fit, fit) <= pg.K_MATCH_RESERVE < pg.match_lds_bytes(fit + 1, fit + 1)
    assert fit == 89 and set(lim["reserve"]) == {(fit, fit), (fit + 1, fit + 1)}
    mg = pg.limit_plants()["mgr"]
    fits = {pg.mgr_fits(*pg.shape(pl.recs), len(pl.recs), pg.MGR_LONGEST) for pl in mg[:2]}, \
        {pg.mgr_fits(*pg.shape(pl.recs), len(pl.recs), pg.MGR_LONGEST) for pl in mg[2:]}
    assert fits == ({True}, {False}) and all(pg.shape(pl.recs)[1] >= pg.K_CLS_MIN_OPS for pl in mg)
    assert all(pg.match_lds_bytes(*pg.shape(pl.recs)) <= pg.lds_room(len(pl.recs), pg.MGR_LONGEST)
               and len(pl.recs) < pg.MGR_LONGEST <= 1050 for pl in mg)
    assert all(len(pl.recs) < 254 and pg.shape(pl.recs)[1] >= pg.K_CLS_MIN_OPS
               for pl in pg.limit_plants()["small cls"])
    # the long variants are past the version-order tier, the longer ones past 2,048
    assert all(len(pl.recs) > 1024 for pl in group("chain-long"))
    assert all(len(pl.recs) >= 2048 for pl in pg.longer_plants())
    assert {pg._kw(pl)["where"] for pl in pg.longer_plants() if pl.family == "pending"
            and pl.verdict == 0} == set(pg.WHERE)


# ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", GROUPS)
def test_oracle_agrees_with_every_plant(name):
    pls = group(name)
    ops, off = pack_keys([pl.recs for pl in pls])
    want_v = np.array([pl.verdict for pl in pls])
    want_f = np.array([pl.fail_op for pl in pls])
    assert ((want_v == 0) == (want_f >= 0)).all() and (want_v == 0).any() and (want_v == 1).any()
    _, j = oracle.check(ops, off, algo=oracle.JITC, n_threads=8, max_configs=1 << 20)
    _, w = oracle.check(ops, off, algo=oracle.WGL, n_threads=8, max_configs=1 << 20)
    bad = np.nonzero((j["verdict"] != want_v) | (w["verdict"] != want_v) |
                     (j["fail_op"] != want_f))[0]
    assert len(bad) == 0, [(pls[k].tag, int(j["verdict"][k]), int(w["verdict"][k]),
                            int(j["fail_op"][k])) for k in bad[:5]]
    inv = np.nonzero(want_v == 0)[0]
    assert all(j["fail_prefix_end"][k] == pls[k].recs[pls[k].fail_op][5] for k in inv)


@pytest.mark.parametrize("name", GROUPS)
def test_restatement_agrees_and_its_witnesses_certify(name):
    """gapmatch_ref decides every plant as constructed and bisects to the
    same fail op; every valid plant's witness passes oracle.check_witness.
    Behind the long ladders every tenth plant (the bisection in Python is
    slow there); the oracle runs on all of them above."""
    pls = group(name)
    if name.endswith("long"):
        pls = pls[::10]
    wits, valid = [], []
    for pl in pls:
        if pl.verdict == 1:
            v, w = gm.decide(pl.recs, witness=True)
            assert v == 1, pl.tag
            wits.append(w)
            valid.append(pl)
        else:
            assert gm.decide(pl.recs) == 0, pl.tag
            assert gm.first_failure(pl.recs) == (pl.fail_op, pl.recs[pl.fail_op][5]), pl.tag
    ops, off = pack_keys([pl.recs for pl in valid])
    wit = np.array([x for w in wits for x in w], dtype=np.int32)
    kind = np.full(len(valid), abi.LC_WITNESS_FULL, dtype=np.int32)
    st, _ = oracle.check_witness(ops, off, wit, kind)
    assert (st == oracle.WIT_OK).all(), [valid[k].tag for k in np.nonzero(st != oracle.WIT_OK)[0]]
