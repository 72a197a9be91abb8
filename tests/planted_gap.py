"""Deterministic keys for the gap matching (csrc/gapmatch.h, driven by
gap_tier.hip and, for crash-light keys, by fast_gap in check_kernel.hip),
planted where the matching changes hands: at the 64-op chunks of the scans,
at the 64 levels the augmenting path's flip takes per pass, at the class
mode's 128 optional ops and 64 classes, at the 64-gap steps of the violation
scan, at fast_gap's limits and at the LDS placement's.  No randomness.

Records are [f, value, expected, version, call, ret] as in planted.py, and
every builder returns planted.Plant(family, tag, recs, verdict, fail_op) with
the verdict and the canonical fail op known from the construction.  Every
invalid plant has a valid twin that differs in one field (of one record; the
records stay sorted by call, so the record may sit elsewhere).

Two parameters are common to all builders:
  pre  a clean ladder of `pre` :ok writes in front (position p: version p + 1,
       value p % 7, call 4p, ret 4p + 1).  It shifts the gap positions, and
       pre >= LONG lifts the key past the version-order tier's 1,024 records,
       so the gap tier proper decides it whatever fast_gap's limits say.
  pad  crashed writes called after the key's last return: never eligible for
       any gap, but counted in n_opt, which keeps n_opt >= G (the G > n_opt
       shortcut then never decides for the matching) and, from 128 on, turns
       the class-indexed mode on.

The gaps start at position P0 = pre and time T = 4 * pre; step i of a family
owns the eight event slots from T + 8i.

tests/test_planted_gap.py pins every plant against both oracle searches and
gapmatch_ref, and proves the construction (what call-order first-fit leaves
open, the augmenting path's length) with a first-fit of its own."""
import functools

from helpers import INF, C, N, R, W
from planted import Plant, interleave  # noqa: F401  (interleave: for the GPU batches)

SHIFT = 5            # a small ladder: the same gaps at other positions and record indices
LONG = 1030          # past kFastMaxRecords = 1,024
LONGER = 2050        # past 2,048: 512-thread workgroups, multisection rounds
NOBODY = 51          # a value no op writes
V0 = 50              # chain: the value only o_0 writes
PADV = 100           # the pads' value: chain's o_1 has it too (no class of its own)

# gapmatch.h / check_kernel.hip / gap_tier.hip constants the edges come from
K_WAVE, K_MAX_CLS, K_CLS_MIN_OPS = 64, 64, 128
K_FG_MAX_GAPS, K_FG_MAX_OPS, K_FG_STASH = 48, 96, 32
K_MATCH_RESERVE = 8 << 10


def match_lds_bytes(g, n_opt):
    return 36 * g + 44 * n_opt + 16 * K_MAX_CLS + 16


# the largest G = n_opt whose matching fits the LDS kept after a skeleton
RESERVE_FIT = max(g for g in range(1, 200) if match_lds_bytes(g, g) <= K_MATCH_RESERVE)


def lds_room(n_key, n_longest):
    """LDS left for a key's matching after its skeleton (68 B per record of
    its own capacity), in a batch whose LDS is sized by the longest key's
    skeleton plus the reserve (gap_tier.hip gap_ws / lincheck.cpp gap_plan)."""
    cap = lambda n: (n + 2 + 3) & ~3  # noqa: E731
    return 68 * (cap(n_longest) - cap(n_key)) + K_MATCH_RESERVE


def mgr_fits(g, n_opt, n_key, n_longest):
    """mgr_room: the class mode's per-op copies of matched gap records (16 B
    per op) fit behind the matching."""
    return match_lds_bytes(g, n_opt) + 16 * n_opt <= lds_room(n_key, n_longest)


def _mgr_edge():
    """(pad, longest): chain(3, pad=pad) has room for the copies beside a key
    of `longest` records and chain(3, pad=pad + 1) has not; both in class mode."""
    for longest in range(200, 400):
        for pad in range(K_CLS_MIN_OPS - 4, 200):
            if mgr_fits(4, 4 + pad, 8 + pad, longest) and not mgr_fits(4, 5 + pad, 9 + pad, longest) \
                    and match_lds_bytes(4, 5 + pad) <= lds_room(9 + pad, longest):
                return pad, longest
    raise AssertionError("no mgr_room edge")


MGR_PAD, MGR_LONGEST = _mgr_edge()


def _ladder(pre):
    return [[W, p % 7, N, p + 1, 4 * p, 4 * p + 1] for p in range(pre)]


def _finish(family, tag, recs, fail, pad, verdict, t=None, thin=False):
    """Append the pads (from time t: the same for a plant and its twins), sort
    by call and find the fail op's index.  thin: a crashed read [nil nil]
    after every pad (it constrains nothing), so that no aligned run of 64
    records holds more than 32 crashed writes."""
    last = max(max(r[4] for r in recs), max([r[5] for r in recs if r[5] != INF] or [0]))
    t = last + 1 if t is None else t
    assert t > last
    if thin:
        recs = recs + [[W if i % 2 == 0 else R, PADV if i % 2 == 0 else N, N, N, t + i, INF]
                       for i in range(2 * pad)]
    else:
        recs = recs + [[W, PADV, N, N, t + i, INF] for i in range(pad)]
    recs.sort(key=lambda r: r[4])
    calls = [r[4] for r in recs]
    assert len(set(calls)) == len(calls), tag
    fail_op = -1 if fail is None else [i for i, r in enumerate(recs) if r is fail][0]
    assert (verdict == 0) == (fail_op >= 0)
    return Plant(family, tag, recs, verdict, fail_op)


def _tag(family, **kw):
    return family + " " + " ".join("%s=%s" % i for i in sorted(kw.items()) if i[1] is not None)


def shape(recs):
    """(G, n_opt) of the whole key: unpinned positions below the last one a
    required op needs, and crashed mutations."""
    pinned = {r[3] - 1 for r in recs if r[0] != R and r[5] != INF}
    m = max([r[3] for r in recs if r[5] != INF and r[3] != N] or [0])
    return (sum(1 for p in range(m) if p not in pinned),
            sum(1 for r in recs if r[0] != R and r[5] == INF))


# ---------------------------------------------------------------------------
def _chain_recs(L, ncls, pre, last_call=None, last=None):
    """The chain's records without the final read: crashed writes o_0 .. o_L
    called in that order, and version-only reads r_0 .. r_{L-1}, r_j of
    version P0 + j + 1 returning between the calls of o_{j+1} and o_{j+2}.
    last_call moves o_L's call; `last` replaces o_L altogether."""
    assert L >= 1 and 2 <= ncls <= L + 1
    T, P0 = 4 * pre, pre
    recs = _ladder(pre)
    for i in range(L + 1):
        call = T + i if i < 2 else T + 8 * (i - 1)
        v = V0 if i == 0 else PADV + (i - 1) % (ncls - 1)
        if i == L and last is not None:
            recs.append(last)
        else:
            recs.append([W, v, N, N, last_call if i == L and last_call is not None else call, INF])
    for j in range(L):
        recs.append([R, N, N, P0 + j + 1, T + 8 * j + 4, T + 8 * j + 6])
    return recs


def chain(L, ncls=2, pre=0, pad=0, bad=None, thin=False):
    """An augmenting path of exactly L + 1 ops.  Gaps g_0 .. g_L at positions
    P0 .. P0 + L; gap j < L is value-free and its deadline (r_j's return)
    admits o_0 .. o_{j+1}; g_L is claimed by a read F of V0, which only o_0
    writes.  Call-order first-fit gives g_j <- o_j and g_L then needs the
    whole chain flipped (g_L <- o_0, g_j <- o_{j+1}).  o_1 .. o_L are spread
    over ncls - 1 values, so the key has ncls classes.

    bad = "late"   o_L called one event after g_{L-1}'s deadline D: o_0 ..
                   o_{L-1} must fill L + 1 gaps (Hall); fails at F.
          "early"  o_L called at D - 1, after r_{L-1} was called: valid.  (D - 1
                   and D + 1 are the calls next to the deadline: a key's
                   event indices are distinct, so none equals it.)
          "noval"  F claims a value nobody writes; fails at F."""
    T, P0 = 4 * pre, pre
    D = T + 8 * (L - 1) + 6
    lc = {"late": D + 1, "early": D - 1}.get(bad)
    recs = _chain_recs(L, ncls, pre, last_call=lc)
    F = [R, NOBODY if bad == "noval" else V0, N, P0 + L + 1, T + 8 * L + 4, T + 8 * L + 6]
    recs.append(F)
    ok = bad in (None, "early")
    return _finish("chain", _tag("chain", L=L, ncls=ncls, pre=pre, pad=pad, bad=bad,
                                 thin=1 if thin else None), recs,
                   None if ok else F, pad, int(ok), T + 8 * L + 8, thin)


# ---------------------------------------------------------------------------
def _u(i):
    return 200 + i          # the value gap i's read claims


A_VAL = 10000


def _a(i):
    """The value of pair i's first-called write.  The same for every
    pair: the a's are left over, and left-over crashed writes of one value
    are one counted class to the oracle's JITC search, which crashed writes
    of k values would cost 2^k configurations."""
    return A_VAL


def _b(i):
    return 10001 + i        # pair i's second-called write, which its CAS expects


def coupled(G, ats, pre=0, pad=0, bad=None, second=None):
    """G consecutive gaps; gap i is filled by its own crashed write of _u(i)
    and claimed by a read.  At every i in ats gap i is free (no read of its
    version) and gap i + 1 takes a crashed CAS [b -> _u(i + 1)]; two writes
    are eligible for the free gap, a called first, then b.  First-fit places
    a, the CAS expects b: a violation the expected-value-first branch repairs.

    bad = ("val", i)   the b of pair i writes a value the CAS does not expect:
                       every value of the free gap is tried and fails.
          ("late", i)  that b is called one event past the free gap's deadline
                       (the return of gap i + 1's read).
    Both fail at the read that claims the CAS's value.

    second = i (in ats, gap i - 1 an ordinary one): the pair's first-called
    CAS expects _u(i - 1), whose only writer is gap i - 1's own and cannot be
    spared; a second CAS expects b's value.  The value the branch tries
    first fails in the matching, the search backtracks and a later-tried
    value (b's) holds."""
    ats = tuple(sorted(ats))
    T, P0 = 4 * pre, pre
    cas_at = {i + 1 for i in ats}
    assert all(0 <= i and i + 1 < G and i not in cas_at for i in ats)
    if second is not None:
        assert second in ats and second >= 1 and second - 1 not in ats and second - 1 not in cas_at
    recs = _ladder(pre)
    fail = None
    for i in range(G):
        S = T + 8 * i
        read = [R, _u(i), N, P0 + i + 1, S + 4, S + 6]
        if i in ats:
            recs.append([W, _a(i), N, N, S, INF])
            b = [W, _b(i), N, N, S + 1, INF]
            if bad == ("val", i):
                b[1] = NOBODY
            elif bad == ("late", i):
                b[4] = S + 8 + 7
            recs.append(b)
            continue
        if i in cas_at:
            if second == i - 1:
                recs.append([C, _u(i), _u(i - 2), N, S, INF])
                recs.append([C, _u(i), _b(i - 1), N, S + 1, INF])
            else:
                recs.append([C, _u(i), _b(i - 1), N, S, INF])
            if bad is not None and bad[1] == i - 1:
                fail = read
        else:
            recs.append([W, _u(i), N, N, S, INF])
        recs.append(read)
    assert (bad is None) == (fail is None)
    return _finish("coupled", _tag("coupled", G=G, ats="+".join(map(str, ats)), pre=pre, pad=pad,
                                   bad=bad and "%s@%d" % bad, second=second),
                   recs, fail, pad, int(bad is None), T + 8 * G + 8)


# ---------------------------------------------------------------------------
WHERE = ("first", "second", "middle", "last")
# pending: how many of the X_i have a crashed write that could take their
# position instead (each doubles the frontier of the oracle's searches)
RIVALS = 1


def pending(L, where, npend=1, pre=0, pad=0, dup=False, good=False, via=False):
    """An invalid key in which gap positions near the failing return are held
    by :ok writes called before that return and returning after it: pinned in
    the whole key, optional ops pinned to their position in every prefix the
    counterexample search probes.

    "middle" / "last": the valid chain(L) with o_L replaced by the :ok write
    X_0 of version P0 + L (g_{L-1}'s position): in a prefix X_0 is the free
    end of the augmenting path from g_L.  Then npend - 1 positions held by
    :ok writes X_1 .., the first RIVALS of them each called before a crashed
    write that could take the position too (first-fit matches X_i, and it has
    to stay), then one gap claimed by a
    read F2 of a value nobody writes (good=True: of the value the crashed
    write z has).  The X return after F2 ("middle") or between F2's call and
    its return ("last": F2's is the key's last return).
    dup: a second :ok write claims X_0's version as well, called later and
    returning last: two pinned ops in one gap's list while both are pending
    (with L = 64 and npend = 65 the prefixes before F2's return hold 128
    optional ops or more: the list is the class mode's aPH / aPN).
    via: X_1's rival (value 7000) is called before X_1, so first-fit gives
    X_1's gap to the rival; a further gap after the X_i is claimed by a read
    Fv of 7000, which only the rival writes.  In every prefix from Fv's
    return on that gap needs an augmenting path of two ops: the rival, then
    through X_1's gap to the pinned X_1, the path's free end at a gap the
    search reached (not its root, as X_0 is).
    A matched pinned op is never on a path: it is eligible for its own gap
    only, so that gap is matched to it, and a search reaches a matched gap
    only through the op it is matched to; the search would have had to visit
    the pinned op from its own gap first.  No plant can make an augmenting
    search visit one, in either mode.

    "first" / "second": no chain (L = 0): positions 0 .. npend - 1 held by the
    X_i, the gap after them claimed by F2, whose return is the key's first
    (lo == 0: no witness pass), or its second after a read of version 0."""
    assert where in WHERE and npend >= 1
    T, P0 = 4 * pre, pre
    chained = where in ("middle", "last")
    assert chained == (L >= 1) and (chained or pre == 0)
    if chained:
        # X_0 where o_L was called; its return is set below
        x0 = [W, PADV, N, P0 + L, T + 1 if L == 1 else T + 8 * (L - 1), None]
        recs = _chain_recs(L, 2, pre, last=x0)
        recs.append([R, V0, N, P0 + L + 1, T + 8 * L + 4, T + 8 * L + 6])
        xs, S, q = [x0], T + 8 * (L + 1), P0 + L + 1
        n_more = npend - 1
    else:
        recs, xs, S, q, n_more = [], [], 8, 0, npend
        if where == "second":
            recs.append([R, N, N, 0, 0, 1])
    assert not via or (chained and n_more >= 1 and RIVALS >= 1)
    for i in range(n_more):
        first = int(via and i == 0)  # the rival called first
        x = [W, 300 + i, N, q + i + 1, S + 2 * i + first, None]
        recs.append(x)
        if i < RIVALS:
            recs.append([W, 7000, N, N, S + 2 * i + 1 - first, INF])
        xs.append(x)
    S, q = S + 2 * n_more, q + n_more
    if via:
        recs.append([R, 7000, N, q + 1, S, S + 2])
        S, q = S + 4, q + 1
    z = [W, 60, N, N, S, INF]
    F2 = [R, 60 if good else NOBODY, N, q + 1, S + 2, S + 4 + (npend + 1 if where == "last" else 0)]
    recs += [z, F2]
    for i, x in enumerate(xs):
        x[5] = S + 4 + i if where == "last" else S + 6 + i
    if dup:
        assert chained
        recs.append([W, PADV + 1, N, xs[0][3], S + 1, F2[5] + npend + 8])
    return _finish("pending", _tag("pending", L=L, where=where, npend=npend, pre=pre, pad=pad,
                                   dup=int(dup), good=int(good), via=1 if via else None),
                   recs, None if good and not dup else F2, pad, int(good and not dup))


# ---------------------------------------------------------------------------
# the edges (tests/test_planted_gap.py, test_every_edge_is_planted, names them)
CHAIN_L_SCAN = (1, 2, 3, 62, 63, 64, 65, 126)   # n_opt = L + 1 < 128
CHAIN_L_CLS = (127, 128, 129, 191)              # n_opt >= 128 without pads
CHAIN_NCLS = (2, 63, 64, 65)                    # 65: scan mode whatever n_opt
CHAIN_BAD = ("late", "early", "noval")
COUPLED_G = (65, 66, 129)
# several pairs in one key (multi-push), on both sides of gap 64 where G allows
COUPLED_MANY = {65: (0, 30, 61, 63), 66: (0, 30, 62, 64), 129: (0, 62, 64, 100, 127)}


def coupled_ats(G):
    """Single pairs on either side of the violation scan's 64-gap step and at
    its clamp: the pair (i, i + 1) needs i + 1 < G."""
    return sorted(i for i in {0, 62, 63, 64, G - 2} if i + 1 < G)


PENDING_N = (1, 2, 65)


def _with_twins(make, bads):
    return [make(None)] + [make(b) for b in bads]


@functools.lru_cache(maxsize=None)
def chain_plants(pre=0):
    out = []
    for L in CHAIN_L_SCAN + CHAIN_L_CLS:
        bads = CHAIN_BAD if L in (1, 3, 63, 64, 65, 128, 129) else ("late", "noval")
        out += _with_twins(lambda b: chain(L, 2, pre, 1, b), bads)
        if L in (63, 64, 127):  # no pad: G == n_opt, the deadline chunk's last op is the last op
            out += _with_twins(lambda b: chain(L, 2, pre, 0, b), ("late",))
    # class mode from the pads: n_opt = 128 exactly, 129, and one short of it
    for L, pad in ((3, 123), (3, 124), (3, 125), (62, 65), (63, 64), (64, 64), (65, 62)):
        out += _with_twins(lambda b: chain(L, 2, pre, pad, b), ("late", "noval"))
    # o_1 .. o_L over ncls - 1 values: 63 and 64 classes in class mode, 65 in scan
    for ncls in CHAIN_NCLS[1:]:
        for L, pad in ((ncls - 1, 130), (130, 0), (191, 3)):
            out += _with_twins(lambda b: chain(L, ncls, pre, pad, b), ("late",))
    return tuple(out)


def _evens(G):
    """A run of 12 pairs at consecutive even gaps (a run of branch levels),
    across gap 64 where G allows, else the last 12.  (12, not every even gap:
    each left-over write doubles the configurations of the oracle's WGL
    search, which decides 16 pairs within its budget and not 32.)"""
    hi = min(76, (G - 2) // 2 * 2 + 2)
    return tuple(range(hi - 24, hi, 2))


@functools.lru_cache(maxsize=None)
def coupled_plants(pre=0):
    out = []
    for G in COUPLED_G:
        for at in coupled_ats(G):
            out += _with_twins(lambda b: coupled(G, (at,), pre, 1, b), (("val", at), ("late", at)))
        many = COUPLED_MANY[G]
        out += _with_twins(lambda b: coupled(G, many, pre, 1, b), (("val", many[2]), ("late", many[-1])))
        ev = _evens(G)
        out += _with_twins(lambda b: coupled(G, ev, pre, 1, b), (("val", ev[-1]), ("late", ev[len(ev) // 2])))
        # backtracking: the early pair at 3 holds only with a later-tried value
        late = COUPLED_MANY[G][2:4]
        out.append(coupled(G, (3,) + late, pre, 1, second=3))
        out.append(coupled(G, (3,) + late, pre, 1, bad=("val", late[1]), second=3))
    # few classes and n_opt >= 128 from the pads: branches in class mode
    out += _with_twins(lambda b: coupled(20, (0, 9, 18), pre, 120, b), (("val", 9), ("late", 18)))
    out += _with_twins(lambda b: coupled(3, (0,), pre, 0, b), (("val", 0), ("late", 0)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def pending_plants(pre=0):
    out = []
    for n in PENDING_N:
        for where in WHERE:
            if where in ("first", "second") and pre:
                continue  # the key's first returns are the ladder's
            for L in ((2, 64) if where in ("middle", "last") else (0,)):
                out += [pending(L, where, n, pre, 1), pending(L, where, n, pre, 1, good=True)]
    out += [pending(3, "middle", 2, pre, 1, dup=True), pending(64, "last", 1, pre, 1, dup=True),
            pending(64, "middle", 65, pre, 1, dup=True),  # two on one gap's list in class mode
            pending(3, "middle", 2, pre, 130), pending(3, "middle", 2, pre, 130, good=True)]
    # the pinned op the free end of a path through its rival: scan and class mode
    for L, n, where in ((2, 2, "middle"), (3, 3, "last"), (64, 65, "middle"), (64, 65, "last")):
        out += [pending(L, where, n, pre, 1, via=True), pending(L, where, n, pre, 1, good=True, via=True)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def limit_plants():
    """{name: plants}: the smallest shapes on either side of each crash-light
    and placement limit.  "in ..." groups stay within fast_gap's limits (short
    keys: fast_gap decides them where the version order ran); each "past ..."
    group is just past one limit and is handed to the gap tier proper."""
    g = {}
    both = lambda make: _with_twins(make, ("late",))  # noqa: E731
    # (pre = 1 and thin pads: at most 32 crashed writes in every aligned run
    # of 64 records, so that only the limit meant is passed)
    g["in gaps"] = [pl for G in (47, 48) for pl in both(lambda b: chain(G - 1, 2, 1, 1, b))]
    g["past gaps"] = both(lambda b: chain(48, 2, 1, 1, b))
    g["in ops"] = [pl for n in (95, 96) for pl in both(lambda b: chain(3, 2, 0, n - 4, b, True))]
    g["past ops"] = both(lambda b: chain(3, 2, 0, 97 - 4, b, True))
    # 32 / 33 crashed ops in one aligned run of 64 records: 32 steps of
    # (write, read); one free pair (two writes, no read) makes it 33.  pre =
    # 192: the run is records 192 .. 255, the fourth wave's
    for pre in (0, 192):
        w = "" if pre == 0 else " wave3"
        g["in stash" + w] = _with_twins(lambda b: coupled(32, (), pre, 0, b), ())
        g["past stash" + w] = _with_twins(lambda b: coupled(32, (5,), pre, 0, b), (("val", 5),))
    # G = n_opt on either side of match_lds_bytes(G, n_opt) = kMatchReserve
    g["reserve"] = [pl for G in (RESERVE_FIT, RESERVE_FIT + 1)
                    for pl in both(lambda b: chain(G - 1, 2, 0, 0, b))]
    # n_opt >= 128 on either side of mgr_room, beside a key of MGR_LONGEST
    # records.  (Not as its batch's longest key, as the reserve's plants are:
    # there the room is kMatchReserve = 8,192 B, and class mode's matching with
    # the copies needs 60 * 128 + 36 G + 1,040 > 8,192 at the least, so mgr_room
    # is false for every such key and has no edge.)
    g["mgr"] = [pl for pad in (MGR_PAD, MGR_PAD + 1) for pl in both(lambda b: chain(3, 2, 0, pad, b))]
    # class mode below 254 records (cap < 4 * kMaxCls: scan mode without LDS)
    g["small cls"] = both(lambda b: chain(3, 2, 0, 130, b)) + both(lambda b: chain(100, 5, 0, 30, b))
    return g


def lengthen(pl, pre):
    """The same plant behind a ladder of `pre` more writes (by its tag; a
    ladder of LONG or more is replaced, not added to)."""
    return _REBUILD[pl.family](pl, pre)


def _kw(pl):
    kw = dict(f.split("=", 1) for f in pl.tag.split(" ")[1:])
    return {k: int(v) if v.lstrip("-").isdigit() else v for k, v in kw.items()}


def _re_chain(pl, pre):
    k = _kw(pl)
    return chain(k["L"], k["ncls"], pre + (k["pre"] if k["pre"] < 256 else 0), k["pad"], k.get("bad"),
                 bool(k.get("thin")))


def _re_coupled(pl, pre):
    k = _kw(pl)
    ats = tuple(int(x) for x in str(k["ats"]).split("+")) if "ats" in k and str(k["ats"]) else ()
    bad = k.get("bad")
    if bad:
        kind, at = bad.split("@")
        bad = (kind, int(at))
    return coupled(k["G"], ats, pre + (k["pre"] if k["pre"] < 256 else 0), k["pad"], bad,
                   k.get("second"))


def _re_pending(pl, pre):
    k = _kw(pl)
    return pending(k["L"], k["where"], k["npend"], pre, k["pad"], bool(k["dup"]), bool(k["good"]),
                   bool(k.get("via")))


_REBUILD = {"chain": _re_chain, "coupled": _re_coupled, "pending": _re_pending}

FAMILIES = ("chain", "coupled", "pending")


@functools.lru_cache(maxsize=None)
def family_plants(family, pre=0):
    return {"chain": chain_plants, "coupled": coupled_plants, "pending": pending_plants}[family](pre)


@functools.lru_cache(maxsize=None)
def all_limit_plants():
    return tuple(pl for pls in limit_plants().values() for pl in pls)


@functools.lru_cache(maxsize=None)
def longer_plants():
    """A handful behind a ladder of LONGER writes: 512-thread workgroups and
    multisection rounds, with pending's invalid plants among them."""
    return (chain(64, 2, LONGER, 1), chain(64, 2, LONGER, 1, "late"), chain(129, 2, LONGER, 1, "late"),
            coupled(65, (0, 61, 63), LONGER, 1), coupled(65, (0, 61, 63), LONGER, 1, ("val", 61)),
            pending(2, "middle", 2, LONGER, 1), pending(64, "last", 65, LONGER, 1),
            pending(3, "middle", 2, LONGER, 1, good=True),
            # the failing return the key's first and second: padded, not laddered
            pending(0, "first", 2, 0, LONGER), pending(0, "second", 1, 0, LONGER))
