"""Deterministic keys for the certificate finder (cert.hip, cert_kernel): one
infeasibility each, built to be found by one stage at one edge of that
stage's ownership pattern — the r = tid + 256 k record strides, the suffix
minimum in which thread t owns ceil((M + 1) / 256) consecutive positions,
the contiguous record runs of ceil(n / 256) prefix-summed into the list of
version-less candidates, the i = lane + 64 k open positions of the PROOF
search.  No randomness.

Records are [f, value, expected, version, call, ret] as in helpers.py.  Every
plant is a version-pinned key: every :ok mutation carries a version and no
read is [nil x], so the version-order and gap tiers decide it and name the
failing return.  Events take even times in call order (the odd ones are spare
for a twin that moves one event).  The base is a ladder: the write at
position p has value val(p) and version v0 + p + 1, called and returned in
turn.  Pads of [nil nil] reads after the failing return change n without
changing the prefix.

Every builder returns a Plant: the records, the expected verdict, the fail
op, and for an invalid plant the certificate it is built to get — (kind, a,
b, c) and the set — derived by hand from the builder, not read back from any
finder.  Each invalid plant has a valid twin (good=True) that differs in one
field.  tests/test_planted_cert.py pins all of it on the CPU."""
import functools
from collections import namedtuple

from helpers import INF, C, N, R, W

Plant = namedtuple("Plant", "family tag recs verdict fail_op cert cset t0 v0 init")

NONE, DUP, UNREACH, CLAIMS, PAIR, ORDER, HALL, PROOF = range(8)
BRANCH = 2
NO_CERT = (NONE, -1, -1, 0)

# (first call, init_version, init_value) of the `base` family
BASES = ((1 << 40, 0, N), (1 << 62, 0, N), (0, 7, 3))


def val(p):
    return p % 7


def tok(kind, a, b=0):
    x = (kind << 30) | (a << 15) | b
    return x - (1 << 32) if x >= (1 << 31) else x


class _Key:
    """Records appended in call order; every event takes the next even time."""

    def __init__(self, t0=0, v0=0, init=N):
        self.recs, self.t, self.t0, self.v0, self.init = [], t0, t0, v0, init

    def tick(self):
        self.t += 2
        return self.t - 2

    def call(self, f, value, expected, version):
        """Called and left open (crashed unless ret() closes it)."""
        self.recs.append([f, value, expected, version, self.tick(), INF])
        return len(self.recs) - 1

    def ret(self, i):
        self.recs[i][5] = self.tick()

    def ok(self, f, value, expected, version):
        i = self.call(f, value, expected, version)
        self.ret(i)
        return i

    def ver(self, p):
        """The version the mutation at position p leaves."""
        return self.v0 + p + 1

    def ladder(self, p0, p1):
        for p in range(p0, p1):
            self.ok(W, val(p), N, self.ver(p))

    def before(self, p):
        """The value before position p of the ladder."""
        return val(p - 1) if p else self.init

    def nil_reads(self, upto):
        """[nil nil] reads until the next record has index `upto`."""
        assert len(self.recs) <= upto, (len(self.recs), upto)
        while len(self.recs) < upto:
            self.ok(R, N, N, N)

    def plant(self, family, tag, good, fail_op, cert, cset=(), pad=0):
        self.nil_reads(max(pad, len(self.recs)))
        if good:
            fail_op, cert, cset = -1, NO_CERT, ()
        tag = "%s %s good=%d t0=%d v0=%d" % (family, tag, int(good), self.t0, self.v0)
        return Plant(family, tag, self.recs, int(good), fail_op, tuple(cert), tuple(cset),
                     self.t0, self.v0, self.init)


def _wrong(v):
    return 5 if v == N else (v + 1) % 7


# ---- ORDER between two mutations -------------------------------------------
ORDER_L = (256, 257, 512, 513, 1024)


def order_mut(L, p, d, good=False, base=(0, 0, N)):
    """M = L - 1 positions.  The ladder below p; a crashed version-less
    filler (it can hold p) and writes pinned at p+1 .. p+d-1 that never
    return (so b's return is legal; crashed version-less ones would do as
    well, but no search decides a key with hundreds of those); b, pinned at
    p+d, called and returned; the ladder above p+d; then a, pinned at p,
    called after all of them: its lower bound at index p lies above the
    suffix minimum of the upper bounds, which is b's return (the positions
    between have no required holder, the ones above returned later).  Twin:
    a claims position M instead."""
    M = L - 1
    assert 0 <= p and d >= 1 and p + d < M
    k = _Key(*base)
    k.ladder(0, p)
    k.call(W, val(p), N, N)
    for j in range(1, d):
        k.call(W, val(p + j), N, k.ver(p + j))
    b = k.ok(W, val(p + d), N, k.ver(p + d))
    k.ladder(p + d + 1, M)
    a = k.ok(W, val(p), N, k.ver(M if good else p))
    return k.plant("order_mut", "L=%d p=%d d=%d" % (L, p, d), good, a, (ORDER, a, b, 0))


def order_mut_edges(L):
    """(p, d): p and p+1 on the two sides of every thread edge (per t) of the
    suffix minimum; p, and p+d, on each side of the edges of order_edges at
    distances 1, 2, one wave and three waves."""
    per = (L + 255) // 256
    M = L - 1
    out = set()
    for t in range(1, 256):  # every thread edge, straddled
        if per * t + 1 < M:
            out.add((per * t - 1, 1))
    for e in order_edges(L):
        for d in (1, 2, 64 * per, 3 * 64 * per):
            for p in (e - 1, e, e - d, e - d - 1):  # p at the edge, and p+d at it
                if p >= 0 and p + d < M:
                    out.add((p, d))
    return sorted(out)


def order_edges(L):
    """Thread edges (the first and the last thread's, one inside a wave) and
    every wave edge of the suffix minimum over L indices."""
    per = (L + 255) // 256
    return sorted({per * t for t in (1, 100, 255)} | {64 * per * w for w in (1, 2, 3)})


# ---- CLAIMS across strides --------------------------------------------------
CLAIMS_AT = ((255, 511), (256, 512), (300, 520))


def claims_far(i1, i2, good=False, base=(0, 0, N)):
    """Three reads of version v0 + 1 with values x, x and y: the y-reader is
    record 0 and returns last, the x-readers are records i1 and i2 (different
    256-strides; both find the clash, the lower pair wins)."""
    k = _Key(*base)
    x, y = 4, 6
    ry = k.call(R, x if good else y, N, k.ver(0))
    k.ok(W, x, N, k.ver(0))
    k.nil_reads(i1)
    r1 = k.ok(R, x, N, k.ver(0))
    k.nil_reads(i2)
    k.ok(R, x, N, k.ver(0))
    k.ret(ry)
    return k.plant("claims_far", "i1=%d i2=%d" % (i1, i2), good, ry, (CLAIMS, ry, r1, 0))


# ---- PAIR against a required holder ----------------------------------------
PAIR_Q = (0, 1, 255, 256, 257)


def pair_far(q, two=False, at=0, good=False, base=(0, 0, N)):
    """q >= 1: the holder H of q-1 (value hv) is called early and returns
    last; meanwhile a crashed filler of value w holds q-1 for the consumers
    of q: reads [v0+q w] at records 300 and 520 (threads 44 and 8 of two
    strides: the lower record is not the lower thread's) and a CAS at q
    expecting w at a higher record.  At H's return every consumer disagrees
    with it: the lowest q, then the lowest consumer record.  two: H is a CAS
    expecting another value than the ladder left at q-2 (the initial one for
    q = 1) — a clash at q-1 as well, which is lower.  q = 0: a CAS at
    position 0 against the initial value, as record `at`."""
    k = _Key(*base)
    if q == 0:
        k.nil_reads(at)
        e = _wrong(k.init)
        c = k.ok(C, 2, k.init if good else e, k.ver(0))
        return k.plant("pair_far", "q=0 at=%d" % at, good, c, (PAIR, -1, c, 0))
    hv, w = 2, 5
    k.ladder(0, q - 1)
    e = k.before(q - 1)
    if two:
        h = k.call(C, w if good else hv, _wrong(e), k.ver(q - 1))
    else:
        h = k.call(W, w if good else hv, N, k.ver(q - 1))
    k.call(W, w, N, N)
    k.nil_reads(300)
    r1 = k.ok(R, w, N, k.v0 + q)
    k.nil_reads(520)
    k.ok(R, w, N, k.v0 + q)
    k.nil_reads(530)
    k.ok(C, 1, w, k.ver(q))
    k.ret(h)
    if two:
        # (its twin would need two fields: the two-clash plants have none)
        assert not good
        cert = (PAIR, len(k.recs[:q - 1]) - 1 if q >= 2 else -1, h, q - 1)
    else:
        cert = (PAIR, h, r1, q)
    return k.plant("pair_far", "q=%d two=%d" % (q, int(two)), good, h, cert)


# ---- the list of version-less candidates; Hall's condition over all --------
def hall_key(m, layout="front", lead=0, pad=0, good=False, base=(0, 0, N), family="ulist"):
    """m open positions 0..m-1, each needed and given its value by a read
    [v0+g+1 x_g] (x_g = 10 + g, but x_{m-1} = x_0), and m version-less
    crashed candidates: one of value x_g for g < m-1 — every third a CAS
    expecting x_{g-1} — and a decoy of a value nobody needs (it keeps the
    last read reachable).  Every position has exactly one candidate, the
    first and the last the same one: m positions, m - 1 candidates.  A
    candidate the list drops, doubles or misplaces leaves a position empty
    (HALL over one position, another certificate).  Twin: the decoy writes
    x_0.  layout: the candidates all called first ("front"), or each just
    before its position's read ("inter": every position's deadline cuts the
    list short).  lead: [nil nil] reads before everything.  m = 1: the decoy
    alone, position 0 empty."""
    k = _Key(*base)
    k.nil_reads(lead)
    x = [10 + g for g in range(m)]
    x[m - 1] = x[0]

    def cand(g):
        if g == m - 1:
            k.call(W, x[0] if good else 9, N, N)  # the decoy
        elif g % 3 == 2:
            k.call(C, x[g], x[g - 1], N)
        else:
            k.call(W, x[g], N, N)

    if layout == "front":
        for g in range(m):
            cand(g)
    last = -1
    for g in range(m):
        if layout == "inter":
            cand(g)
        last = k.ok(R, x[g], N, k.ver(g))
    tag = "m=%d %s lead=%d n=%d" % (m, layout, lead, max(pad, len(k.recs)))
    return k.plant(family, tag, good, last, (HALL, -1, -1, m), range(m), pad=pad)


ULIST_N = (255, 256, 257, 511, 512, 513, 1023, 1025)
ULIST_NU = (1, 2, 255, 256, 257)


# ---- deadlines --------------------------------------------------------------
DEADLINE_P = (0, 255, 256)


def deadline(p, how, good=False, base=(0, 0, N)):
    """Position p is open; a read [v0+p+1 nil] returns (the deadline); a read
    [v0+p+1 y] returns later (the cut).  how:
      "ulist": a crashed write of x and one of z are called before the
        deadline (not candidates: the wrong value, yet the scan must go on
        past them), a crashed write of y just after it — in the prefix, and
        ruled out by the deadline alone.  Position p is empty.
      "pin": the same with a pending :ok write of y pinned at p.
      "ulist_ok" / "pin_ok": the write of y is called just before the
        deadline and is p's candidate; a read [v0+p+2 w] then finds
        position p+1 empty: p + 1, not p.
    Twin of the first two: the write of y called one tick earlier, before the
    deadline (the same record order); of the last two: the last read is
    [v0+p+1 y] again."""
    k = _Key(*base)
    x, y, z, w = 1, 4, 2, 6
    pin = how.startswith("pin")
    k.ladder(0, p)
    k.call(W, x, N, N)
    k.call(W, z, N, N)
    r1 = k.call(R, N, N, k.ver(p))
    late = not how.endswith("_ok")
    if late:
        k.ret(r1)
    c2 = k.call(W, y, N, k.ver(p) if pin else N)
    if late and good:
        k.recs[c2][4] = k.recs[r1][5] - 1
    if not late:
        k.ret(r1)
    r2 = k.ok(R, y, N, k.ver(p))
    if late:
        fail, cset = r2, [p]
    else:
        fail = k.ok(R, y if good else w, N, k.ver(p) if good else k.ver(p + 1))
        cset = [p + 1]
    if pin:
        k.ret(c2)
    return k.plant("deadline", "p=%d %s" % (p, how), good, fail, (HALL, -1, -1, 1), cset)


# ---- pending :ok mutations pinned to an open position -----------------------
PINNED_G = (0, 255, 256, 511)


def pinned(g, ops, cas=False, good=False, base=(0, 0, N)):
    """`ops` pending :ok mutations pinned at the open position g, none able
    to hold it: writes of another value than the read [v0+g+1 y] needs, or
    (cas) CAS writing y but expecting another value than the ladder left.
    Twin: the middle one writes y / expects that value.  Only the middle
    one returns (after the read): two returned ops would claim one version."""
    k = _Key(*base)
    y = 4
    k.ladder(0, g)
    pend = []
    for j in range(ops):
        right = good and j == ops // 2
        if cas:
            e = k.before(g)
            pend.append(k.call(C, y, e if right else _wrong(e), k.ver(g)))
        else:
            pend.append(k.call(W, y if right else _wrong(y), N, k.ver(g)))
    r = k.ok(R, y, N, k.ver(g))
    k.ret(pend[ops // 2])  # (the others never return: two would claim one version)
    return k.plant("pinned", "g=%d ops=%d cas=%d" % (g, ops, int(cas)), good, r,
                   (HALL, -1, -1, 1), [g])


# ---- the lowest of several empty positions ---------------------------------
def hall_one(g, good=False, base=(0, 0, N)):
    """Positions g and g+1 open; g's only candidate a crashed write of x,
    g+1's a crashed CAS expecting x.  The read [v0+g+1 y] takes both away at
    once: g needs y, g+1 a CAS that expects y.  g = 255: threads 255 and 0
    of two strides find one each; the lower position is the certificate's.
    A read [v0+g+2 3] called first and returned in between makes g+1
    needed and a write of 3 its holder.  Twin: the read is
    [v0+g+1 x]."""
    k = _Key(*base)
    x, y = 1, 4
    k.ladder(0, g)
    k.call(W, x, N, N)
    k.call(C, 3, x, N)
    r1 = k.call(R, 3, N, k.ver(g + 1))
    r = k.call(R, x if good else y, N, k.ver(g))
    k.ret(r1)
    k.ret(r)
    return k.plant("hall_one", "g=%d" % g, good, r, (HALL, -1, -1, 1), [g])


def hall_one_far(g_lo, g_hi, top, good=False, base=(0, 0, N)):
    """The ladder below g_lo; every position of g_lo .. top-1 but g_lo and
    g_hi has a write pinned to it that never returns (g_lo + 1 and g_lo + 2 have
    two, so the write at `top` stays reachable); then the write pinned at
    `top` returns and makes them all needed at once.  g_lo and g_hi are
    empty, found in different strides; the lower wins.  Twin: the last write
    claims position g_lo."""
    k = _Key(*base)
    k.ladder(0, g_lo)
    pend = []
    for g in range(g_lo + 1, top):
        if g != g_hi:
            pend.append(k.call(W, val(g), N, k.ver(g)))
        if g in (g_lo + 1, g_lo + 2):
            pend.append(k.call(W, val(g), N, k.ver(g)))
    r = k.ok(W, val(top), N, k.ver(g_lo if good else top))
    return k.plant("hall_one", "lo=%d hi=%d top=%d" % (g_lo, g_hi, top), good, r,
                   (HALL, -1, -1, 1), [g_lo])


# ---- PAIR between two open positions ---------------------------------------
PAIR_OPEN_Q = (1, 255, 256, 257, 512)


def pair_open(q, good=False, base=(0, 0, N)):
    """Positions q-1 and q open, each with one candidate, a pending :ok op
    pinned to it: a write of x at q-1, a CAS expecting another value at q.
    The write pinned at q+1 returns and needs both.  (The form with a
    required holder at q-1 cannot be reached: a CAS that expects another
    value than a required holder left is no candidate of q, which is then
    empty — hall_one's stage.)  Twin: the CAS expects x."""
    k = _Key(*base)
    x = 4
    k.ladder(0, q - 1)
    a = k.call(W, x, N, k.ver(q - 1))
    b = k.call(C, 2, x if good else _wrong(x), k.ver(q))
    r = k.ok(W, 1, N, k.ver(q + 1))
    k.ret(a)
    k.ret(b)
    return k.plant("pair_open", "q=%d" % q, good, r, (PAIR, a, b, q))


# ---- PROOF ------------------------------------------------------------------
def proof_tokens(chain, k_free, conflict):
    """The case splits of proof_key's refutation in preorder: every free
    position in turn (two cases each), then the first conflict position
    (conflict - 1 cases), and for conflict = 4 the second one below each of
    its cases (two cases); the rest is forced."""
    def sub(i):
        p = chain + i
        if i < k_free:
            return [tok(BRANCH, p, 2)] + sub(i + 1) * 2
        if conflict == 3:
            return [tok(BRANCH, p, 2)]
        return [tok(BRANCH, p, 3)] + [tok(BRANCH, p + 1, 2)] * 3
    return sub(0)


def proof_nodes(chain, k_free, conflict):
    """Iterations of the device's search loop (cert.hip, ++nodes): one per
    forced step of the chain, one per split, and per innermost case one
    forced step and the closing iteration."""
    leaf = 1 + 2 * 2 if conflict == 3 else 1 + 3 * (1 + 2 * 2)
    return chain + (2 ** k_free - 1) + 2 ** k_free * leaf


def proof_depth(k_free, conflict):
    return k_free + conflict - 2


def proof_key(k_free, conflict, chain=0, pad=0, good=False, base=(0, 0, N)):
    """helpers.proof_cap_key after `chain` positions that each have exactly
    one candidate (forced, in turn, before any split): k_free positions with
    two crashed writes of their value each, then `conflict` positions that
    all need value 9 with conflict - 1 crashed writes of it.  Open positions:
    chain + k_free + conflict.  Fails at the read of the last conflict
    position.  Twin: that read asks for no value.
    k_free = 0: the conflict alone would be outnumbered (Hall's condition,
    no search), so one more position follows it, needing value 8 with
    conflict - 1 crashed writes of it (as many candidates as the conflict's
    positions have: the search splits the lower one).  Its read is called
    after the failing read and returns before it, so both are required."""
    assert conflict in (3, 4)
    k = _Key(*base)
    for p in range(chain):
        k.call(W, 100 + p, N, N)
        k.ok(R, 100 + p, N, k.ver(p))
    last = -1
    for i in range(k_free + conflict):
        p = chain + i
        if i < k_free:
            k.call(W, 10 + i, N, N)
            k.call(W, 10 + i, N, N)
        elif i == k_free:
            for _ in range(conflict - 1):
                k.call(W, 9, N, N)
            if k_free == 0:
                for _ in range(conflict - 1):
                    k.call(W, 8, N, N)
        v = 10 + i if i < k_free else 9
        if good and i == k_free + conflict - 1:
            v = N
        if k_free == 0 and i == conflict - 1:
            last = k.call(R, v, N, k.ver(p))
            k.ok(R, 8, N, k.ver(p + 1))
            k.ret(last)
        else:
            last = k.ok(R, v, N, k.ver(p))
    toks = proof_tokens(chain, k_free, conflict)
    n = max(pad, len(k.recs))
    tag = "k=%d c=%d chain=%d n=%d" % (k_free, conflict, chain, n)
    nodes, depth = proof_nodes(chain, k_free, conflict), proof_depth(k_free, conflict)
    proved = nodes <= PROOF_NODES and len(toks) <= n and depth <= (n + 2) // 4
    cert = (PROOF, -1, -1, len(toks)) if proved else NO_CERT
    return k.plant("proof", tag, good, last, cert, toks if proved else (), pad=pad)


PROOF_NODES = 2048
# the largest k_free whose proof fits under the node cap, and the next
# (conflict = 3: 3 * 2^(k+1) - 1 nodes; conflict = 4: 17 * 2^k - 1)
NODE_CAP_K = {3: (8, 9), 4: (6, 7)}
PROOF_OPEN = (63, 64, 65, 128)


def proof_size(k_free, conflict, chain=0):
    return 2 * chain + 3 * k_free + 2 * conflict - 1 + (conflict if k_free == 0 else 0)


@functools.lru_cache(maxsize=None)
def proof_plants():
    out = []
    for conflict in (3, 4):
        for depth in (1, 2, 3, 4):
            kf = depth - (conflict - 2)
            if kf < 0:
                continue
            n0 = proof_size(kf, conflict)
            n_tok = len(proof_tokens(0, kf, conflict))
            # every n % 4 from the smallest size the proof's tokens fit in;
            # among them the sizes whose frame cap is the depth, or one more
            lo = max(n0, n_tok)
            sizes = set(range(lo, lo + 4))
            for nf in (depth, depth + 1):
                sizes |= {n for n in range(4 * nf - 2, 4 * nf + 2) if n >= lo}
            for n in sorted(sizes):
                out += [proof_key(kf, conflict, pad=n), proof_key(kf, conflict, pad=n, good=True)]
        # no token room: the bare key of depth 4
        out += _both(proof_key, 5 - conflict + 1, conflict)
        # open positions across the lanes of the wave, a forced chain first
        for ng in PROOF_OPEN:
            kf = 2
            chain = ng - kf - conflict
            out += [proof_key(kf, conflict, chain=chain),
                    proof_key(kf, conflict, chain=chain, good=True)]
        # the node cap
        for kf in NODE_CAP_K[conflict]:
            n_tok = len(proof_tokens(0, kf, conflict))
            out += _both(proof_key, kf, conflict, pad=min(n_tok + 7, 1100))
    return tuple(out)


# ---- PROOF deeper than it is wide: the frame cap -----------------------------
DEEP_D = (3, 4, 5, 6)


def proof_deep(d, pad=0, good=False, base=(0, 0, N)):
    """A refutation of d nested splits and d tokens in 2 d + 3 records, so
    that the frame cap (n + 2) / 4 can lie below the depth: two writes of 1
    and 2 pinned at position 0, two CAS pinned at each of 1 .. d-1, both
    expecting 2 and writing 1 and 2, two CAS pinned at d that expect 3 —
    none of them ever returns — and a write pinned at d+1 that returns and
    needs them all.  Every position has two candidates; at each the case
    "writes 1" leaves the next position empty and the case "writes 2" goes
    on, until position d, which no value suits.  With fewer than d frames
    the search gives up at its next split: no certificate.  Twin: one CAS
    at d expects 2."""
    k = _Key(*base)
    k.call(W, 1, N, k.ver(0))
    k.call(W, 2, N, k.ver(0))
    for p in range(1, d):
        k.call(C, 1, 2, k.ver(p))
        k.call(C, 2, 2, k.ver(p))
    k.call(C, 1, 3, k.ver(d))
    k.call(C, 2, 2 if good else 3, k.ver(d))
    r = k.ok(W, 1, N, k.ver(d + 1))
    n = max(pad, len(k.recs))
    toks = [tok(BRANCH, p, 2) for p in range(d)]
    proved = d <= (n + 2) // 4
    return k.plant("proof_deep", "d=%d n=%d" % (d, n), good, r,
                   (PROOF, -1, -1, d) if proved else NO_CERT, toks if proved else (), pad=pad)


def proof_deep_sizes(d):
    """Key sizes at which the frame cap is d - 1, d and d + 1."""
    return [n for nf in (d - 1, d, d + 1) for n in range(4 * nf - 2, 4 * nf + 2) if n >= 2 * d + 3]


# ---- Hall's condition over many positions, in a key of m + 1 records --------
def hall_pinned(m, good=False, base=(0, 0, N)):
    """m open positions made needed at once by a read [v0+m nil]: positions
    0 .. m-3 each have a write pinned to them that never returns, and one
    crashed version-less write is everybody's candidate — the only one of
    m-2 and m-1.  A write pinned beyond them keeps the read reachable.
    m positions, m - 1 candidates.  Twin: that write is pinned at m-1."""
    assert m >= 3
    k = _Key(*base)
    for g in range(m - 2):
        k.call(W, val(g), N, k.ver(g))
    k.call(W, 5, N, N)
    k.call(W, 6, N, k.ver(m - 1 if good else m + 5))
    r = k.ok(R, N, N, k.v0 + m)
    return k.plant("hall_all", "m=%d pinned" % m, good, r, (HALL, -1, -1, m), range(m))


# ---- the families -----------------------------------------------------------
FAMILIES = ("order_mut", "claims_far", "pair_far", "ulist", "deadline", "pinned", "hall_one",
            "hall_all", "pair_open", "proof", "proof_deep", "base")
HALL_ALL_M = (1, 2, 255, 256, 257, 600)


def _both(f, *a, **kw):
    return [f(*a, **kw), f(*a, good=True, **kw)]


def _ulist_plants():
    out = []
    for n in ULIST_N:
        for nu in ULIST_NU + (100,):
            for layout in ("front", "inter"):
                # (hundreds of crashed writes pending at once: no search decides that)
                if 2 * nu > n or (layout == "front" and nu > 2):
                    continue
                # the candidates from record 0, and at the key's end
                for lead in sorted({0, n - 2 * nu}):
                    out += _both(hall_key, nu, layout, lead, n)
    return out


@functools.lru_cache(maxsize=None)
def family_plants(family):
    out = []
    if family == "order_mut":
        for L in ORDER_L:
            for p, d in order_mut_edges(L):
                out += _both(order_mut, L, p, d)
    elif family == "claims_far":
        for i1, i2 in CLAIMS_AT:
            out += _both(claims_far, i1, i2)
    elif family == "pair_far":
        for at in (0, 255, 256, 600):
            out += _both(pair_far, 0, at=at)
        for q in PAIR_Q[1:]:
            out += _both(pair_far, q)
            out.append(pair_far(q, two=True))
    elif family == "ulist":
        out = _ulist_plants()
    elif family == "deadline":
        for p in DEADLINE_P:
            for how in ("ulist", "pin", "ulist_ok", "pin_ok"):
                out += _both(deadline, p, how)
    elif family == "pinned":
        for g in PINNED_G:
            for ops in (1, 2, 3):
                for cas in (False, True):
                    out += _both(pinned, g, ops, cas)
    elif family == "hall_one":
        for g in (0, 10, 255, 511):
            out += _both(hall_one, g)
        out += _both(hall_one_far, 10, 300, 310)
        out += _both(hall_one_far, 255, 256, 520)
    elif family == "hall_all":
        for m in HALL_ALL_M:
            # (a read per position: 2 m records; past 1,100, one read for all)
            out += _both(hall_key, m, "inter", family="hall_all") if 2 * m <= 1100 else \
                _both(hall_pinned, m)
        out += _both(hall_pinned, 257)
    elif family == "pair_open":
        for q in PAIR_OPEN_Q:
            out += _both(pair_open, q)
    elif family == "proof":
        out = list(proof_plants())
    elif family == "proof_deep":
        for d in DEEP_D:
            for n in proof_deep_sizes(d):
                out += _both(proof_deep, d, n)
    elif family == "base":
        for b in BASES:
            out += base_set(b)
    return tuple(out)


def base_set(base):
    """One plant of every certificate above (and its twin) on another first
    call or another initial version and value."""
    out = []
    out += _both(order_mut, 257, 63, 64, base=base)
    out += _both(claims_far, 255, 511, base=base)
    out += _both(pair_far, 0, at=3, base=base)
    out += _both(pair_far, 256, base=base)
    out.append(pair_far(2, two=True, base=base))
    out += _both(hall_key, 100, "inter", 0, 257, base=base)
    out += _both(hall_key, 40, "inter", 5, 0, base=base, family="hall_all")
    for how in ("ulist", "pin", "ulist_ok", "pin_ok"):
        out += _both(deadline, 3, how, base=base)
    out += _both(pinned, 0, 2, True, base=base)
    out += _both(pinned, 5, 3, False, base=base)
    out += _both(hall_one, 255, base=base)
    out += _both(pair_open, 256, base=base)
    out += _both(proof_key, 2, 3, base=base)
    out += _both(proof_key, 2, 4, 10, 40, base=base)
    out += _both(proof_deep, 4, 13, base=base)
    out += _both(proof_deep, 4, 14, base=base)
    out += _both(hall_pinned, 70, base=base)
    return out


def all_plants():
    return [pl for fam in FAMILIES for pl in family_plants(fam)]
