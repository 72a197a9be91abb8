"""Deterministic version-less keys for the frontier-search tiers
(lds_tier_kernel, hbm_tier_kernel, hbm_coop_kernel, the dump kernels behind
lc_check_frontiers), with set sizes, window occupancy, record counts and value
ids chosen to land where check_kernel.hip changes hands:

  128            configurations per LDS region (kLdsCap, LdsStore::insert)
  1,688 / 3,456  pool entries of the cooperative tier (CoopTab<LT>::kPool)
  2^14           configurations per set on the first HBM rung (kHbmCap[0])
  64             window slots; 64 records per streamed chunk (kWave)
  255            cooperative returns per 8-bit LDS epoch (kLepochMask)
  15             the first value id past the value-legality table (kVTab)

The 2^18 and 2^21 rungs of kHbmCap are out of scope: a key that large takes
the oracle and one wavefront far longer than a test of a few seconds may.

No randomness.  Records are [f, value, expected, version, call, ret] as in
helpers.py; every version is nil, so the version-order and gap tiers pass
every key on.  Each builder returns a planted.Plant: the records, the verdict
and the fail op by construction.  The set sizes a plant reaches are not
claimed here: tests/test_planted_search.py takes them from search_ref and
asserts that every edge is hit exactly.

A fan is the unit: classes[i] crashed writes of value i + 1, all open
together, optional crashed CAS classes (expected, value, count) as tuners,
then one :ok op X called after all of them, then :ok reads.  (A tuner CAS
v -> v beside the class of value v acts as one class of 1 + a (c + 1) counts
in c + a slots: sizes no 64-slot window could otherwise reach.)  X's return
expands everything; by the deadline order a visited configuration is a count
per class plus the last value, so for a pure fan |R| = prod(c_i + 1) and
|W| = 1 + sum_i c_i prod_{j != i}(c_j + 1).  The tuned fans below were picked
by enumerating classes and tuners with search_ref."""
import functools

from helpers import INF, C, N, R, W
from planted import Plant, interleave as _interleave

NOBODY = 99  # a value no op of any plant writes


class _Key:
    """Records appended in call order, one event index per call / return."""

    def __init__(self):
        self.recs, self.t = [], 0

    def crashed(self, f, value, expected=N, count=1):
        for _ in range(count):
            self.recs.append([f, value, expected, N, self.t, INF])
            self.t += 1

    def call(self, f, value, expected=N):
        self.recs.append([f, value, expected, N, self.t, INF])
        self.t += 1
        return len(self.recs) - 1

    def ret(self, i):
        self.recs[i][5] = self.t
        self.t += 1

    def ok(self, f, value, expected=N):
        """Called and returned with nothing in between; its record index."""
        i = self.call(f, value, expected)
        self.ret(i)
        return i

    def stage(self, classes, tuners=(), x=0, values=None):
        """One fan: the crashed writes (of values[i], by default i + 1), the
        tuners, then X — an :ok write of x, or with x=None an :ok read of
        NOBODY.  Returns X's record index."""
        for i, c in enumerate(classes):
            self.crashed(W, values[i] if values else i + 1, count=c)
        for e, v, c in tuners:
            self.crashed(C, v, e, count=c)
        return self.ok(R, NOBODY) if x is None else self.ok(W, x)

    def collapse(self, classes, values=None):
        """After a stage whose X wrote another value: reads of the class
        values in turn, as many rounds as the largest class.  Each read keeps
        only the configurations that linearize one more write of its value
        after the read before it, so (classes of equal size, two or more
        classes or a single write) one configuration is left at the end,
        with every crashed write linearized — and retired."""
        for rnd in range(max(classes)):
            for i, c in enumerate(classes):
                if c > rnd:
                    self.ok(R, values[i] if values else i + 1)


def _tag(family, **kw):
    return "%s %s" % (family, " ".join("%s=%s" % (k, "".join(str(v).split()))
                                       for k, v in sorted(kw.items())))


def _close(k, x, closer):
    """The end of a fan key whose X has record index x (see fan)."""
    if closer == "x":
        return x
    if closer == "read":
        return k.ok(R, NOBODY)
    k.ok(R, 0)
    return -1


def fan(classes, tuners=(), closer="valid"):
    """closer "valid": X writes 0 and a read of 0 follows (every configuration
    keeps it).  "read": the read sees NOBODY instead — the frontier empties
    one return after the large one, and that return visits what is left of
    the fan.  "x": X itself reads NOBODY — |W| is full, |R| = 0, the key
    fails at the large return."""
    k = _Key()
    x = k.stage(classes, tuners, x=None if closer == "x" else 0)
    fail = _close(k, x, closer)
    return Plant("fan", _tag("fan", c=tuple(classes), t=tuple(tuners), closer=closer), k.recs,
                 int(fail < 0), fail)


def two_fans(first, tuners, second, closer="valid"):
    """A second fan opened while the first one's frontier (its |R|) stands:
    the second X's return is entered with that many configurations."""
    k = _Key()
    k.stage(first, tuners)
    n = len(first)
    x = k.stage(second, x=None if closer == "x" else 0, values=[n + 1 + i for i in range(len(second))])
    fail = _close(k, x, closer)
    return Plant("two_fans", _tag("two_fans", a=tuple(first), t=tuple(tuners), b=tuple(second),
                                  closer=closer), k.recs, int(fail < 0), fail)


def one_two_one(classes, good=True):
    """Frontier 1 -> several -> 1: the lone configuration's walk branches at
    X (the return is redone on the general path), the reads collapse the
    frontier back to one configuration, then a read legal in it (it takes no
    slot) and an :ok write follow; the last read sees that write (or,
    good=False, NOBODY)."""
    k = _Key()
    k.stage(classes)
    k.collapse(classes)
    k.ok(R, len(classes))   # the value the last collapsing read left
    k.ok(W, 7)
    fail = k.ok(R, 7 if good else NOBODY)
    return Plant("one_two_one", _tag("one_two_one", c=tuple(classes), good=int(good)), k.recs,
                 int(good), -1 if good else fail)


def epochs(threes, twos, good=True):
    """`threes` stages of fan (1, 1) and `twos` of fan (1), each collapsed to
    one configuration: three and two returns on the general path apiece, so
    3 * threes + 2 * twos in all — the cooperative tier's 8-bit LDS epoch
    wraps after 255.  A last read sees the value the last stage left (or
    NOBODY)."""
    k = _Key()
    for s in range(threes + twos):
        classes = (1, 1) if s < threes else (1,)
        k.stage(classes)
        k.collapse(classes)
    fail = k.ok(R, (2 if twos == 0 else 1) if good else NOBODY)
    return Plant("epochs", _tag("epochs", threes=threes, twos=twos, good=int(good)), k.recs,
                 int(good), -1 if good else fail)


def window(slots, variant="plain"):
    """`slots` ops holding a window slot at once (the window has 64).
    "plain": slots - 1 crashed writes of value 1 (one class: the frontier
    stays at `slots` configurations), then X, an :ok write of 0, and a read
    of it.
    "reads": an :ok write of 3 first (it returns and is retired), then
    `slots` crashed writes of 1, then reads that take no slot: [nil nil], a
    crashed one, and a read of 3 — legal in the lone configuration.
    "reuse": among slots - 2 crashed writes of 1 an :ok write Y of 2 stays
    open; a read of 2 takes the last slot, and its return puts Y into every
    configuration: Y is retired before it returns.  A crashed write and an
    :ok write of 0 then take Y's and the read's slots."""
    k = _Key()
    if variant == "reads":
        k.ok(W, 3)
        k.crashed(W, 1, count=slots)
        k.ok(R, N)
        k.crashed(R, 5)
        k.ok(R, 3)
    elif variant == "reuse":
        k.crashed(W, 1, count=10)
        y = k.call(W, 2)
        k.crashed(W, 1, count=slots - 12)
        k.ok(R, 2)
        k.ret(y)
        k.crashed(W, 1)
        k.ok(W, 0)
        k.ok(R, 0)
    else:
        k.crashed(W, 1, count=slots - 1)
        k.ok(W, 0)
        k.ok(R, 0)
    return Plant("window", _tag("window", slots=slots, v=variant), k.recs, 1, -1)


CHUNK = 64
CHUNKED_N = (63, 64, 65, 127, 128, 129, 192, 193)


def chunked(n, call_first=False, good=True):
    """n records.  Before every multiple b of 64 up to n: a fan (2, 2) as
    records b-6 .. b-3, X as record b-2 (the frontier is now 9 configurations
    in a region), and a read of X's value as record b-1, left open — the
    record stream reloads after its call.  The first event after the reload
    is that read's return, or with call_first the call of record b (another
    read) and then the return.  Reads then collapse the frontier; everything
    else is :ok writes and reads one at a time.  good=False: the read before
    the last reload sees NOBODY, so the first return after that reload
    fails.  The key is the first n records of this layout."""
    k = _Key()
    last = n // CHUNK * CHUNK
    fail = -1
    v, cur = 3, None  # the next filler value; the value the lone configuration holds
    while len(k.recs) < n:
        b = (len(k.recs) // CHUNK + 1) * CHUNK
        if len(k.recs) == b - 6:
            k.stage((2, 2))
            bad = not good and b == last
            r1 = k.call(R, NOBODY if bad else 0)
            assert r1 == b - 1
            if bad:
                fail = r1
            if call_first:
                r2 = k.call(R, 0)
                k.ret(r1)
                k.ret(r2)
            else:
                k.ret(r1)
                k.ok(R, 0)
            k.collapse((2, 2))
            cur = 2
        elif cur is None or len(k.recs) % 2 == 0:
            v = cur = 3 + (v - 2) % 4
            k.ok(W, v)
        else:
            k.ok(R, cur)
    recs = k.recs[:n]
    assert good or 0 <= fail < n
    return Plant("chunked", _tag("chunked", n=n, cf=int(call_first), good=int(good)), recs,
                 int(fail < 0), fail)


# value ids on either side of the cooperative tier's 16-entry legality table
# (ids -1 .. 14 are in it; a configuration holding 15 or more falls back)
VALUE_SETS = ((13, 14), (14, 15), (15, 16), (0, 15), (N, 14))


def values(ids, counts=None, tuners=(), x=7, good=True):
    """A fan whose classes write the value ids `ids` (counts: 3 of each by
    default), X writing x, collapsed for equal counts, and a last read of
    the last id (good=False: of NOBODY)."""
    counts = tuple(counts or (3,) * len(ids))
    k = _Key()
    k.stage(counts, tuners, x=x, values=ids)
    if len(set(counts)) == 1 and not tuners:
        k.collapse(counts, values=ids)
    fail = k.ok(R, ids[-1] if good else NOBODY)
    return Plant("values", _tag("values", ids=tuple(ids), c=counts, t=tuple(tuners), x=x,
                                good=int(good)), k.recs, int(good), -1 if good else fail)


def late_value(good=True):
    """Ids below 15 only through two collapsed fans (the table path), then a
    fan in which id 20 appears (the fallback), then small ids again."""
    k = _Key()
    for ids in ((1, 2), (3, 14), (5, 20), (6, 7)):
        k.stage((2, 2), x=9, values=ids)
        k.collapse((2, 2), values=ids)
    fail = k.ok(R, 7 if good else NOBODY)
    return Plant("values", _tag("late_value", good=int(good)), k.recs, int(good),
                 -1 if good else fail)


# ---- the plants, by group.  Fans are (quantity, classes, tuners, closer):
# the quantity is what tests/test_planted_search.py asserts of search_ref's
# sizes for that key, exactly.

# largest max(|W|, |R|) of a return: kLdsCap = 128
LDS_EDGE = (
    (127, (5, 11), (), "valid"), (127, (5, 11), (), "x"), (127, (1, 2, 6), (), "read"),
    (128, (7, 8), (), "valid"), (128, (7, 8), (), "x"), (128, (1, 2, 3), ((0, 1, 1),), "read"),
    (129, (1, 4, 5), (), "valid"), (129, (1, 4, 5), (), "x"), (129, (3, 6), ((1, 2, 1),), "read"),
)
# largest |R| + |W| of a return: CoopTab<2048>::kPool = 1,688 (4 waves) and
# CoopTab<4096>::kPool = 3,456 (8 and 16 waves)
POOL_EDGE = (
    (1687, (2, 6, 11), ((1, 2, 2),), "valid"), (1687, (5, 5, 6), ((3, 1, 2),), "x"),
    (1688, (2, 6, 13), ((1, 2, 1),), "valid"), (1688, (22, 37), (), "x"),
    (1688, (3, 4, 13), ((0, 3, 1),), "read"),
    (1689, (3, 3, 13), ((3, 0, 1),), "valid"), (1689, (3, 5, 15), ((1, 3, 1),), "x"),
    (3455, (1, 2, 3, 36), (), "valid"), (3455, (1, 6, 33), ((2, 3, 3),), "x"),
    (3456, (23, 24), ((2, 1, 1),), "valid"), (3456, (4, 4, 5, 6), (), "x"),
    (3456, (25, 27), ((2, 0, 1),), "x"),
    (3457, (2, 17, 17), (), "valid"), (3457, (7, 7, 19), (), "x"),
)
# largest |F| entering a return: two fans in sequence, (quantity, first,
# tuners, second, closer) — a cooperative return whose frontier alone
# fills, or does not fit, the pool.  |R| of a fan is a product of per-class
# counts (c + 1, or 1 + a (c + 1) with a CAS v -> v tuner), which 1,689 =
# 3 x 563 and the prime 3,457 are not; a CAS 1 -> 2 and a CAS 2 -> 1 couple
# two classes and reach them
POOL_NF = (
    (1688, (30, 7), ((1, 1, 6),), (1,), "valid"),
    (1689, (10, 14), ((1, 2, 1), (2, 1, 5)), (1,), "valid"),
    (3456, (3, 7, 8, 11), (), (1,), "valid"),
    (3457, (13, 27), ((1, 2, 4), (2, 1, 1)), (1,), "valid"),
)
# largest max(|W|, |R|) of a return: kHbmCap[0] = 2^14 (a 16,385 key is
# decided on the 2^18 rung)
RUNG_EDGE = (
    (16383, (1, 2, 3, 4, 36), (), "valid"), (16383, (1, 2, 3, 4, 36), (), "x"),
    (16384, (5, 9), ((1, 1, 14), (2, 2, 11)), "valid"), (16384, (5, 9), ((1, 1, 14), (2, 2, 11)), "x"),
    (16385, (3, 3, 3, 7, 7), (), "valid"), (16385, (3, 3, 3, 7, 7), (), "x"),
)
# |F| before the failing read: what lc_check_frontiers dumps (128 is the LDS
# dump's capacity; the rest come from its HBM retry)
DUMP_FANS = (
    (127, (42,), ((1, 1, 2),), "read"), (128, (3, 3, 7), (), "read"), (129, (2, 21), ((2, 1, 1),), "read"),
    (4000, (9, 19, 19), (), "read"),
)
# the quantities each table must hit: E - 1, E and E + 1 of every edge
# (POOL_NF: E and E + 1)
EDGES = {"LDS_EDGE": (127, 128, 129), "POOL_EDGE": (1687, 1688, 1689, 3455, 3456, 3457),
         "POOL_NF": (1688, 1689, 3456, 3457), "RUNG_EDGE": (16383, 16384, 16385),
         "DUMP_FANS": (127, 128, 129)}

MIXED_VALUES = ((2, 14, 15, 40), (2, 2, 2, 1))  # ids on both sides of 15 in one fan
EPOCHS = ((84, 1), (85, 0), (84, 2), (85, 1), (169, 2))  # 254, 255, 256, 257, 511 returns

GROUPS = ("small", "lds", "epochs", "pool", "rung", "window65", "dump")


def build(row):
    """The plant of one table row."""
    return fan(*row[1:]) if len(row) == 4 else two_fans(*row[1:])


def with_twins(rows):
    """The plants of a table's rows, and every chosen fan's other two
    variants (the valid key, the failing read, the failing X): their sizes
    are whatever search_ref finds, off the edge as a rule."""
    out, seen = [], set()
    for row in rows:
        for closer in (row[3], "valid", "read", "x"):
            pl = fan(row[1], row[2], closer)
            if pl.tag not in seen:
                seen.add(pl.tag)
                out.append(pl)
    return out


def interleave(plants):
    """Long and short keys alternating, as planted.interleave."""
    return tuple(_interleave(list(plants)))


@functools.lru_cache(maxsize=None)
def group(name):
    """The plants of one group (or of several, "a+b"), long and short keys
    alternating."""
    if "+" in name:
        out = [pl for part in name.split("+") for pl in group(part)]
    elif name == "small":
        out = [one_two_one(c, g) for c in ((1,), (1, 1)) for g in (True, False)]
        out += [window(63), window(64), window(64, "reads"), window(63, "reuse"),
                window(64, "reuse")]
        for n in CHUNKED_N:
            for cf in (False, True):
                out.append(chunked(n, cf))
                if n >= CHUNK:
                    out.append(chunked(n, cf, good=False))
        for ids in VALUE_SETS:
            out += [values(ids), values(ids, good=False)]
        out += [values(*MIXED_VALUES), values(*MIXED_VALUES, good=False),
                values((14, 15), (3, 3), ((15, 14, 2), (14, 15, 1))),
                late_value(), late_value(good=False)]
    elif name == "lds":
        out = with_twins(LDS_EDGE)
    elif name == "epochs":
        out = [epochs(a, b) for a, b in EPOCHS] + [epochs(85, 0, good=False),
                                                   epochs(85, 1, good=False)]
    elif name == "pool":
        out = with_twins(POOL_EDGE) + [build(row) for row in POOL_NF]
    elif name == "rung":
        out = with_twins(RUNG_EDGE)
    elif name == "window65":
        out = [window(65), window(65, "reuse"), window(65, "reads")]
    elif name == "dump":
        out = [build(row) for row in DUMP_FANS]
    else:
        raise KeyError(name)
    return interleave(out)
