"""Deterministic version-less keys for the first witness stage
(witness_search_kernel: ws_search and its helpers, csrc/witness_search.hip),
placed where the depth-first search changes hands:

  64       window slots; 64 records per chunk of the streamed event pass
  5 / 8    nodes per bucket / buckets probed of the dead-end cache
  65,536   steps (kWitnessNodeCap)
  128      records per carving unit of a wave's frames, events and slots
           (witness_round)

No randomness.  Records are [f, value, expected, version, call, ret] as in
helpers.py; every version is nil, so the search tiers decide the key and it
reaches the stage with witness kind NONE.  Each builder returns a
planted.Plant: the records, the verdict and the fail op by construction.  How
many steps, cache hits, stored, spilled and dropped dead ends a plant takes is
not claimed here: tests/test_planted_witness.py takes them from
tests/search_order_ref.py and asserts that every edge is hit.

A back-fan is the unit: m crashed writes of distinct values b+1 .. b+m, all
open, then :ok reads of b+m, b+m-1, .., b+1, one after the other.  The only
order is W_m R_m W_m-1 R_m-1 ..; the search tries the lowest slot first, so it
walks subsets x last value before it finds that order, caching dead ends all
the way.  When the last read has returned every write of the fan is
linearized: one configuration is left, and another fan can follow."""
import functools

from helpers import C, N, R, W
from planted import Plant, interleave as _interleave
from planted_search import NOBODY, _Key, _tag

FILL = 50  # the value of the sequential :ok writes around a fan


def _fan(k, m, base=0, reads=None, crashed_reads=()):
    """One back-fan into key k: its writes, crashed reads of the fan values
    `crashed_reads` (legal mid-fan: taken first, forced, and ranked), then the
    first `reads` (default: all m) of its :ok reads."""
    for v in range(1, m + 1):
        k.crashed(W, base + v)
    for v in crashed_reads:
        k.crashed(R, base + v)
    for v in range(m, m - (m if reads is None else reads), -1):
        k.ok(R, base + v)


def backfan(m, crashed_reads=()):
    k = _Key()
    _fan(k, m, crashed_reads=crashed_reads)
    return Plant("backfan", _tag("backfan", m=m, cr=tuple(crashed_reads)), k.recs, 1, -1)


def chain(ms):
    """Back-fans one after the other, fan i with the values 20 i + 1 .. ."""
    k = _Key()
    for i, m in enumerate(ms):
        _fan(k, m, base=20 * i)
    return Plant("chain", _tag("chain", m=tuple(ms)), k.recs, 1, -1)


def ahead(p, m=9):
    """p sequential :ok writes, then an m-fan: its records are p .. p + 2m - 1,
    its crashed writes in slots 0 .. m - 1."""
    k = _Key()
    for _ in range(p):
        k.ok(W, FILL)
    _fan(k, m)
    return Plant("ahead", _tag("ahead", p=p, m=m), k.recs, 1, -1)


def opened(f, m=9):
    """f crashed reads of a value nobody writes — never legal, each holds a
    slot for good — then an m-fan: f + m + 1 ops are open while a read of the
    fan is.  The search tiers give a crashed read no slot."""
    k = _Key()
    k.crashed(R, NOBODY, count=f)
    _fan(k, m)
    return Plant("opened", _tag("opened", f=f, m=m), k.recs, 1, -1)


def reuse(m, good=True):
    """An m-fan in slots that are not contiguous, with :ok [nil nil] reads
    (always legal, so forced at once) as the other slot holders.  L, A and B
    are called first (slots 0, 1, 2).  A returns behind the first crashed
    write (slot 3) and the second takes its slot; the others go above.  L
    returns after the fan's second read and B after the third, so the fan
    stands in slots 1, 3, 4, .. round B.  The fan's reads take the slot above
    the writes until L's return frees slot 0; a rewind to a frame below that
    return puts L back where a read of the fan was in between."""
    assert m >= 5
    k = _Key()
    l, a, b = k.call(R, N), k.call(R, N), k.call(R, N)
    k.crashed(W, 1)
    k.ret(a)
    for v in range(2, m + 1):
        k.crashed(W, v)
    k.ok(R, m)
    k.ok(R, m - 1)
    k.ret(l)
    k.ok(R, m - 2)
    k.ret(b)
    for v in range(m - 3, 1, -1):
        k.ok(R, v)
    fail = k.ok(R, 1 if good else NOBODY)
    return Plant("reuse", _tag("reuse", m=m, good=int(good)), k.recs, int(good), -1 if good else fail)


def unwritten(m, done):
    """An m-fan with `done` of its reads, then an :ok read of a value nobody
    wrote: the key fails there, the order is wanted at the event before that
    read's return, with the fan's crashed writes open across it.  done = 0:
    the failing read is the key's first return."""
    k = _Key()
    _fan(k, m, reads=done)
    fail = k.ok(R, NOBODY)
    k.ok(W, FILL)  # (beyond the cut)
    return Plant("unwritten", _tag("unwritten", m=m, done=done), k.recs, 0, fail)


def deadline():
    """The pick among candidates when the returning op is none of them: a
    crashed write of 2 (slot 0), :ok writes of 1 and of 2 (slots 1, 2) and X,
    an :ok CAS 2 -> 5 (slot 3), open together; X returns first, then the
    write of 2, then the write of 1, then a read of 1.  At X's return X is
    not legal; of the three writes the :ok write of 2 has the earliest return
    and goes first — not the lowest slot (the crashed write, which goes
    last), nor the lower :ok slot — then X; the crashed write is never
    ranked.  Trying the lowest slot first would find another valid order."""
    k = _Key()
    k.crashed(W, 2)
    a, b, x = k.call(W, 1), k.call(W, 2), k.call(C, 5, 2)
    k.ret(x)
    k.ret(b)
    k.ret(a)
    k.ok(R, 1)
    return Plant("deadline", "deadline", k.recs, 1, -1)


def write_reads(r):
    """A write, then r reads of it: r + 1 steps, one per op ranked."""
    k = _Key()
    k.ok(W, 1)
    for _ in range(r):
        k.ok(R, 1)
    return Plant("write_reads", _tag("write_reads", r=r), k.recs, 1, -1)


def length(n, m=7):
    """n records: sequential :ok writes, an m-fan in the middle, sequential
    :ok writes and reads of them."""
    k = _Key()
    for _ in range((n - 2 * m) // 2):
        k.ok(W, FILL)
    _fan(k, m)
    tail = 0
    while len(k.recs) < n:
        k.ok(R if tail % 2 else W, FILL)
        tail += 1
    return Plant("length", _tag("length", n=n, m=m), k.recs, 1, -1)


BACKFANS = tuple(range(1, 11))
CAPPED = (11,)                       # a lone fan past the node cap
FORCED = ((5, (3,)), (6, (6, 1)), (8, (4, 5)))  # (m, crashed reads of these fan values)
CHAINS = ((3, 4), (5, 5, 5), (10, 9), (10, 10), (10, 10, 8), (10, 10, 10))
AHEAD_P = tuple(range(55, 65)) + tuple(range(119, 129))
OPENED_F = (53, 54, 55)              # 63, 64, 65 ops open beside a 9-fan
UNWRITTEN = ((6, 6), (7, 3), (5, 0), (9, 9))
WRITE_READS = (1, 30)
LENGTHS = (127, 128, 129, 255, 256, 257)


@functools.lru_cache(maxsize=None)
def plants():
    """Every hand plant, in family order."""
    out = [backfan(m) for m in BACKFANS + CAPPED]
    out += [backfan(m, cr) for m, cr in FORCED]
    out += [chain(ms) for ms in CHAINS]
    out += [ahead(p) for p in AHEAD_P]
    out += [opened(f) for f in OPENED_F]
    out += [reuse(6), reuse(8), reuse(6, good=False)]
    out += [unwritten(m, done) for m, done in UNWRITTEN]
    out += [deadline()]
    out += [write_reads(r) for r in WRITE_READS]
    out += [length(n) for n in LENGTHS]
    return tuple(out)


FAMILIES = ("backfan", "chain", "ahead", "opened", "reuse", "unwritten", "deadline", "write_reads", "length")


def family(name):
    return tuple(pl for pl in plants() if pl.family == name)


def interleaved():
    """The hand plants as one batch, long and short keys alternating."""
    return tuple(_interleave(plants()))
