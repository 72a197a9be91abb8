"""Deterministic version-less keys for the counted-class search
(counted_tier_kernel behind LC_FLAG_COUNTED_CLASSES, counted_frontier_kernel
behind lc_check_frontiers_counted, witness_counted_kernel behind
LC_FLAG_COUNTED_WITNESS), placed where the rule of csrc/counted.h and the
kernels change hands:

  2^k members      a field one bit wider (width = floor(log2 m) + 1)
  field all ones   the add `word + (1 << shift)` next to a full neighbour
  16 / 17 classes  kCountedMaxClasses; 63 / 64 field bits: one slot / none
  slots            `slots` ops open at once fit, one more does not
  64               records per streamed chunk (`called` across a reload)
  pbit             a pending :ok member of a class's tuple goes first
  1 <-> several    counts carried out of and back into the lone configuration
  2^14             configurations per set on the first capacity (kHbmCap[0])
  15               the first value id past the legality table

No randomness.  Records are [f, value, expected, version, call, ret] as in
helpers.py; every version is nil (one plant of `extremes` aside).  Each builder
returns a planted.Plant: the records, the verdict and the fail op by
construction.  What a plant reaches — member counts, field bits, slots, set
sizes — is not claimed here: tests/test_planted_counted.py takes it from
counted_ref / search_ref and asserts that every edge is hit exactly.

lc_check hands a key to the counted tier only after the slot tiers' 64-slot
window overflowed, so a plant meant for it holds at least 65 crashed mutations
open: its own large class, or the ANCHOR — 65 crashed CAS from a value nobody
writes, never legal, a class of width 7.  Small keys without an anchor
(group "direct") go to lc_check_frontiers_counted, which always counts.

A round is an :ok write of 0 followed by an :ok read of v: the read needs a
write of v linearized after the write of 0, so every round uses up one more
crashed member of a class that writes v."""
import functools

from helpers import C, N, R, W
from planted import Plant, interleave as _interleave
from planted_search import NOBODY, _Key, _tag, fan

ANCHOR = 65
LADDER_M = (1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128, 255, 256)
DIRECT_M = (1, 2, 3, 4, 7, 8)


def _anchor(k):
    k.crashed(C, NOBODY - 1, NOBODY, count=ANCHOR)


def _rounds(k, v, n, w=0):
    last = -1
    for _ in range(n):
        k.ok(W, w)
        last = k.ok(R, v)
    return last


def _plant(family, k, good, fail, **kw):
    return Plant(family, _tag(family, **kw), k.recs, int(good), -1 if good else fail)


def ladder(m, extra=False, anchor=None):
    """m crashed writes of 1, then m rounds of 1 (extra: m + 1, the last read
    fails).  The frontier holds a configuration per count."""
    anchor = m < ANCHOR if anchor is None else anchor
    k = _Key()
    if anchor:
        _anchor(k)
    k.crashed(W, 1, count=m)
    fail = _rounds(k, 1, m + int(extra))
    return _plant("ladder", k, not extra, fail, m=m, extra=int(extra), anchor=int(anchor))


NEIGHBOUR_M = (3, 4, 7, 8)        # the driven class: all ones at 3 and 7, the top bit alone at 4 and 8
NEIGHBOUR_POS = ("first", "middle", "last")


def neighbours(m, pos, twin=None):
    """Classes of crashed writes in a row: a bystander, the driven class (m
    members, all linearized first), the stepped class below it (4 members,
    width 3: one bit short it would carry into the driven field), each
    stepped to full by rounds.  pos: the driven class is the key's first
    class (its field ends at bit 63), a middle one, or the stepped class is
    the last one (its field borders the slots).  twin "driven" / "stepped":
    one round more of that class's value, which fails."""
    k = _Key()
    order = {"first": ("d", "s", "b", "a"), "middle": ("a", "d", "s", "b"),
             "last": ("a", "b", "d", "s")}[pos]
    for c in order:
        if c == "a":
            _anchor(k)
        else:
            k.crashed(W, {"d": 1, "s": 2, "b": 3}[c], count={"d": m, "s": 4, "b": 3}[c])
    _rounds(k, 3, 1)   # the bystander's field: 1 of 3
    _rounds(k, 1, m)
    fail = _rounds(k, 2, 4)
    if twin:
        fail = _rounds(k, 1 if twin == "driven" else 2, 1)
    return _plant("neighbours", k, not twin, fail, m=m, pos=pos, twin=twin or "-")


CLASS_COUNTS = (1, 2, 15, 16, 17)


def class_count(n, extra=False, anchor=True):
    """n classes: the anchor (or, without it, one more one-member class),
    n - 2 one-member CAS classes that are never legal, and last a one-member
    class of writes of 1.  One round of 1 (extra: two, the second fails);
    n = 1: a write and a read of 0 (extra: the read sees NOBODY)."""
    k = _Key()
    if anchor:
        _anchor(k)
    for i in range(n - 2 + (0 if anchor else 1)):
        k.crashed(C, 20 + i, 100 + i)
    if n >= 2:
        k.crashed(W, 1)
        fail = _rounds(k, 1, 1 + int(extra))
    else:
        k.ok(W, 0)
        fail = k.ok(R, NOBODY if extra else 0)
    return _plant("class_count", k, not extra, fail, n=n, extra=int(extra), anchor=int(anchor))


def _one_slot(k, last=127):
    """Nine classes: eight of 127 never-legal CAS and one of `last` crashed
    writes of 1 — 63 field bits and one slot at 127, 64 bits at 128."""
    for i in range(8):
        k.crashed(C, 20 + i, 100 + i, count=127)
    k.crashed(W, 1, count=last)


def nine_classes(last, extra=False):
    """The one-slot layout (last = 127) and its unfit neighbour (128), with
    `last` rounds of 1 (extra: one more, which fails)."""
    k = _Key()
    _one_slot(k, last)
    fail = _rounds(k, 1, last + int(extra))
    return _plant("class_count", k, not extra, fail, nine=last, extra=int(extra))


def slots(n_open, good=True):
    """The anchor (width 7: 57 slots) and n_open :ok writes of 2 open at once
    (one tuple: deadline order makes them a chain), returned in call order,
    then a read of 2 (good=False: of NOBODY)."""
    k = _Key()
    _anchor(k)
    ws = [k.call(W, 2) for _ in range(n_open)]
    for i in ws:
        k.ret(i)
    fail = k.ok(R, 2 if good else NOBODY)
    return _plant("slots", k, good, fail, open=n_open, g=int(good))


def slot_reuse(good=True):
    """57 writes of 2 fill the window; the first returns and is retired; a
    write of 3 called then takes its slot — the lowest."""
    k = _Key()
    _anchor(k)
    ws = [k.call(W, 2) for _ in range(57)]
    k.ret(ws[0])
    y = k.call(W, 3)
    for i in ws[1:]:
        k.ret(i)
    k.ret(y)
    fail = k.ok(R, 3 if good else NOBODY)
    return _plant("slots", k, good, fail, reuse=1, g=int(good))


def one_slot(n_open):
    """The one-slot layout with n_open other ops open at once: 0 (reads that
    take no slot), 1 (a write, then a read of it), 2 (two writes overlap:
    one more than the layout has slots)."""
    k = _Key()
    _one_slot(k)
    if n_open == 0:
        k.ok(R, N)
        k.ok(R, N)
    elif n_open == 1:
        k.ok(W, 0)
        k.ok(R, 0)
    else:
        a = k.call(W, 0)
        b = k.call(W, 2)
        k.ret(a)
        k.ret(b)
        k.ok(R, 2)
    return _plant("slots", k, True, -1, one_slot=n_open)


# (records of class X — crashed writes of 1; whether one more member is the key's last record)
CHUNK_LAYOUTS = (((63, 64, 127, 128), False), ((64, 65, 127, 128), True), ((65, 66, 126, 127), False),
                 ((10, 63, 191), True), ((63, 64, 127, 128), True))


def chunks(xs, last_crashed=False, extra=False):
    """Records 0 .. : :ok writes and reads one at a time, except the records
    `xs` (class X, crashed writes of 1) and the 65 records from 67 on that
    are not in xs (the anchor).  Then len(xs) rounds of 1 (extra: one more,
    which fails), and with last_crashed one more member of X as the key's
    last record — called too late to serve any read."""
    k = _Key()
    left, v = ANCHOR, 0
    while len(k.recs) <= max(xs) or left:
        i = len(k.recs)
        if i in xs:
            k.crashed(W, 1)
        elif i >= 67 and left:
            k.crashed(C, NOBODY - 1, NOBODY)
            left -= 1
        elif i % 2 == 0:
            v = 3 + (i // 2) % 4
            k.ok(W, v)
        else:
            k.ok(R, v)
    fail = _rounds(k, 1, len(xs) + int(extra))
    if last_crashed:
        k.crashed(W, 1)
    return _plant("chunks", k, not extra, fail, xs=tuple(xs), last=int(last_crashed),
                  extra=int(extra))


PENDING_WHEN = ("before", "between", "after", "late")


def pending_ok(when, extra=False):
    """An :ok write Y of 1 beside two crashed writes of 1.  Y returns before
    their calls, between them, after them, or ("late") after the first round
    of 1 — which either Y or a crashed member can then serve.  Two rounds
    (late: three) are valid, one more fails."""
    k = _Key()
    _anchor(k)
    y = k.call(W, 1)
    if when == "before":
        k.ret(y)
    k.crashed(W, 1)
    if when == "between":
        k.ret(y)
    k.crashed(W, 1)
    if when == "after":
        k.ret(y)
    n = 2
    if when == "late":
        _rounds(k, 1, 1)
        k.ret(y)
    fail = _rounds(k, 1, n + int(extra))
    return _plant("pending_ok", k, not extra, fail, when=when, extra=int(extra))


def cas_pair(n, extra=False):
    """CAS classes 0 -> 1 and 1 -> 0 of n members each behind a write of 0:
    reads of 1 and 0 in turn drive each to its member count (extra: one more
    read of 1, which fails)."""
    k = _Key()
    _anchor(k)
    k.crashed(C, 1, 0, count=n)
    k.crashed(C, 0, 1, count=n)
    k.ok(W, 0)
    for _ in range(n):
        k.ok(R, 1)
        fail = k.ok(R, 0)
    if extra:
        fail = k.ok(R, 1)
    return _plant("cas", k, not extra, fail, pair=n, extra=int(extra))


def cas_and_write(extra=False):
    """A write class and a CAS class 0 -> 1 of one value, two members each:
    four rounds of 1, a fifth fails."""
    k = _Key()
    _anchor(k)
    k.crashed(W, 1, count=2)
    k.crashed(C, 1, 0, count=2)
    fail = _rounds(k, 1, 4 + int(extra))
    return _plant("cas", k, not extra, fail, write=1, extra=int(extra))


def cas_expected(extra=False):
    """CAS classes 0 -> 1 and 2 -> 1, two members each: two rounds of 1 after
    a write of 0 and two after a write of 2 (extra: a third after 0 fails)."""
    k = _Key()
    _anchor(k)
    k.crashed(C, 1, 0, count=2)
    k.crashed(C, 1, 2, count=2)
    _rounds(k, 1, 2, w=0)
    fail = _rounds(k, 1, 2, w=2)
    if extra:
        fail = _rounds(k, 1, 1, w=0)
    return _plant("cas", k, not extra, fail, expected=1, extra=int(extra))


def single_several(good=True):
    """A read of 1 with one crashed write of 1 called: the lone configuration
    takes it (count 1, no branch).  Two more are called and a round of 1
    branches from that configuration; a second round leaves one
    configuration again, count 3.  A third round then needs a fourth member:
    called before it (good) or after it, as the key's last record."""
    k = _Key()
    _anchor(k)
    k.crashed(W, 1)
    k.ok(R, 1)
    k.crashed(W, 1, count=2)
    _rounds(k, 1, 2)
    if good:
        k.crashed(W, 1)
    fail = _rounds(k, 1, 1)
    if not good:
        k.crashed(W, 1)
    return _plant("single_several", k, good, fail, g=int(good))


# classes (a, b) of a two-class fan closed by a write and a read of 0, and
# what tests/test_planted_counted.py asserts of it: |R| or |W| of its large return
RUNG_R = (((127, 126), 16256), ((127, 127), 16384), ((127, 128), 16512))
RUNG_W = (((90, 90), 16381), ((75, 108), 16384), ((49, 165), 16385))
RUNG_CAP = 1 << 14


def rung(classes, closer="valid"):
    pl = fan(classes, closer=closer)
    return Plant("rung", _tag("rung", c=tuple(classes), closer=closer), pl.recs, pl.verdict,
                 pl.fail_op)


VALUE_IDS = (0, 14, 15, 16)


def values(extra=False):
    """Two crashed writes of each of the ids 0, 14, 15 and 16 (on both sides
    of the 16-entry legality table), two rounds of each behind writes of 7
    (extra: a third round of 16, which fails)."""
    k = _Key()
    _anchor(k)
    for v in VALUE_IDS:
        k.crashed(W, v, count=2)
    for v in VALUE_IDS:
        fail = _rounds(k, v, 2, w=7)
    if extra:
        fail = _rounds(k, 16, 1, w=7)
    return _plant("extremes", k, not extra, fail, ids=VALUE_IDS, extra=int(extra))


BAD_VERSIONS = (1 << 40, -7)


def far_version(extra=False):
    """A crashed write of 5 without a version, and two that carry versions no
    state reaches (2^40 and -7: one class once saturated, never legal).  One
    round of 5 is valid, a second fails."""
    k = _Key()
    _anchor(k)
    k.crashed(W, 5)
    for ver in BAD_VERSIONS:
        k.crashed(W, 5)
        k.recs[-1][3] = ver
    fail = _rounds(k, 5, 1 + int(extra))
    return _plant("extremes", k, not extra, fail, far_version=1, extra=int(extra))


def witness_unfit():
    """17 one-member CAS classes that are never legal and 48 [nil nil] reads
    open at once around a write and a read of 0: the search tiers give the
    reads no slot and decide the key, the witness stages count 65 ops open,
    and 17 classes fit no layout."""
    k = _Key()
    for i in range(17):
        k.crashed(C, 20 + i, 100 + i)
    rs = [k.call(R, N) for _ in range(48)]
    k.ok(W, 0)
    k.ok(R, 0)
    for i in rs:
        k.ret(i)
    return _plant("class_count", k, True, -1, witness_unfit=1)


GROUPS = ("small", "ladders", "rung")   # for lc_check and the witness stage
# "direct" and "noslot" are for lc_check_frontiers_counted alone: keys that do
# not overflow the slot tiers' window, and the one-slot layout with nothing
# else open — without an :ok op that constrains, lc_check decides that key
# before any search
ALL_GROUPS = GROUPS + ("direct", "noslot")


def interleave(plants):
    return tuple(_interleave(list(plants)))


@functools.lru_cache(maxsize=None)
def group(name):
    """The plants of one group, long and short keys alternating."""
    both = (False, True)
    if name == "small":
        out = [ladder(m, x) for m in LADDER_M if m < 127 for x in both]
        out += [neighbours(m, pos, tw) for m in NEIGHBOUR_M for pos in NEIGHBOUR_POS
                for tw in (None, "driven", "stepped")]
        out += [class_count(n, x) for n in CLASS_COUNTS for x in both]
        out += [slots(n) for n in (56, 57, 58)] + [slots(57, good=False), slot_reuse(),
                                                    slot_reuse(good=False)]
        out += [one_slot(n) for n in (1, 2)]
        out += [chunks(xs, lc, x) for xs, lc in CHUNK_LAYOUTS for x in both]
        out += [pending_ok(w, x) for w in PENDING_WHEN for x in both]
        out += [cas_pair(n, x) for n in (1, 2, 3, 4) for x in both]
        out += [f(x) for f in (cas_and_write, cas_expected, values, far_version) for x in both]
        out += [single_several(g) for g in (True, False)]
    elif name == "ladders":
        out = [ladder(m, x) for m in LADDER_M if m >= 127 for x in both]
        out += [nine_classes(last, x) for last in (127, 128) for x in both]
    elif name == "rung":
        out = [rung(c, closer) for c, _ in RUNG_R + RUNG_W for closer in ("valid", "read")]
    elif name == "direct":
        out = [ladder(m, x, anchor=False) for m in DIRECT_M for x in both]
        out += [class_count(16, x, anchor=False) for x in both]
        out += [class_count(17, False, anchor=False)]
    elif name == "noslot":
        out = [one_slot(0)]
    else:
        raise KeyError(name)
    return interleave(out)


# the family each mutant of counted_ref is aimed at
MUTANT_FAMILY = {"width_short": "ladder", "tuple_no_expected": "cas", "tuple_no_version": "extremes",
                 "no_pbit": "pending_ok", "called_at_start": "single_several",
                 "retire_fields": "single_several", "slots_plus_one": "slots"}
