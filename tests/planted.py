"""Deterministic keys with one planted violation each, placed where the
version-order decision (check_kernel.hip, fast_key) changes hands: between
the four positions of a thread, between lanes, between the 16-lane rows of
the DPP scan (64 positions), between waves (256 positions), at the last
positions below the count of placed mutations M and at the record counts
around the LDS clear's 4 * tid <= n guard.  No randomness.

Records are [f, value, expected, version, call, ret] as in helpers.py.  The
base key is a ladder: record s has call 4s and ret 4s + 1 (two spare event
slots per step for inserted ops), the j-th write has value j % 7 and version
j + 1, and with reads_every = r an :ok read of the current version and value
follows every r-th write.  "Position" p is the p-th mutation (version p + 1);
in an all-writes ladder it is also the record index, in an interleaved one the
two fall on different thread / row / wave boundaries.

Every builder returns a Plant: the records, the expected verdict (1 valid,
0 invalid) and the expected canonical fail op (the :ok record whose return
first makes the prefix non-linearizable; -1 for a valid key).  Each invalid
plant has a valid twin: the same builder with good=True (one field differs),
or the plain ladder for swap / hole / dup.  tests/test_planted.py pins every
verdict and fail op against the CPU oracle's searches."""
import functools
from collections import namedtuple

from helpers import INF, C, N, R, W

Plant = namedtuple("Plant", "family tag recs verdict fail_op")

# positions on either side of every ownership boundary of timing_fails
# (thread 4, row 64, wave 256) and of first_failure's / fast_gap's wave scans;
# 383 / 384 and 447 / 448: the row totals merged in a wave that also has `pre`
POSITIONS = (0, 1, 2, 3, 4, 15, 16, 62, 63, 64, 65, 127, 128, 191, 192, 254, 255, 256, 257,
             383, 384, 447, 448, 511, 512, 767, 768)
# record counts around the thread, row and wave sizes and the tier's 1,024
LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1020, 1021, 1022, 1023, 1024)
# past the version-order tier: the gap tier proper decides (gap_tier.hip)
LONG_LENGTHS = (1025, 3001)
# gap_tier.hip: record chunks of T = 256 / 512 threads, kSetupBatch = 4 chunks
# kept in registers (1,024 / 2,048 records), and a suffix-minimum scan in
# which thread t owns ceil(M / T) consecutive positions, so its wave
# boundaries fall at multiples of 64 * ceil(M / T): 320 for M = 1,025 and 256
# for the interleaved ladder's M = 769; 768 (T = 256) and 384 (T = 512) for
# M = 3,001, 576 and 320 for the interleaved M = 2,251
LONG_POSITIONS = {
    1025: (0, 3, 4, 63, 64, 255, 256, 319, 320, 511, 512, 639, 640, 767, 768, 959, 960, 1023),
    3001: (0, 319, 320, 383, 384, 575, 576, 767, 768, 1023, 1024, 2047, 2048),
}
FAR_D = (2, 20)


def val(p):
    """The value the ladder's write at position p leaves."""
    return p % 7


def _wrong(v):
    return 3 if v == N else (v + 1) % 7


@functools.lru_cache(maxsize=None)
def _ladder(n, reads_every=0, t0=0, far=None):
    """(records, held): held[p] = record index of the write at position p.
    The records are shared between keys: builders replace, never mutate.
    far = (p, d, late): the writes at positions p .. p+d laid out as far()
    describes, when they fit."""
    recs, held = [], []
    while len(recs) < n:
        s, p = len(recs), len(held)
        t = t0 + 4 * s
        if far and p == far[0] and s + far[1] + 1 <= n:
            d = far[1]
            for j in range(1, d):  # holders of p+1 .. p+d-1: called first, left open
                recs.append([W, val(p + j), N, p + j + 1, t + j - 1, t + d + 3 + j])
            # the holder of p+d returns at t+d (before the holder of p is
            # called: only A[p] > B[p+d] fails) or at t+d+2 (after: valid)
            recs.append([W, val(p + d), N, p + d + 1, t + d - 1, t + d if far[2] else t + d + 2])
            recs.append([W, val(p), N, p + 1, t + d + 1, t + d + 3])
            held.append(s + d)
            held.extend(range(s, s + d))
            continue
        recs.append([W, val(p), N, p + 1, t, t + 1])
        held.append(s)
        if reads_every and (p + 1) % reads_every == 0 and len(recs) < n:
            t = t0 + 4 * len(recs)
            recs.append([R, val(p), N, p + 1, t, t + 1])
    return tuple(recs), tuple(held)


def ladder(n, reads_every=0):
    """The base key: n records, valid."""
    return [list(r) for r in _ladder(n, reads_every)[0]]


def n_positions(n, reads_every=0):
    """M of the n-record ladder."""
    return len(_ladder(n, reads_every)[1])


def _tag(family, n, re, **kw):
    return "%s n=%d re=%d %s" % (family, n, re, " ".join("%s=%s" % i for i in sorted(kw.items())))


def base(n, re=0):
    return Plant("base", _tag("base", n, re), list(_ladder(n, re)[0]), 1, -1)


def swap(n, re, p):
    """Versions of the writes at positions p, p+1 exchanged: the holder of
    p+1 returns before the holder of p is called."""
    b, held = _ladder(n, re)
    recs = list(b)
    i, j = held[p], held[p + 1]
    recs[i] = b[i][:3] + [p + 2] + b[i][4:]
    recs[j] = b[j][:3] + [p + 1] + b[j][4:]
    return Plant("swap", _tag("swap", n, re, p=p), recs, 0, i)


def far(n, re, p, d, good=False):
    """Holders of positions p+1 .. p+d-1 called first and left open, then the
    holder of p+d called and returned, then the holder of p, then the open
    ones return.  Fails at the return of the holder of p+d."""
    b, held = _ladder.__wrapped__(n, re, 0, (p, d, not good))  # (not cached: one key each)
    assert held[p] > held[p + d], "the segment does not fit"
    return Plant("far", _tag("far", n, re, p=p, d=d, good=int(good)), list(b),
                 1 if good else 0, -1 if good else held[p + d])


def hole(n, re, p):
    """Every version from position p on shifted up by one (reads too):
    nothing writes version p+1."""
    b, held = _ladder(n, re)
    recs = [r if r[3] < p + 1 else r[:3] + [r[3] + 1] + r[4:] for r in b]
    return Plant("hole", _tag("hole", n, re, p=p), recs, 0, held[p])


def dup(n, re, p):
    """The write at position p+1 claims version p+1 as well."""
    b, held = _ladder(n, re)
    recs = list(b)
    j = held[p + 1]
    recs[j] = b[j][:3] + [p + 1] + b[j][4:]
    return Plant("dup", _tag("dup", n, re, p=p), recs, 0, j)


def _insert(n, re, s, body):
    """An n-record key: the (n-1)-record ladder (one step later in time) with
    body = [f, value, expected, version] called and returned in the spare
    slots before record s.  Returns (records, writes before s, M)."""
    b, held = _ladder(n - 1, re, 4)
    recs = list(b)
    recs.insert(s, list(body) + [4 * s + 2, 4 * s + 3])
    return recs, sum(1 for h in held if h < s), len(held)


def read_past(n, re, s, k):
    """An :ok read [k nil] as record s.  Valid when k is the version current
    there; k = M + 1 and k = n are versions nothing writes."""
    recs, cur, m = _insert(n, re, s, [R, N, N, k])
    ok = k == cur
    return Plant("read_past", _tag("read_past", n, re, s=s, k=k), recs, int(ok), -1 if ok else s)


def read_val(n, re, s, good=False):
    """A read of the version current at record s (0 before the first write)
    with a value: the one there, or another."""
    b, held = _ladder(n - 1, re, 4)
    cur = sum(1 for h in held if h < s)
    v = val(cur - 1) if cur else N
    recs, _, _ = _insert(n, re, s, [R, v if good else _wrong(v), N, cur])
    return Plant("read_val", _tag("read_val", n, re, s=s, good=int(good)), recs,
                 int(good), -1 if good else s)


def cas_exp(n, re, p, good=False):
    """The write at position p as a CAS expecting the value before it, or
    another."""
    b, held = _ladder(n, re)
    recs = list(b)
    i = held[p]
    e = val(p - 1) if p else N
    recs[i] = [C, val(p), e if good else _wrong(e)] + b[i][3:]
    return Plant("cas_exp", _tag("cas_exp", n, re, p=p, good=int(good)), recs,
                 int(good), -1 if good else i)


def read_stale(n, re, p, d=1, good=False):
    """A read called after the write at position p+d returned that claims
    version p+1 (stale; valid twin: version p+d+1)."""
    held = _ladder(n - 1, re, 4)[1]
    s = held[p + d] + 1
    recs, cur, _ = _insert(n, re, s, [R, N, N, p + d + 1 if good else p + 1])
    assert cur == p + d + 1
    return Plant("read_stale", _tag("read_stale", n, re, p=p, d=d, good=int(good)), recs,
                 int(good), -1 if good else s)


def read_future(n, re, p, good=False):
    """A read that returned before the write at position p+1 was called and
    claims version p+2 (valid twin: version p+1)."""
    held = _ladder(n - 1, re, 4)[1]
    assert p + 1 < len(held)
    s = held[p] + 1
    recs, cur, _ = _insert(n, re, s, [R, N, N, p + 1 if good else p + 2])
    assert cur == p + 1
    return Plant("read_future", _tag("read_future", n, re, p=p, good=int(good)), recs,
                 int(good), -1 if good else s)


def crash(n, re, gaps, late=None):
    """The writes at positions `gaps` replaced by crashed version-less
    writes, each called where it was — except the one at `late`, called in
    the spare slot after the write at position late+1 returned: past its
    gap's deadline.  The record that followed it (a read of version late+1
    or the write at late+1) then needs a position nothing can fill."""
    b, held = _ladder(n, re)
    recs = list(b)
    for g in gaps:
        i = held[g]
        recs[i] = [W, val(g), N, N, b[i][4], INF]
    fail = -1
    if late is not None:
        assert late in gaps and late + 1 not in gaps
        i, j = held[late], held[late + 1]
        op = recs.pop(i)
        recs.insert(j, op[:4] + [b[j][5] + 1, INF])  # (j: after the write, one index down)
        fail = i
    return Plant("crash", _tag("crash", n, re, gaps="+".join(map(str, gaps)), late=late), recs,
                 0 if late is not None else 1, fail)


FAMILIES = ("swap", "far", "hole", "dup", "read_past", "read_val", "cas_exp", "read_stale",
            "read_future", "crash")


def _at(family, n, re, p):
    """The family's plants (invalid ones and their twins) at position p of
    the n-record ladder; nothing where p does not exist for it."""
    m = n_positions(n, re)
    m1 = n_positions(n - 1, re) if n > 1 else 0  # builders that insert a record
    out = []
    if family == "swap" and p + 1 < m:
        out.append(swap(n, re, p))
    elif family == "far":
        # p as the late holder's position and as the early returner's (p0 + d)
        for d, p0 in [(d, q) for d in FAR_D for q in (p, p - d)]:
            if p0 >= 0 and p0 + d < m:
                try:
                    out += [far(n, re, p0, d), far(n, re, p0, d, good=True)]
                except AssertionError:  # the segment runs past the key's end
                    pass
    elif family == "hole" and p < m:
        out.append(hole(n, re, p))
    elif family == "dup" and p + 1 < m:
        out.append(dup(n, re, p))
    elif family == "read_past" and p < n:
        # record p is the read; the versions nothing writes, and the current one
        _, cur, mm = _insert(n, re, p, [R, N, N, 0])
        for k in sorted({mm + 1, n, cur}):
            out.append(read_past(n, re, p, k))
    elif family == "read_val" and p < n:
        out += [read_val(n, re, p), read_val(n, re, p, good=True)]
    elif family == "cas_exp" and p < m:
        out += [cas_exp(n, re, p), cas_exp(n, re, p, good=True)]
    elif family == "read_stale":
        for d in (1, 5):
            if p + d < m1:
                out += [read_stale(n, re, p, d), read_stale(n, re, p, d, good=True)]
    elif family == "read_future" and p + 1 < m1:
        out += [read_future(n, re, p), read_future(n, re, p, good=True)]
    elif family == "crash" and p + 1 < m:
        out += [crash(n, re, (p,), late=p), crash(n, re, (p,))]
    return out


def _positions(n, re, wanted):
    m = n_positions(n, re)
    return sorted({p for p in wanted if p < max(m, n)} | {max(m - 2, 0), max(m - 1, 0)})


@functools.lru_cache(maxsize=None)
def family_plants(family):
    """Every plant of one family the version-order tier sees (n <= 1,024):
    all POSITIONS on the 1,024-write ladder and on the 1,023-record ladder
    with a read after every third write, and for every length of LENGTHS
    (both ladders) the last two positions."""
    out, seen = [], set()

    def add(plants):
        for pl in plants:
            if pl.tag not in seen:
                seen.add(pl.tag)
                out.append(pl)

    for n, re in ((1024, 0), (1023, 3)):
        for p in _positions(n, re, POSITIONS):
            add(_at(family, n, re, p))
    for n in LENGTHS:
        for re in (0, 3):
            last = {n_positions(n, re) - 2, n_positions(n, re) - 1, n - 2, n - 1}
            for p in sorted(q for q in last if q >= 0):
                add(_at(family, n, re, p))
    if family == "crash":
        # several gaps in one key, in different threads, rows and waves: the
        # gap tables are compacted across waves (fg_prefix_wave) and each
        # gap's deadline is a suffix minimum across them
        for n, re in ((1024, 0), (1023, 3)):
            m = n_positions(n, re)
            gs = tuple(g for g in (0, 3, 63, 64, 255, 256, 511, 700, 767, 1000) if g + 1 < m)
            add([crash(n, re, gs)] + [crash(n, re, gs, late=g) for g in gs if g + 1 not in gs])
    return tuple(out)


@functools.lru_cache(maxsize=None)
def base_plants():
    """The valid ladders of every length (both kinds)."""
    return tuple(base(n, re) for n in LENGTHS for re in (0, 3))


@functools.lru_cache(maxsize=None)
def long_plants(n):
    """The same plants on keys past the version-order tier's 1,024 records
    (n of LONG_LENGTHS): the gap tier proper decides them, crash-free or not.
    Every family on the all-writes ladder just past the tier; fewer on the
    3,001-record keys and the interleaved ladders (the keys are long), and
    one far / stale distance."""
    out, seen = [], set()
    for re in (0, 3):
        out.append(base(n, re))
        if n == LONG_LENGTHS[0]:
            fams = FAMILIES if re == 0 else ("swap", "far", "read_val", "crash")
        else:
            fams = ("swap", "far", "read_val", "crash") if re == 0 else ("swap", "crash")
        for p in _positions(n, re, LONG_POSITIONS[n]):
            for family in fams:
                for pl in _at(family, n, re, p):
                    if pl.tag not in seen and " d=2 " not in pl.tag and " d=5 " not in pl.tag:
                        seen.add(pl.tag)
                        out.append(pl)
    return tuple(out)


def interleave(plants):
    """Long and short keys alternating (longest, shortest, second longest,
    ...): a workgroup that decides a 5-record key after a 1,024-record one
    meets the longer key's tables beyond its own n, and the other way round."""
    by_len = sorted(plants, key=lambda pl: (-len(pl.recs), pl.tag))
    out = []
    lo, hi = 0, len(by_len) - 1
    while lo <= hi:
        out.append(by_len[lo])
        if lo != hi:
            out.append(by_len[hi])
        lo, hi = lo + 1, hi - 1
    return out
