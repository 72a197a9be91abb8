"""A literal Python restatement of the counted-class search (DESIGN.md §4,
`counted_tier_kernel` and `counted_frontier_kernel`; the layout rule of
csrc/counted.h).  TEST INFRASTRUCTURE ONLY.  It shares no code with oracle.c,
search_ref.py or counted_order_ref.py.

    layout   classes = the distinct (f, value, expected, version) among the
             key's crashed writes/CAS, in order of first call; class c with m
             members owns a field of floor(log2 m) + 1 bits, fields packed
             from bit 63 down; slots = 64 - field bits; the key fits with at
             most 16 classes and at least one slot.
    word     a configuration is (64-bit word, (version, value)); the word is
             a Python int masked to 64 bits — count fields on top, one-bit
             window slots below (bit s set: the op in slot s is linearized).
    call     of a crashed write/CAS: its class's `called` goes up.  Of any
             other op that constrains (not a crashed or [nil nil] read, not a
             read legal in a lone configuration): the lowest free slot; none
             free: the key stops (LC_REASON_WINDOW_OVERFLOW).  A read is
             linearized at once wherever it is legal.
    return   of the op in slot s: R = the configurations with bit s, W the
             others; every configuration of W is expanded once.  Candidates:
             a pending slot mutation that is legal and has no pending member
             of its tuple with an earlier deadline (return, then call) in a
             slot; class c when legal, field_c < called_c and no pending :ok
             member of the tuple in a slot.  Successor: word | bit, or word +
             (1 << shift_c); then every pending read legal in the new state.
             F = R without bit s; empty: invalid at this op.  Slot bits set
             in every configuration of F are retired (AND over slot bits
             only: count fields stay).  A lone configuration is walked as a
             chain while it has one candidate; at two it takes the general
             path from the configuration the return was entered with.

configs_explored counts the initial configuration and every successor
generated, duplicates included; max_frontier is the largest F after a return.

`mutant=` changes one line of the rule (MUTANTS); the suite must tell each
from the true rule on some plant.  Nothing on the device is ever mutated."""
from collections import namedtuple

INF = (1 << 63) - 1
R, W, C, N = 0, 1, 2, -1
M64 = (1 << 64) - 1
MAX_CLASSES = 16
VALID, INVALID, UNKNOWN = 1, 0, -1
REASON_NONE, REASON_NONLINEARIZABLE, REASON_CONFIG_BUDGET, REASON_WINDOW_OVERFLOW = 0, 1, 2, 3

MUTANTS = ("width_short", "tuple_no_expected", "tuple_no_version", "no_pbit", "called_at_start",
           "retire_fields", "slots_plus_one")

Result = namedtuple("Result", "verdict reason fail_op fail_prefix_end configs_explored "
                              "max_frontier layout slots_used_max returns frontier window64 "
                              "return_ops noops")
SIX = Result._fields[:6]


def version_of(v):
    """A version as the device reads it: one no state reaches is saturated."""
    return 0x7FFFFFFE if (v < -1 or v > 0x7FFFFFFE) else v


def class_key(rec, mutant=None):
    f, value, expected, version = rec[0], rec[1], rec[2], version_of(rec[3])
    if mutant == "tuple_no_expected":
        expected = None
    if mutant == "tuple_no_version":
        version = None
    return (f, value, expected, version)


def width_of(m, mutant=None):
    if mutant == "width_short":
        return (m - 1).bit_length()  # ceil(log2 m)
    return m.bit_length()            # floor(log2 m) + 1


def layout(recs, mutant=None):
    """The layout as abi.counted_plan reports it, and per class its member
    records in call order (under "members_of", beside the plan's fields)."""
    members = {}  # first call first: records are sorted by call
    for i, r in enumerate(recs):
        if r[0] in (W, C) and r[5] == INF:
            members.setdefault(class_key(r, mutant), []).append(i)
    classes, bits = [], 0
    for idx in members.values():
        first = recs[idx[0]]
        w = width_of(len(idx), mutant)
        bits += w
        classes.append({"f": first[0], "value": first[1], "expected": first[2],
                        "version": version_of(first[3]), "members": len(idx), "shift": 64 - bits,
                        "width": w})
    # counted.h, counted_slots: min(64 - field bits, 64 - classes).  Every
    # width is at least 1, so the first term is the smaller one and the rule
    # is "64 - field bits"; the second keeps class lanes and slot lanes apart
    slots = min(64 - bits, 64 - len(classes))
    fits = int(len(classes) <= MAX_CLASSES and slots >= 1)
    if mutant == "slots_plus_one":
        slots += 1
    return {"n_classes": len(classes), "field_bits": bits, "slots": slots, "fits": fits,
            "classes": classes[:MAX_CLASSES]}, list(members.values())


def plan(recs):
    """What abi.counted_plan returns for these records."""
    return layout(recs)[0]


def _legal(rec, ver, val):
    f, value, expected, version = rec[0], rec[1], rec[2], version_of(rec[3])
    if f == R:
        return (version == N or version == ver) and (value == N or value == val)
    if version != N and version != ver + 1:
        return False
    return f == W or val == expected


def check(recs, init=(0, N), stop=None, mutant=None, budget=1 << 22):
    """The counted search of one key (records sorted by call).  With stop=i
    the search ends at record i's :ok return and Result.frontier is the
    frontier that return would expand, as a list of (version, value, sorted
    pending record indices) — [] when that return is a no-op, None when the
    search cannot get there (as the device's -1).  More than `budget`
    configurations: :unknown, LC_REASON_CONFIG_BUDGET (a mutant may never end)."""
    assert mutant is None or mutant in MUTANTS, mutant
    lay, members_of = layout(recs, mutant)

    def result(verdict, reason, fail=-1, end=-1, frontier=None):
        return Result(verdict, reason, fail, end, explored, max_frontier, lay, slots_used_max,
                      returns, frontier, window64, return_ops, noops)

    explored = max_frontier = 1
    slots_used_max = 0
    returns, window64 = [], False
    return_ops, noops = [], []  # the general-path returns' records; :ok records whose return found no slot
    if not lay["fits"]:
        return result(UNKNOWN, REASON_WINDOW_OVERFLOW)
    if stop is not None and not (0 <= stop < len(recs) and recs[stop][5] != INF):
        return result(VALID, REASON_NONE)  # (frontier None: not an :ok op)

    n_slots = lay["slots"]
    ncls = lay["n_classes"]
    shift = [c["shift"] for c in lay["classes"]]
    wmask = [(1 << c["width"]) - 1 for c in lay["classes"]]
    slotbits = (1 << n_slots) - 1
    rep = [recs[idx[0]] for idx in members_of]          # the class lane's precondition and effect
    cls_of = {class_key(recs[idx[0]], mutant): c for c, idx in enumerate(members_of)}
    called = [len(idx) if mutant == "called_at_start" else 0 for idx in members_of]
    slot_rec = [None] * n_slots                         # slot -> record
    before = [0] * n_slots                              # slot -> slots that go first (its tuple, earlier deadline)
    cls_before = [0] * ncls                             # class -> slots of pending :ok members of its tuple
    occ = rdm = 0
    single = True
    frontier = [(0, tuple(init))]                       # single: the lone (counts, state)

    def field(word, c):
        return (word >> shift[c]) & wmask[c]

    def reads_legal(ver, val):
        out = 0
        for s in range(n_slots if rdm else 0):
            if (rdm >> s) & 1 and _legal(recs[slot_rec[s]], ver, val):
                out |= 1 << s
        return out

    def successors(word, ver, val):
        """[(word, state)] of every candidate of (word, (ver, val)), read
        closure applied."""
        out = []
        pending = occ & ~rdm & ~word & slotbits
        for s in range(n_slots if pending else 0):
            if (pending >> s) & 1 \
                    and before[s] & ~word == 0 and _legal(recs[slot_rec[s]], ver, val):
                out.append((word | (1 << s), recs[slot_rec[s]][1]))
        for c in range(ncls):
            if field(word, c) < called[c] and _legal(rep[c], ver, val) \
                    and (mutant == "no_pbit" or cls_before[c] & ~word == 0):
                out.append(((word + (1 << shift[c])) & M64, rep[c][1]))
        return [(w | reads_legal(ver + 1, v), (ver + 1, v)) for w, v in out]

    def retire(bits):
        nonlocal occ, rdm
        occ &= ~bits
        rdm &= ~bits
        for s in range(n_slots):
            if (bits >> s) & 1:
                slot_rec[s] = None
            before[s] &= ~bits
        for c in range(ncls):
            cls_before[c] &= ~bits

    def open64():
        """Ops a slot-per-op search holds open now: the slots, and every
        called member no slot-per-op configuration set could have retired."""
        least = [min(field(w, c) for w, _ in frontier) for c in range(ncls)]
        return bin(occ).count("1") + sum(called_now[c] - least[c] for c in range(ncls))

    called_now = [0] * ncls  # (called, but counted from the calls under every mutant)

    def dump():
        out = []
        for word, (ver, val) in frontier:
            pend = [slot_rec[s] for s in range(n_slots) if (occ >> s) & 1 and not (word >> s) & 1]
            for c in range(ncls):
                pend += members_of[c][field(word, c):called[c]]
            out.append((ver, val, tuple(sorted(pend))))
        return out

    events = []
    for i, r in enumerate(recs):
        events.append((r[4], 0, i))
        if r[5] != INF:
            events.append((r[5], 1, i))
    events.sort()
    stop_ret = recs[stop][5] if stop is not None else None

    for t, is_ret, x in events:
        rec = recs[x]
        if stop is not None and t > stop_ret:
            return result(VALID, REASON_NONE, frontier=[])
        if not is_ret:
            # ------------------------------------------------------ call of x
            crashed = rec[5] == INF
            if rec[0] == R:
                if crashed or (rec[1] == N and rec[3] == N):
                    continue
                if single and _legal(rec, *frontier[0][1]):
                    continue
            if open64() == 64:
                window64 = True
            if crashed:
                c = cls_of[class_key(rec, mutant)]
                called_now[c] += 1
                if mutant != "called_at_start":
                    called[c] += 1
                continue
            if occ & slotbits == slotbits:
                return result(UNKNOWN, REASON_WINDOW_OVERFLOW)
            s = next(s for s in range(n_slots) if not (occ >> s) & 1)
            bs = 1 << s
            slot_rec[s] = x
            before[s] = 0
            occ |= bs
            slots_used_max = max(slots_used_max, bin(occ).count("1"))
            if rec[0] == R:
                rdm |= bs
                frontier = [(w | bs if _legal(rec, *st) else w, st) for w, st in frontier]
            else:
                key = class_key(rec, mutant)
                for q in range(n_slots):
                    if q != s and (occ >> q) & 1 and not (rdm >> q) & 1 \
                            and class_key(recs[slot_rec[q]], mutant) == key:
                        if recs[slot_rec[q]][5] <= rec[5]:
                            before[s] |= 1 << q
                        else:
                            before[q] |= bs
                if key in cls_of:
                    cls_before[cls_of[key]] |= bs
            continue

        # -------------------------------------------------------- return of x
        if x not in slot_rec:
            if x == stop:
                return result(VALID, REASON_NONE, frontier=[])
            noops.append(x)
            continue
        s = slot_rec.index(x)
        bs = 1 << s
        if x == stop:
            return result(VALID, REASON_NONE, frontier=dump())
        if single:
            word, st = frontier[0]
            e0, branch, empty = explored, False, False
            while True:
                succ = successors(word, *st)
                if not succ:
                    empty = True
                    break
                if len(succ) > 1:
                    branch = True
                    break
                explored += 1
                if explored > budget:
                    return result(UNKNOWN, REASON_CONFIG_BUDGET)
                word, st = succ[0]
                if word & bs:
                    break
            if branch:
                explored = e0
                single = False
            elif empty:
                return result(INVALID, REASON_NONLINEARIZABLE, x, rec[5])
            else:
                retire(word & slotbits)  # x included
                frontier = [(word & ~slotbits, st)]
        if not single:
            n_f = len(frontier)
            done = {(w & ~bs, st) for w, st in frontier if w & bs}
            work = [c for c in frontier if not c[0] & bs]
            seen = set(work)
            head = 0
            while head < len(work):
                word, st = work[head]
                head += 1
                for nw, nst in successors(word, *st):
                    explored += 1
                    if explored > budget:
                        return result(UNKNOWN, REASON_CONFIG_BUDGET)
                    if nw & bs:
                        done.add((nw & ~bs, nst))
                    elif (nw, nst) not in seen:
                        seen.add((nw, nst))
                        work.append((nw, nst))
            returns.append((n_f, len(work), len(done)))
            return_ops.append(x)
            frontier = sorted(done)
            max_frontier = max(max_frontier, len(frontier))
            if not frontier:
                return result(INVALID, REASON_NONLINEARIZABLE, x, rec[5])
            retire(bs)
            everywhere = M64
            for w, _ in frontier:
                everywhere &= w
            rb = everywhere if mutant == "retire_fields" else everywhere & occ
            if rb:
                retire(rb & slotbits)
                frontier = [(w & ~rb, st) for w, st in frontier]
            if len(frontier) == 1:
                single = True
                frontier = [(frontier[0][0] & ~slotbits, frontier[0][1])]
    return result(VALID, REASON_NONE, frontier=[] if stop is not None else None)


def sizes(res):
    """(largest max(|W|, |R|), largest |R| + |W|, largest |F| entering) over
    the general-path returns."""
    if not res.returns:
        return 0, 0, 0
    return (max(max(w, r) for _, w, r in res.returns), max(w + r for _, w, r in res.returns),
            max(f for f, _, _ in res.returns))
