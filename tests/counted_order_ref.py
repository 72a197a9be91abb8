"""Python restatement of the counted witness search (LC_FLAG_COUNTED_WITNESS,
csrc/witness_counted.hip): a depth-first search for a linearization in which
the crashed writes/CAS hold no window slot but are counted per class.

TEST INFRASTRUCTURE ONLY.  It shares no code with the product; the model is
oracle.brute.step.  The order in which candidates are tried is the device's,
decision for decision, so the number of steps, of cache hits and of dead ends
stored can be compared with what the device reports.

Layout (include/lincheck.h, lc_counted_plan): classes are the distinct
(f, value, expected, version) among the crashed writes/CAS of the whole key,
in order of first call; class c with m members owns a count field of
m.bit_length() bits, packed from bit 63 downward, and lane 63 - c; the low
`slots` = min(64 - bits, 64 - classes) bits and lanes are window slots.

search(records, cut, init) -> Result(status, ranks, steps, hits, stored):
  status  "found" | "none" (every order tried) | "budget" | "unfit"
  ranks   per record its rank, -1 = left out (None unless found)
  steps   ops linearized, retries included (the device's `nodes`)
  hits    nodes met again after they were found to be dead ends
  stored  dead ends stored
"""
import collections

from oracle import brute

INF = (1 << 63) - 1
R, W, C = brute.READ, brute.WRITE, brute.CAS
NODE_CAP = 1 << 16  # kWitnessNodeCap

Result = collections.namedtuple("Result", "status ranks steps hits stored")


def _version(v):
    return 0x7FFFFFFE if (v < -1 or v > 0x7FFFFFFE) else v


def _tuple(r):
    return (r[0], r[1], r[2], _version(r[3]))


def layout(recs):
    """(class tuple -> index, shifts, widths, slots, fits)."""
    members = {}
    for r in recs:
        if r[0] in (W, C) and r[5] == INF:
            members[_tuple(r)] = members.get(_tuple(r), 0) + 1
    index, shifts, widths, bits = {}, [], [], 0
    for c, (t, m) in enumerate(members.items()):
        index[t] = c
        widths.append(m.bit_length())
        bits += widths[-1]
        shifts.append(64 - bits)
    slots = min(64 - bits, 64 - len(index))
    return index, shifts, widths, slots, len(index) <= 16 and slots >= 1


def search(records, cut=None, init=(0, -1), max_steps=NODE_CAP):
    recs = [tuple(int(x) for x in r) for r in records]
    n = len(recs)
    if cut is None:
        cut = INF - 1
    cls_of, shifts, widths, slots, fits = layout(recs)
    if not fits:
        return Result("unfit", None, 0, 0, 0)
    ncls = len(shifts)

    # ---- 1. event pass: returns before calls at equal indices, up to the cut
    where = [None] * n              # ("s", slot) | ("c", class) | None
    mem = [[] for _ in range(ncls)]  # per class its members, in call order
    ev = []                          # per return: (record, records called before it, slot)
    opened = {}                      # slot -> record
    i = 0
    while True:
        ncall = recs[i][4] if i < n else INF
        mret = min((recs[r][5] for r in opened.values()), default=INF)
        t = min(ncall, mret)
        if t == INF or t > cut:
            break
        if mret <= ncall:
            s = min(s for s, r in opened.items() if recs[r][5] == mret)
            ev.append((opened.pop(s), i, s))
            continue
        r = recs[i]
        if r[5] == INF:
            if r[0] in (W, C):
                c = cls_of[_tuple(r)]
                where[i] = ("c", c)
                mem[c].append(i)
        else:
            free = [s for s in range(slots) if s not in opened]
            if not free:
                return Result("unfit", None, 0, 0, 0)
            where[i] = ("s", free[0])
            opened[free[0]] = i
        i += 1
    K = len(ev)
    if K == 0:
        return Result("found", [-1] * n, 0, 0, 0)

    wins, ncalled = [], []  # per return k: slot -> record open at it; members called, per class
    win, cnt, c0 = {}, [0] * ncls, 0
    for k, (x, ncalls, _) in enumerate(ev):
        for r in range(c0, ncalls):
            if where[r] and where[r][0] == "s":
                win[where[r][1]] = r
            elif where[r]:
                cnt[where[r][1]] += 1
        c0 = ncalls
        wins.append(dict(win))
        ncalled.append(list(cnt))
        del win[where[x][1]]

    def window(k):
        """slot -> record at return k: called before it, not yet returned."""
        return wins[k]

    def called(k, c):
        return ncalled[k][c]

    def field(mask, c):
        return (mask >> shifts[c]) & ((1 << widths[c]) - 1)

    def candidates(k, mask, state):
        win = window(k)
        cand = {s for s, r in win.items()
                if not (mask >> s) & 1 and brute.step(state, recs[r]) is not None}
        pending = {_tuple(recs[r]) for s, r in win.items() if not (mask >> s) & 1}
        for t, c in cls_of.items():
            if field(mask, c) < called(k, c) and t not in pending and \
                    brute.step(state, t + (0, INF)) is not None:
                cand.add(63 - c)
        return cand

    def pick(cs, k):
        es = ev[k][2]
        if es in cs:
            return es
        win = window(k)
        return min(cs, key=lambda s: (recs[win[s]][5] if s < slots else INF, s))

    # ---- 2. search
    budget = min(max_steps, NODE_CAP)
    iter_limit = 16 * budget + 4 * n + 1024
    k, mask, state = 0, 0, tuple(init)
    frames, dead = [], set()
    steps = hits = iters = 0
    while k < K:
        iters += 1
        if iters > iter_limit or steps > budget:
            return Result("budget", None, steps, hits, len(dead))
        es = ev[k][2]
        if (mask >> es) & 1:  # x is linearized: its return
            mask &= ~(1 << es)
            k += 1
            continue
        cand = set()
        if dead and (k, mask, state) in dead:
            hits += 1
        else:
            cand = candidates(k, mask, state)
            if not cand:
                dead.add((k, mask, state))
        if cand:
            win = window(k)
            reads = {s for s in cand if s < slots and recs[win[s]][0] == R}
            if reads:  # a legal read goes first, and is forced
                s, rem = (es if es in reads else min(reads)), set()
            else:
                s = pick(cand, k)
                rem = cand - {s}
            frames.append(None)
        else:  # dead end: back to the last frame with a candidate left
            while True:
                if not frames:
                    return Result("none", None, steps, hits, len(dead))
                _, k, rem, mask, state = frames[-1]
                if rem:
                    break
                dead.add((k, mask, state))
                frames.pop()
                iters += 1
                if iters > iter_limit:
                    return Result("budget", None, steps, hits, len(dead))
            s = pick(rem, k)
            rem = rem - {s}
        if s < slots:
            rec = window(k)[s]
            nmask = mask | 1 << s
        else:
            c = 63 - s
            rec = mem[c][field(mask, c)]
            nmask = mask + (1 << shifts[c])
        frames[-1] = (rec, k, rem, mask, state)
        state = brute.step(state, recs[rec])
        assert state is not None
        mask = nmask
        steps += 1
    ranks = [-1] * n
    for j, f in enumerate(frames):
        ranks[f[0]] = j
    return Result("found", ranks, steps, hits, len(dead))
