"""Python restatement of the first witness stage (LC_FLAG_SEARCH_WITNESS,
csrc/witness_search.hip, ws_search): a depth-first search for a linearization
in which every open op holds one of 64 window slots, with the dead-end cache
modelled bucket for bucket.

TEST INFRASTRUCTURE ONLY.  It shares no code with the product; the model is
oracle.brute.step.  The order in which candidates are tried, the nodes that
are looked up, stored, spilled to a later bucket or not stored at all, and the
budget test are the device's, decision for decision, so the ranks, the number
of steps and the number of cache hits can be compared with what the device
reports, key for key.

search(records, cut, init, max_steps) -> Result:
  status   "found" | "none" (every order tried) | "budget" | "window"
  ranks    per record its rank, -1 = left out (None unless found)
  steps    ops linearized, retries included (the device's `nodes`)
  hits     nodes met again after they were found to be dead ends (`cache_hits`)
  stored   dead ends stored
  spilled  of those, the ones stored past the first bucket of their probe run
  dropped  dead ends that met 8 full buckets and were not stored
"""
import collections

from oracle import brute

INF = (1 << 63) - 1
R = brute.READ
NODE_CAP = 1 << 16  # kWitnessNodeCap
WINDOW = 64         # slots, one per open op
BUCKETS = 4096      # kWitnessBuckets
ENTRIES = 5         # nodes per bucket
PROBES = 8          # kWitnessProbes
M32, M64 = (1 << 32) - 1, (1 << 64) - 1

Result = collections.namedtuple("Result", "status ranks steps hits stored spilled dropped")
Events = collections.namedtuple("Events", "slots ev open_max")


def ws_hash(k, mask, ver, val):
    """The first bucket of node (k, mask, ver, val), before the modulus."""
    h = (mask * 0x9E3779B97F4A7C15) & M64
    h ^= ((((k & M32) << 32) | (ver & M32)) * 0xC2B2AE3D27D4EB4F) & M64
    h ^= ((val & M32) * 0x165667B19E3779F9) & M64
    h ^= h >> 29
    h = (h * 0xBF58476D1CE4E5B9) & M64
    return h >> 32


class Cache:
    """One key's dead ends: a node goes into the first of its 8 probed buckets
    with a free entry, nothing is removed, a lookup stops at the first bucket
    with a free entry."""

    def __init__(self):
        self.buckets = {}  # bucket number -> the nodes in it, in order of arrival
        self.stored = self.spilled = self.dropped = 0

    def _probe(self, node, insert):
        b0 = ws_hash(*node)
        for probe in range(PROBES):
            b = (b0 + probe) & (BUCKETS - 1)
            entries = self.buckets.get(b, ())
            if node in entries:
                return True
            if len(entries) < ENTRIES:
                if insert:
                    self.buckets.setdefault(b, []).append(node)
                    self.stored += 1
                    self.spilled += probe > 0
                return False
        self.dropped += insert
        return False

    def lookup(self, node):
        return self._probe(node, False)

    def insert(self, node):
        """Store the node unless it is there (True) or its 8 buckets are full."""
        return self._probe(node, True)


def events(records, cut=None):
    """The event pass: returns before calls at equal indices, up to the cut.
    Events(slot per record (None: not called by the cut), per return (record,
    records called before it, slot), most ops open at once) — slots is None
    when a 65th op opens (open_max = 65)."""
    recs = [tuple(int(x) for x in r) for r in records]
    n = len(recs)
    if cut is None:
        cut = INF - 1
    slots, ev, opened, open_max = [None] * n, [], {}, 0
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
        if len(opened) == WINDOW:
            return Events(None, None, WINDOW + 1)
        s = min(s for s in range(WINDOW) if s not in opened)
        slots[i] = s
        opened[s] = i
        open_max = max(open_max, len(opened))
        i += 1
    return Events(slots, ev, open_max)


def search(records, cut=None, init=(0, -1), max_steps=NODE_CAP):
    recs = [tuple(int(x) for x in r) for r in records]
    n = len(recs)
    slots, ev, _ = events(recs, cut)
    if slots is None:
        return Result("window", None, 0, 0, 0, 0, 0)
    K = len(ev)
    if K == 0:
        return Result("found", [-1] * n, 0, 0, 0, 0, 0)

    # per return k: slot -> record open at it (called before it, not returned)
    wins, win, c0 = [], {}, 0
    for x, ncalls, s in ev:
        for r in range(c0, ncalls):
            win[slots[r]] = r
        c0 = ncalls
        wins.append(dict(win))
        del win[s]

    def candidates(k, mask, state):
        cand = 0
        for s, r in wins[k].items():
            if not (mask >> s) & 1 and brute.step(state, recs[r]) is not None:
                cand |= 1 << s
        return cand

    def lowest(bits):
        return (bits & -bits).bit_length() - 1

    def pick(cs, k):
        """x's slot if it is a candidate, else the earliest return (crashed
        ops last), ties by slot."""
        es = ev[k][2]
        if (cs >> es) & 1:
            return es
        win = wins[k]
        return min((s for s in win if (cs >> s) & 1), key=lambda s: (recs[win[s]][5], s))

    budget = min(max_steps, NODE_CAP)
    iter_limit = 16 * budget + 4 * n + 1024
    k, mask, state = 0, 0, tuple(init)
    frames, cache = [], Cache()
    steps = hits = iters = n_ins = 0

    def result(status, ranks=None):
        return Result(status, ranks, steps, hits, cache.stored, cache.spilled, cache.dropped)

    while k < K:
        iters += 1
        if iters > iter_limit or steps > budget:
            return result("budget")
        es = ev[k][2]
        if (mask >> es) & 1:  # x is linearized: its return
            mask &= ~(1 << es)
            k += 1
            continue
        cand = 0
        if n_ins > 0 and cache.lookup((k, mask) + state):
            hits += 1
        else:
            cand = candidates(k, mask, state)
            if not cand:
                cache.insert((k, mask) + state)
                n_ins += 1
        if cand:
            win = wins[k]
            reads = 0
            for s, r in win.items():
                if (cand >> s) & 1 and recs[r][0] == R:
                    reads |= 1 << s
            if reads:  # a legal read goes first, and is forced
                s, rem = (es if (reads >> es) & 1 else lowest(reads)), 0
            else:
                s = pick(cand, k)
                rem = cand & ~(1 << s)
            frames.append(None)
        else:  # dead end: back to the last frame with a candidate left
            while True:
                if not frames:
                    return result("none")
                _, k, rem, mask, state = frames[-1]
                if rem:
                    break
                cache.insert((k, mask) + state)
                n_ins += 1
                frames.pop()
                iters += 1
                if iters > iter_limit:
                    return result("budget")
            s = pick(rem, k)
            rem &= ~(1 << s)
        rec = wins[k][s]
        frames[-1] = (rec, k, rem, mask, state)
        state = brute.step(state, recs[rec])
        assert state is not None
        mask |= 1 << s
        steps += 1
    ranks = [-1] * n
    for j, f in enumerate(frames):
        ranks[f[0]] = j
    return result("found", ranks)
