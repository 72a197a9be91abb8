"""A plain Python statement of the frontier search the GPU's search tiers run
(lds_tier_kernel, hbm_tier_kernel, hbm_coop_kernel), written from DESIGN.md §4
("lds_tier_kernel — JIT search") and the header of check_kernel.hip: Lowe's
just-in-time linearization with the four exact reductions.  It shares no code
with oracle.c and keeps no slots or bit rows: a configuration is (the set of
open ops linearized in it, (version, value)), the open ops are a dict.

    frontier F = {(no op linearized, initial state)}
    call of x:   x becomes open — unless it is a read that never constrains
                 (crashed, or [nil nil]), or F is one configuration and x is
                 a read legal in it (linearized and retired at once).
                 A read is linearized at once in every configuration where
                 it is legal (eager read closure).
    return of x: (nothing if x is not open)
                 R = the configurations that linearized x, W = the others;
                 every configuration of W is expanded once: each pending
                 mutation that is legal there and has the earliest deadline
                 (return, then call; a crashed op never returns) among the
                 pending members of its class (f, value, expected, version)
                 gives a successor, closed under legal pending reads; a
                 successor that linearized x joins R, another one W.
                 F = R without x; empty: the key is invalid at x.
                 Ops linearized in every configuration of F are retired.

configs_explored counts the initial configuration and every successor
generated, duplicates included; max_frontier is the largest F after a return
(1 at the start).  Both are the definitions of include/lincheck.h, which the
oracle shares (tests/test_planted_search.py compares all five fields).

What the oracle does not report and the capacity edges depend on:
  returns    per return on the GENERAL path (F holds several configurations,
             or the lone configuration has two candidates somewhere on its
             walk to x), the triple (|F| before, |W| visited, |R| result);
  slots_max  the most ops open at once (the window holds 64; `overflow` is
             set when a call found 64 open, where the device stops with
             LC_REASON_WINDOW_OVERFLOW — the search here goes on)."""
from collections import namedtuple

from helpers import INF, N, R, W

Result = namedtuple("Result", "verdict fail_op fail_prefix_end configs_explored max_frontier "
                              "returns slots_max overflow")
WINDOW = 64


def _legal(rec, ver, val):
    f, value, expected, version = rec[0], rec[1], rec[2], rec[3]
    if f == R:
        return (version == N or version == ver) and (value == N or value == val)
    if version != N and version != ver + 1:
        return False
    return f == W or val == expected


def _deadline(rec):
    return (rec[5], rec[4])


def check(recs, init_version=0, init_value=N):
    """Result of one key (records sorted by call, as helpers.py makes them)."""
    events = []
    for i, r in enumerate(recs):
        events.append((r[4], 0, i))
        if r[5] != INF:
            events.append((r[5], 1, i))
    events.sort()

    frontier = {(0, (init_version, init_value))}  # (bit i: op i linearized, state)
    open_reads = {}   # op -> record
    classes = {}      # (f, value, expected, version) -> open mutations, earliest deadline first
    n_open = slots_max = 0
    overflow = False
    explored = max_frontier = 1
    returns = []

    def close(lin, state):
        for j, q in open_reads.items():
            if not (lin >> j) & 1 and _legal(q, *state):
                lin |= 1 << j
        return lin

    def drop(i):
        nonlocal n_open
        rec = recs[i]
        if rec[0] == R:
            del open_reads[i]
        else:
            members = classes[tuple(rec[:4])]
            members.remove(i)
            if not members:
                del classes[tuple(rec[:4])]
        n_open -= 1

    is_open = set()
    for _, is_ret, x in events:
        rec = recs[x]
        if not is_ret:
            if rec[0] == R:
                if rec[5] == INF or (rec[1] == N and rec[3] == N):
                    continue
                if len(frontier) == 1 and _legal(rec, *next(iter(frontier))[1]):
                    continue
            if n_open == WINDOW:
                overflow = True
            n_open += 1
            slots_max = max(slots_max, n_open)
            is_open.add(x)
            if rec[0] == R:
                open_reads[x] = rec
                frontier = {(lin | (1 << x) if _legal(rec, *st) else lin, st)
                            for lin, st in frontier}
            else:
                members = classes.setdefault(tuple(rec[:4]), [])
                members.append(x)
                members.sort(key=lambda j: _deadline(recs[j]))
            continue

        if x not in is_open:
            continue
        bx = 1 << x
        n_f = len(frontier)
        done = {(lin & ~bx, st) for lin, st in frontier if lin & bx}
        work = [c for c in frontier if not c[0] & bx]
        seen = set(work)
        branched = False
        head = 0
        while head < len(work):
            lin, (ver, val) = work[head]
            head += 1
            n_cand = 0
            for members in list(classes.values()):
                t = next((j for j in members if not (lin >> j) & 1), None)
                if t is None or not _legal(recs[t], ver, val):
                    continue
                n_cand += 1
                st = (ver + 1, recs[t][1])
                nl = close(lin | (1 << t), st)
                explored += 1
                if nl & bx:
                    done.add((nl & ~bx, st))
                elif (nl, st) not in seen:
                    seen.add((nl, st))
                    work.append((nl, st))
            branched |= n_cand > 1
        if n_f > 1 or branched:
            returns.append((n_f, len(work), len(done)))
        frontier = done
        is_open.discard(x)
        drop(x)
        max_frontier = max(max_frontier, len(frontier))
        if not frontier:
            return Result(0, x, rec[5], explored, max_frontier, returns, slots_max, overflow)
        everywhere = ~0
        for lin, _ in frontier:
            everywhere &= lin
        if everywhere:
            for j in [j for j in is_open if (everywhere >> j) & 1]:
                is_open.discard(j)
                drop(j)
            frontier = {(lin & ~everywhere, st) for lin, st in frontier}
    return Result(1, -1, -1, explored, max_frontier, returns, slots_max, overflow)


def sizes(res):
    """(largest max(|W|, |R|), largest |R| + |W|, largest |F| entering) over
    the key's general-path returns: what the LDS tier's regions, the
    cooperative tier's pool and the HBM rungs have to hold."""
    if not res.returns:
        return 0, 0, 0
    return (max(max(w, r) for _, w, r in res.returns), max(w + r for _, w, r in res.returns),
            max(f for f, _, _ in res.returns))
