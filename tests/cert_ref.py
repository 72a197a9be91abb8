"""Python restatement of the device's certificate finder (cert_kernel in
jepsen/etcd_amd/csrc/cert.hip) — test infrastructure.  Given an invalid
key's records and its failing return `cut`, name facts that rule out every
linearization of the prefix at `cut` (the kinds of include/lincheck.h,
LC_CERT_*).  oracle/cert.c checks what either finder emits from the records
alone; a finder can only fail to find a certificate, never make a wrong one
pass.

The restatement follows the kernel stage by stage, and within a stage makes
the kernel's choice among equally valid answers, so that the device's
certificate can be compared field for field (tests/test_gpu_cert_edges.py):
  UNREACH  over the whole key first: the lowest record;
  DUP      then the lowest (lowest holder of the version, another holder);
  CLAIMS   then the lowest (lowest valued read of the version, a read of
           another value);
  PAIR     the lowest consumer position q, then the lowest consumer record;
  ORDER    the lowest index whose lower bound lies above the suffix minimum
           of the upper bounds, each bound with the record that sets it;
  HALL     the lowest open position without a candidate;
  PAIR     the lowest open q whose sole candidate, a CAS, disagrees;
  HALL     every open position, ascending;
  PROOF    the search of wave 0, loop iteration by loop iteration: the node
           count (one per iteration: closed case, forced step or split), the
           frame cap (cert_layout.h) and the token cap (one per record).
The kernel's kWork cap on candidate checks (2^22 per lane) is not restated:
no key of the suite's sizes comes near it within the node cap.

find(recs, cut) -> (kind, a, b, c, positions)."""
INF = (1 << 63) - 1
NIL = -1
R, W, C = 0, 1, 2
NONE, DUP, UNREACH, CLAIMS, PAIR, ORDER, HALL, PROOF = range(8)
# PROOF tokens (include/lincheck.h LC_CERT_PROOF): kind << 30 | a << 15 | b
FORCE, BRANCH, EMPTY = 1, 2, 3
PROOF_NODES = 2048  # search budget (the device finder's kNodes, cert.hip)
FREE = None         # no value fixed (the kernel's kFree)


def tok(kind, a, b=0):
    """One proof token as the int32 the certificate set holds."""
    x = (kind << 30) | (a << 15) | b
    return x - (1 << 32) if x >= (1 << 31) else x


def untok(t):
    t &= 0xFFFFFFFF
    return t >> 30, (t >> 15) & 0x7FFF, t & 0x7FFF


def n_frames(n):
    """Case-split frames the PROOF search of an n-record key may have open
    (cert_layout.h, cert_n_frames): the key's scratch holds 2 (n + 2) ints,
    the log of assumed positions takes n + 2, a frame takes 4."""
    return (2 * (n + 2) - (n + 2)) // 4


class _Tables:
    """What the fixed stages leave for the candidate scans."""


def find(recs, cut, v0=0, init=-1, proof=True, proof_budget=PROOF_NODES, stats=None):
    n = len(recs)
    inp = [r[4] <= cut for r in recs]
    req = [inp[i] and recs[i][5] <= cut for i in range(n)]
    mut = [r[0] in (W, C) for r in recs]
    n_mut = sum(1 for i in range(n) if inp[i] and mut[i])
    # UNREACH; and the positions held, the claims, the bounds of the required ops
    held, held_cnt, claim, lo, uh = {}, {}, {}, {}, {}
    unreach, M = [], 0
    for r, (f, val, exp, ver, call, ret) in enumerate(recs):
        if not req[r] or ver == NIL:
            continue
        if mut[r]:
            pos = ver - v0 - 1
            if pos < 0 or pos + 1 > n_mut:
                unreach.append(r)
                continue
            held_cnt[pos] = held_cnt.get(pos, 0) + 1
            held[pos] = min(held.get(pos, r), r)
            lo[pos] = max(lo.get(pos, (-1, -1)), (call, r))
            uh[pos] = min(uh.get(pos, (INF, INF)), (ret, r))
            M = max(M, pos + 1)
        elif f == R:
            k = ver - v0
            if k < 0 or k > n_mut or (k == 0 and val != NIL and val != init):
                unreach.append(r)
                continue
            if val != NIL:
                claim[k] = min(claim.get(k, r), r)
            lo[k] = max(lo.get(k, (-1, -1)), (call, r))
            if k > 0:
                uh[k - 1] = min(uh.get(k - 1, (INF, INF)), (ret, r))
            M = max(M, k)
    if unreach:
        return (UNREACH, min(unreach), -1, 0, [])
    # DUP
    best = None
    for r in range(n):
        if not req[r] or not mut[r] or recs[r][3] == NIL:
            continue
        pos = recs[r][3] - v0 - 1
        if held_cnt[pos] > 1 and held[pos] != r:
            best = min(best or (held[pos], r), (held[pos], r))
    if best:
        return (DUP, best[0], best[1], 0, [])
    # CLAIMS
    for r in range(n):
        if not req[r] or recs[r][0] != R or recs[r][3] == NIL or recs[r][1] == NIL:
            continue
        o = claim[recs[r][3] - v0]
        if o != r and recs[o][1] != recs[r][1]:
            best = min(best or (o, r), (o, r))
    if best:
        return (CLAIMS, best[0], best[1], 0, [])
    # PAIR against a required holder: the lowest consumer position q, then
    # its lowest consumer
    def consumer(r):
        f, val, exp, ver = recs[r][:4]
        if not req[r] or ver == NIL:
            return None
        if f == C:
            return ver - v0 - 1, exp
        if f == R and val != NIL:
            return ver - v0, val
        return None

    def clashes(r):
        qw = consumer(r)
        if qw is None:
            return None
        q, want = qw
        if q == 0:
            return q if recs[r][0] == C and want != init else None
        return q if q >= 1 and q - 1 in held and recs[held[q - 1]][1] != want else None

    qs = [q for q in map(clashes, range(n)) if q is not None]
    if qs:
        q = min(qs)
        return (PAIR, held[q - 1] if q else -1, min(r for r in range(n) if clashes(r) == q), q, [])
    # ORDER: the suffix minimum of the upper bounds over indices 0..M, then
    # the lowest index whose lower bound lies above it
    suf, run = {}, (INF, INF)
    for k in range(M, -1, -1):
        run = min(run, uh.get(k, (INF, INF)))
        suf[k] = run
    for k in range(M + 1):
        if k in lo and lo[k][0] > suf[k][0]:
            return (ORDER, lo[k][1], suf[k][1], 0, [])
    # the open positions (needed, held by no required op) and their
    # candidates: the mutations of the prefix without a version, in record
    # (call) order, and the pending :ok mutations pinned to the position
    # (the kernel's list: the highest record first)
    t = _Tables()
    t.recs, t.held, t.claim, t.init, t.M = recs, held, claim, init, M
    t.ulist = [r for r in range(n) if inp[r] and mut[r] and recs[r][3] == NIL]
    t.pins = {}
    for r in range(n):
        if inp[r] and mut[r] and recs[r][3] != NIL and not req[r]:
            g = recs[r][3] - v0 - 1
            if 0 <= g <= n:
                t.pins.setdefault(g, []).insert(0, r)
    t.dl = {g: suf[g][0] for g in range(M)}
    t.fixed = {}
    gaps = [g for g in range(M) if g not in held]
    cands = {g: _cands(t, g, {}, set()) for g in gaps}
    for g in gaps:
        if not cands[g]:
            return (HALL, -1, -1, 1, [g])
    # two open positions whose only candidates disagree on the value between
    # them.  (The kernel also looks at a required holder of q-1; that cannot
    # fire: a CAS expecting another value than a required holder left is no
    # candidate of q — _fits — so q is empty and the stage above has it.  Kept
    # as the kernel has it.)
    for q in gaps:
        if q < 1 or len(cands[q]) != 1 or recs[cands[q][0]][0] != C:
            continue
        b = cands[q][0]
        a = held.get(q - 1)
        if a is None and q - 1 in cands and len(cands[q - 1]) == 1:
            a = cands[q - 1][0]
        if a is not None and recs[a][1] != recs[b][2]:
            return (PAIR, a, b, q, [])
    # Hall's condition over every open position
    union = set()
    for g in gaps:
        union.update(cands[g])
    if len(gaps) > len(union):
        return (HALL, -1, -1, len(gaps), gaps)
    # Infeasibility that only a search finds (a choice at one open position
    # fixes the value or uses the op another one needs): a proof by forced
    # choices and case splits over the candidates (LC_CERT_PROOF)
    if not proof or not gaps or n > 0x7FFF or M > 0x7FFF:
        return (NONE, -1, -1, 0, [])
    toks = prove(t, gaps, n, proof_budget, stats)
    if toks is not None:
        return (PROOF, -1, -1, len(toks), toks)
    return (NONE, -1, -1, 0, [])


def _fixed(t, g):
    """What the required ops alone fix for open position g: the value its
    holder must write, the value a CAS holding it must expect, and the ops
    that pass both and the deadline — in the kernel's scan order: the
    version-less ones called before the deadline, then the pinned list.
    None: the required ops' claims on g clash."""
    if g in t.fixed:
        return t.fixed[g]
    recs, held, claim = t.recs, t.held, t.claim
    want, before, clash = FREE, FREE, False
    if g + 1 in held and recs[held[g + 1]][0] == C:
        want = recs[held[g + 1]][2]
    if g + 1 in claim:
        v = recs[claim[g + 1]][1]
        clash = want is not FREE and want != v
        want = v
    if g == 0:
        before = t.init
    elif g - 1 in held:
        before = recs[held[g - 1]][1]
    elif g in claim:
        before = recs[claim[g]][1]
    dl = t.dl[g]
    out = []
    for x in t.ulist:
        if recs[x][4] >= dl:
            break  # (call order)
        if _fits(recs[x], want, before):
            out.append(x)
    for x in t.pins.get(g, ()):
        if recs[x][4] < dl and _fits(recs[x], want, before):
            out.append(x)
    t.fixed[g] = None if clash else (want, before, out)
    return t.fixed[g]


def _fits(rec, want, before):
    f, val, exp = rec[:3]
    if f == C and before is not FREE and exp != before:
        return False
    return want is FREE or val == want


def _cands(t, g, asg, used):
    """The candidates of open position g under the assumptions (asg:
    position -> record, used: the records assumed): an assumed CAS above g
    fixes what g's holder writes, an assumed holder below g what a CAS at g
    expects, where the required ops leave that free.  (The assumptions only
    narrow what _fixed lists, so the scan starts from its list.)"""
    fx = _fixed(t, g)
    if fx is None:
        return []
    want, before, lst = fx
    recs = t.recs
    if g + 1 < t.M and g + 1 in asg and recs[asg[g + 1]][0] == C:
        v = recs[asg[g + 1]][2]
        if want is not FREE and want != v:
            return []
        want = v
    if before is FREE and g - 1 in asg:
        before = recs[asg[g - 1]][1]
    return [x for x in lst if x not in used and _fits(recs[x], want, before)]


def prove(t, gaps, n, budget=PROOF_NODES, stats=None):
    """The proof's tokens — one BRANCH(position, cases) per case split, in
    preorder — or None (a complete consistent assignment exists, or the
    search ran over its node budget, its frames or the key's token room).
    The kernel's loop: every iteration is a node; at the current assumptions
    an open position with no candidate (the checker re-derives that) closes
    the case — back to the innermost split with a case left, its next case
    the lowest candidate above the one just closed — else the lowest position
    with exactly one candidate is assumed held by it, else a split is taken
    at the position with the fewest candidates (the lowest among equals), its
    first case the lowest candidate.  stats (a dict) receives the node count
    and the deepest frame stack."""
    asg, used, log, frames, toks = {}, set(), [], [], []
    nodes, deepest, cap = 0, 0, n_frames(n)

    def done(result):
        if stats is not None:
            stats.update(nodes=nodes, depth=deepest, tokens=len(toks))
        return result

    while True:
        nodes += 1
        if nodes > budget:
            return done(None)
        open_ = [g for g in gaps if g not in asg]
        if not open_:
            return done(None)  # every open position held: no contradiction here
        cs = {g: sorted(_cands(t, g, asg, used)) for g in open_}
        if any(not cs[g] for g in open_):
            resumed = False
            while frames:
                g, k, i, z, w = frames[-1]
                while len(log) > z:
                    used.discard(asg.pop(log.pop()))
                if i + 1 < k:
                    x = min(c for c in _cands(t, g, asg, used) if c > w)
                    frames[-1] = (g, k, i + 1, z, x)
                    asg[g] = x
                    used.add(x)
                    log.append(g)
                    resumed = True
                    break
                frames.pop()  # every case of this split closed: the case around it is too
            if resumed:
                continue
            return done(toks)
        one = [g for g in open_ if len(cs[g]) == 1]
        if one:  # forced (the checker re-derives it: no token)
            g = one[0]
            asg[g] = cs[g][0]
            used.add(cs[g][0])
            log.append(g)
            continue
        g = min(open_, key=lambda q: (len(cs[q]), q))
        k = len(cs[g])
        if len(frames) >= cap or k > 0x7FFF or len(toks) >= n:
            return done(None)
        toks.append(tok(BRANCH, g, k))
        frames.append((g, k, 0, len(log), cs[g][0]))
        deepest = max(deepest, len(frames))
        asg[g] = cs[g][0]
        used.add(cs[g][0])
        log.append(g)
