"""An independent restatement of the watch checker (include/lincheck_watch.h)
for the tests: classes by tuple equality, distances from an LCS table (not from
Myers), rule 5's script from a Myers of its own over dicts, and patch(), which
applies a script to a log.  Plain Python over lists; nothing of the library."""


def classes(logs):
    """Per thread, the lowest position with an equal log."""
    first = {}
    return [first.setdefault(tuple(log), i) for i, log in enumerate(logs)]


def canonical(logs):
    """Rule 3 -> the canonical thread's position (None without threads)."""
    if not logs:
        return None
    cls = classes(logs)
    size = {r: cls.count(r) for r in set(cls)}
    reps = sorted(size)
    if max(size.values()) > 1:
        return min(reps, key=lambda r: (-size[r], r))
    return min(reps, key=lambda r: (-len(logs[r]), r))


def lcs(a, b):
    prev = [0] * (len(b) + 1)
    for x in a:
        cur = [0]
        for j, y in enumerate(b):
            cur.append(prev[j] + 1 if x == y else max(prev[j + 1], cur[j]))
        prev = cur
    return prev[len(b)]


def distance(a, b):
    return len(a) + len(b) - 2 * lcs(a, b)


def trim(A, B):
    """Rule 4 -> (p, s)."""
    p = 0
    while p < min(len(A), len(B)) and A[p] == B[p]:
        p += 1
    s = 0
    while s < min(len(A), len(B)) - p and A[len(A) - 1 - s] == B[len(B) - 1 - s]:
        s += 1
    return p, s


DELETE, INSERT = 0, 1


def _down(k, d, v):
    return k == -d or (k != d and v[k - 1] < v[k + 1])


def myers(a, b, base=0):
    """Rule 5 on the middles -> [(op, at, value)] in path order."""
    n, m = len(a), len(b)
    v, rows = {1: 0}, []
    for d in range(n + m + 1):
        rows.append(dict(v))  # V_{d-1}
        for k in range(-d, d + 1, 2):
            x = v[k + 1] if _down(k, d, v) else v[k - 1] + 1
            while x < n and x - k < m and a[x] == b[x - k]:
                x += 1
            v[k] = x
        if abs(n - m) <= d and (d - (n - m)) % 2 == 0 and v[n - m] >= n:
            break
    script, k = [], n - m
    for d in range(len(rows) - 1, 0, -1):
        prev = rows[d]
        if _down(k, d, prev):
            x = prev[k + 1]
            script.append((INSERT, base + x, b[x - (k + 1)]))
            k += 1
        else:
            x = prev[k - 1]
            script.append((DELETE, base + x, a[x]))
            k -= 1
    return script[::-1]


def patch(A, script):
    """The log that the script makes of A; asserts what rule 5 promises."""
    out, i, last = [], 0, 0
    for op, at, value in script:
        assert last <= at <= len(A), (at, last)
        last = at
        out.extend(A[i:at])
        i = max(i, at)
        if op == DELETE:
            assert i == at and A[at] == value, (at, value)
            i = at + 1
        else:
            assert op == INSERT and i == at
            out.append(value)
    out.extend(A[i:])
    return out


def check(logs, revisions, n_nonmonotonic=0, max_d=4096):
    """Rules 2 to 9 -> a dict: cls, canonical, canonical_size, n_classes,
    distance (per thread), deltas [(thread, distance, p, s, script or None)] in
    rule 7's order, valid (True / False / "unknown")."""
    cls = classes(logs)
    canon = canonical(logs)
    dist, deltas = [0] * len(logs), []
    for t, log in enumerate(logs):
        if cls[t] == canon:
            continue
        A, B = logs[canon], log
        p, s = trim(A, B)
        a, b = A[p:len(A) - s], B[p:len(B) - s]
        dist[t] = distance(a, b)
        assert dist[t] == distance(A, B)
        deltas.append((t, dist[t], p, s, myers(a, b, p) if dist[t] <= max_d else None))
    deltas.sort(key=lambda d: (-d[1], d[0]))
    if n_nonmonotonic:
        valid = False
    elif not logs or len(set(revisions)) > 1:
        valid = "unknown"
    else:
        valid = not deltas
    return {"cls": cls, "canonical": canon, "canonical_size": 0 if canon is None else cls.count(canon),
            "n_classes": len(set(cls)), "distance": dist, "deltas": deltas, "valid": valid}
