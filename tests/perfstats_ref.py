"""The rules of include/lincheck_perf.h restated in plain Python: events sorted
by (process, position), dicts for the tables.  It shares no code with the
library; tests compare the library's arrays with what `reference` returns."""
import math

NONE = -2 ** 63
INVOKE = 0
COUNTERS = ("valid", "n_events", "n_client", "n_pairs", "n_pending", "n_ignored_completions", "n_mismatched_f",
            "count", "ok", "fail", "info", "t_max", "n_rate_buckets", "n_quant_buckets")


def quantile_index(q, n):
    return min(n - 1, int(math.floor(q * float(n))))


def reference(events, n_f, qs, rate_dt, quant_dt):
    """events: (time, process, f, type) per position -> (tables, summary).
    tables: by_f [n_f][4], comp_pos [n], latency_ns [n], rate [n_f][3][buckets],
    quant [n_f][buckets][n_q], quant_n [n_f][buckets], as nested lists."""
    n = len(events)
    client = [(p, pos) for pos, (t, p, f, ty) in enumerate(events) if p >= 0]
    client.sort()  # rule 3: each process's subsequence, in history order
    t_max = max([events[pos][0] for _, pos in client], default=0)
    n_rate, n_quant = t_max // rate_dt + 1, t_max // quant_dt + 1
    by_f = [[0, 0, 0, 0] for _ in range(n_f)]
    rate = [[[0] * n_rate for _ in range(3)] for _ in range(n_f)]
    comp_pos, latency = [-1] * n, [NONE] * n
    groups = {}
    s = dict.fromkeys(COUNTERS, 0)
    s.update(n_events=n, n_client=len(client), t_max=t_max, n_rate_buckets=n_rate, n_quant_buckets=n_quant)
    for i, (p, pos) in enumerate(client):
        t, _, f, ty = events[pos]
        prev = events[client[i - 1][1]] if i > 0 and client[i - 1][0] == p else None
        nxt = events[client[i + 1][1]] if i + 1 < len(client) and client[i + 1][0] == p else None
        if ty == INVOKE:
            if nxt is None or nxt[3] == INVOKE:
                s["n_pending"] += 1
                continue
            s["n_pairs"] += 1
            s["n_mismatched_f"] += nxt[2] != f
            comp_pos[pos], latency[pos] = client[i + 1][1], nxt[0] - t
            groups.setdefault((f, t // quant_dt), []).append(nxt[0] - t)
        else:
            by_f[f][0] += 1
            by_f[f][ty] += 1
            rate[f][ty - 1][t // rate_dt] += 1
            if prev is None or prev[3] != INVOKE:
                s["n_ignored_completions"] += 1
    quant = [[[NONE] * len(qs) for _ in range(n_quant)] for _ in range(n_f)]
    quant_n = [[0] * n_quant for _ in range(n_f)]
    for (f, b), ls in groups.items():
        ls.sort()
        quant_n[f][b] = len(ls)
        quant[f][b] = [ls[quantile_index(q, len(ls))] for q in qs]
    for k, name in enumerate(("count", "ok", "fail", "info")):
        s[name] = sum(row[k] for row in by_f)
    s["valid"] = int(all(row[1] > 0 for row in by_f if row[0] > 0))
    return {"by_f": by_f, "comp_pos": comp_pos, "latency_ns": latency, "rate": rate, "quant": quant,
            "quant_n": quant_n}, s
