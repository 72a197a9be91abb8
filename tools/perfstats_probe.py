"""Dev: lc_perf_stats (the composed checker's :stats and :perf on the device)
against lc_perf_stats_host, this project's single-threaded host function
(jepsen cannot run here), on one GPU.

Workload: a numpy-built history shaped like tools/edn_e2e.py's (concurrency
20, 2 % of the ops crash with :info and the thread goes on under a new process
id, three :f) with :time added: an op takes 0.2-2 ms, a thread thinks up to
1 ms between ops.  Default sizes: 2.5 M events (edn_e2e.py's) and 24.9 M (C2's,
as tools/events_probe.py --synth).  The two functions alternate in one process
on the same arrays: one warm-up of each, then `reps` of each; medians and
ranges, with the device call's h2d_ms / kernel_ms / total_ms from its summary
and its wall time as the caller sees it (the binding's allocations included).
The encoding of op maps into records is not timed.
    python tools/perfstats_probe.py [events ...] [--reps N] [--no-points]
Prints one JSON line per size."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from jepsen.etcd_amd import abi  # noqa: E402

CONCURRENCY, N_F, P_INFO = 20, 3, 0.02
COUNTERS = ("valid", "n_client", "n_pairs", "n_pending", "n_ignored_completions", "n_mismatched_f", "count", "ok",
            "fail", "info", "t_max", "n_rate_buckets", "n_quant_buckets")


def spread(xs):
    return {"median": round(statistics.median(xs), 3), "min": round(min(xs), 3), "max": round(max(xs), 3)}


def history(n_events, seed=5):
    """-> an abi.PS_EVENT_DTYPE array of about n_events records, ordered by time."""
    rng = np.random.default_rng(seed)
    m = n_events // (2 * CONCURRENCY)  # ops per thread
    parts = []
    for thread in range(CONCURRENCY):
        latency = rng.integers(200_000, 2_000_000, size=m)
        think = rng.integers(1, 1_000_000, size=m)
        invoke = np.cumsum(latency + think) - latency
        u = rng.random(m)
        ctype = np.where(u < P_INFO, abi.LC_EV_INFO, np.where(u < 0.1, abi.LC_EV_FAIL, abi.LC_EV_OK))
        crashes = np.cumsum(ctype == abi.LC_EV_INFO) - (ctype == abi.LC_EV_INFO)  # before this op
        process = thread + CONCURRENCY * crashes
        f = rng.integers(0, N_F, size=m)
        ev = np.zeros(2 * m, dtype=abi.PS_EVENT_DTYPE)
        ev["time"] = np.concatenate([invoke, invoke + latency])
        ev["process"] = np.concatenate([process, process])
        ev["f"] = np.concatenate([f, f])
        ev["type"] = np.concatenate([np.zeros(m, dtype=np.uint8), ctype.astype(np.uint8)])
        parts.append(ev)
    ev = np.concatenate(parts)
    return ev[np.argsort(ev["time"], kind="stable")]


def probe(n_events, reps, points):
    ev = history(n_events)
    out = {"events": len(ev), "points": points, "reps": reps, "record_bytes": ev.nbytes}
    dev_wall, host_wall, sums = [], [], []
    with abi.Context(device_mask=1) as ctx:
        for rep in range(reps + 1):
            a = time.perf_counter()
            got, gs = ctx.perf_stats(ev, N_F, points=points)
            b = time.perf_counter()
            want, ws = abi.perf_stats_host(ev, N_F, points=points)
            c = time.perf_counter()
            assert all(gs[k] == ws[k] for k in COUNTERS), (gs, ws)
            assert all(got[k] is None if want[k] is None else (got[k] == want[k]).all() for k in want)
            if rep:
                dev_wall.append((b - a) * 1e3)
                host_wall.append((c - b) * 1e3)
                sums.append((gs, ws))
    out["device_wall_ms"] = spread(dev_wall)
    for k in ("total_ms", "h2d_ms", "kernel_ms"):
        out["device_" + k] = spread([g[k] for g, _ in sums])
    out["host_wall_ms"] = spread(host_wall)
    out["host_total_ms"] = spread([w["total_ms"] for _, w in sums])
    for k in ("n_client", "n_pairs", "n_pending", "n_rate_buckets", "n_quant_buckets", "valid"):
        out[k] = sums[-1][0][k]
    print(json.dumps(out), flush=True)


def main(argv):
    reps, points, sizes = 5, True, []
    it = iter(argv)
    for a in it:
        if a == "--reps":
            reps = int(next(it))
        elif a == "--no-points":
            points = False
        else:
            sizes.append(int(a))
    for n in sizes or (2_500_000, 24_900_000):
        probe(n, reps, points)


if __name__ == "__main__":
    main(sys.argv[1:])
