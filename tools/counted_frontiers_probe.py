"""Time the diagnostics step (knossos's :configs) for a batch of crash-heavy
mutex keys, the way RegisterChecker runs it: the batched slot search
(lc_check_frontiers, which leaves these keys out), then either the one-key
fallback (FrontierExchange.frontier, key by key: --path fallback) or one call
over the counted search (lc_check_frontiers_counted: --path counted).  With
--path both the two alternate, round by round.  Median of --rounds rounds
after one warm-up each; one JSON line per path.

The batch: 16 keys shaped like K1 / K2 of tests/test_counted_frontiers.py with
70-250 crashed ops each, every one invalid at its last :ok op with a frontier
of one configuration and all its crashed acquires / releases pending.

    python tools/counted_frontiers_probe.py [--path both] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def keys():
    """(records, fail op, pending ops at the failure) per key."""
    from helpers import FREE, HELD, INF, C, N
    acq, rel = [C, HELD, FREE, N], [C, FREE, HELD, N]
    out = []
    for i in range(16):
        m = 70 + 12 * i
        if i % 2 == 0:  # K1: m crashed acquires, two :ok acquires
            recs = [acq + [t, INF] for t in range(m)] + [acq + [m, m + 1], acq + [m + 2, m + 3]]
        else:           # K2: m crashed releases, three crashed acquires, four :ok releases
            recs, t = [], 0
            for j in range(m):
                recs.append(rel + [t, INF]); t += 1
                if j < 3:
                    recs.append(acq + [t, INF]); t += 1
            for _ in range(4):
                recs.append(rel + [t, t + 1]); t += 2
        out.append((recs, len(recs) - 1, m + 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--path", default="both", choices=["both", "fallback", "counted"])
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    from helpers import FREE, pack_keys
    from jepsen.etcd_amd import abi
    from jepsen.etcd_amd.fx import FrontierExchange
    ks = keys()
    ops, off = pack_keys([k[0] for k in ks])
    stops = np.array([k[1] for k in ks], dtype=np.int64)
    o = abi.default_opts(init_value=FREE)
    paths = ["fallback", "counted"] if a.path == "both" else [a.path]
    ms = {p: [] for p in paths}
    listed = {}
    with abi.Context(1) as ctx, FrontierExchange(device=0) as fx:
        for rnd in range(a.rounds + 1):
            for p in paths:
                t0 = time.perf_counter()
                got = ctx.check_frontiers(ops, off, stops, 10, o)
                left = [k for k, c in enumerate(got) if c is None]
                if p == "counted":
                    sub_ops, sub_off = pack_keys([ks[k][0] for k in left])
                    more, _ = ctx.check_frontiers_counted(sub_ops, sub_off, stops[left], 10, o)
                else:
                    more = [fx.frontier(ops[off[k]:off[k + 1]], int(stops[k]), 10, o) for k in left]
                dt = (time.perf_counter() - t0) * 1e3
                if rnd:  # (the first round warms up: allocations, the engine)
                    ms[p].append(dt)
                assert len(left) == len(ks) and all(c is not None and len(c) == 1 for c in more)
                listed[p] = [len(c[0][2]) for c in more]
    for p in paths:
        print(json.dumps({
            "path": p, "lib": os.environ.get("LINCHECK_LIB", "tree"), "keys": len(ks),
            "crashed": [k[2] - 1 for k in ks], "median_ms": round(statistics.median(ms[p]), 3),
            "rounds_ms": [round(x, 3) for x in ms[p]], "pending_listed": listed[p],
            "pending_whole": [k[2] for k in ks]}))


if __name__ == "__main__":
    main()
