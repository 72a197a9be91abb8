"""What the witness search (LC_FLAG_SEARCH_WITNESS) costs, and how its
depth-first search compares with the frontier search: per batch, the call
with the flag off and on alternating in one process (median of --calls each
after a warm-up of both), the stage's statistics, and for a sample of keys
checked one at a time the search's steps against the frontier search's
configs_explored.  One JSON line per batch.

    python tools/search_witness_probe.py [--batch model|counted_c|c5] [--calls 5] [--sample 48] [--off-only]

Batches: model — cas-register 1,000 x 1,000 at concurrency 20 (versions
stripped); counted_c — batch C of tests/test_counted.py, each key cut before
its 65th crashed op; c5 — the C5 fixture under LC_FLAG_NO_FAST_PATH.
With a library that lacks the feature (LINCHECK_LIB = the parent commit's, in
a process of its own), or with --off-only, only the flag-off call is timed:
the baseline for "the flag costs nothing when off", and this library's
flag-off call measured the same way (no flag-on call in between).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def load(batch, abi):
    """(ops, key_off, init_value, flags)"""
    if batch == "model":
        ops, off, _, _ = abi.synth(1000, 1000, concurrency=20, seed=7)
        ops = ops.copy()
        ops[:, 3] = -1
        return ops, off, -1, 0
    if batch == "c5":
        z = np.load(os.path.join(ROOT, "tests", "golden", "c5.npz"))
        return z["ops"], z["key_off"], -1, abi.LC_FLAG_NO_FAST_PATH
    import test_counted as t
    from helpers import pack_keys
    keys, init = t.batch("C")
    cut = []
    for recs in keys:
        crashed = 0
        for i, r in enumerate(recs):
            crashed += r[5] == t.INF
            if crashed > 64:
                recs = recs[:i]
                break
        cut.append(recs)
    ops, off = pack_keys(cut)
    return ops, off, init, abi.LC_FLAG_COUNTED_CLASSES


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "calls_ms": [round(x, 3) for x in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="model", choices=["model", "counted_c", "c5"])
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--sample", type=int, default=48)
    ap.add_argument("--off-only", action="store_true")
    a = ap.parse_args()
    from jepsen.etcd_amd import abi
    has = hasattr(abi.lib(), "lc_last_witness_stats") and not a.off_only
    ops, off, init, flags = load(a.batch, abi)
    o_off = abi.default_opts(init_value=init, flags=flags)
    o_on = abi.default_opts(init_value=init, flags=flags | 64)
    out = {"batch": a.batch, "keys": len(off) - 1, "records": len(ops), "feature": has,
           "lib": os.environ.get("LINCHECK_LIB", "tree")}
    t_off, t_on = [], []
    with abi.Context(1) as ctx:
        for i in range(a.calls + 1):
            t0 = time.perf_counter()
            _, r, _, _ = ctx.check(ops, off, o_off, witness=True)
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                t_off.append(dt)
            if not has:
                continue
            t0 = time.perf_counter()
            _, r, wit, kind = ctx.check(ops, off, o_on, witness=True)
            dt = (time.perf_counter() - t0) * 1e3
            if i:
                t_on.append(dt)
        out["flag_off"] = spread(t_off)
        out["valid"], out["invalid"], out["unknown"] = (int((r["verdict"] == v).sum()) for v in (1, 0, -1))
        if has:
            out["flag_on"] = spread(t_on)
            out["stats"] = ctx.last_witness_stats()
            out["kinds"] = {int(k): int((kind == k).sum()) for k in np.unique(kind)}
            # steps per key against the frontier search's configurations:
            # a sample of the keys, one key per call
            idx = np.linspace(0, len(off) - 2, min(a.sample, len(off) - 1)).astype(int)
            ratio, rate = [], []
            for k in idx:
                sub = ops[off[k]:off[k + 1]]
                so = np.array([0, len(sub)], dtype=np.int64)
                _, rk, _, kk = ctx.check(sub, so, o_on, witness=True)
                st = ctx.last_witness_stats()
                if st["n_found"] == 1:
                    ratio.append(st["nodes"] / max(1, int(rk["configs_explored"][0])))
                    rate.append((st["nodes"], st["kernel_ms"], len(sub)))
            if ratio:
                out["nodes_per_config"] = {"keys": len(ratio), "median": round(statistics.median(ratio), 4),
                                           "max": round(max(ratio), 4), "min": round(min(ratio), 4)}
                big = max(rate)
                # one wave's pace: the sampled key with the most steps (its
                # event pass and the launch are in kernel_ms too)
                out["one_key"] = {"nodes": big[0], "kernel_ms": round(big[1], 4), "records": big[2],
                                  "nodes_per_ms": round(big[0] / max(big[1], 1e-9), 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
