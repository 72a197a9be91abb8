"""What the counted witness stage (LC_FLAG_COUNTED_WITNESS) costs.  One JSON
line per batch.

    python tools/counted_witness_probe.py --leg stage [--batches ABC] [--calls 5]
    python tools/counted_witness_probe.py --leg off --batch model|counted_c [--calls 5]

--leg stage: batches A, B, C of tests/test_counted.py under
LC_FLAG_COUNTED_CLASSES | LC_FLAG_SEARCH_WITNESS, the call with
LC_FLAG_COUNTED_WITNESS off and on alternating in one process (median of
--calls each after a warm-up of both): host wall time of lc_check_ex, the
stage's kernel_ms / nodes / cache_hits, the first stage's statistics and,
from the same call, the counted tier's own kernel_ms (lc_last_counted_stats):
the stage against the tier that decided the same keys.  The key with the most
steps is then checked alone: one wave's pace.

--leg off: the call WITHOUT the new flag, for a comparison with the parent
commit's library (LINCHECK_LIB, each library in processes of its own,
alternating): model — cas-register 1,000 x 1,000 at concurrency 20, versions
stripped, LC_FLAG_SEARCH_WITNESS; counted_c — batch C with
LC_FLAG_COUNTED_CLASSES | LC_FLAG_SEARCH_WITNESS.
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

CC, SW, CW = 32, 64, 128


def spread(ms):
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3),
            "max_ms": round(max(ms), 3), "calls_ms": [round(x, 3) for x in ms]}


def timed(ctx, ops, off, o):
    t0 = time.perf_counter()
    out = ctx.check(ops, off, o, witness=True)
    return (time.perf_counter() - t0) * 1e3, out


def stage(abi, name, calls):
    import test_counted as t
    ops, off, init = t.packed(name)
    o_off = abi.default_opts(init_value=init, flags=CC | SW)
    o_on = abi.default_opts(init_value=init, flags=CC | SW | CW)
    out = {"leg": "stage", "batch": name, "keys": len(off) - 1, "records": len(ops)}
    t_off, t_on, k_ms, tier_ms = [], [], [], []
    with abi.Context(1) as ctx:
        for i in range(calls + 1):
            dt, _ = timed(ctx, ops, off, o_off)
            if i:
                t_off.append(dt)
            dt, (_, res, wit, kind) = timed(ctx, ops, off, o_on)
            if i:
                t_on.append(dt)
                k_ms.append(ctx.last_counted_witness_stats()["kernel_ms"])
                tier_ms.append(ctx.counted_stats()["kernel_ms"])
        out["flag_off"], out["flag_on"] = spread(t_off), spread(t_on)
        out["stage"] = ctx.last_counted_witness_stats()
        out["stage_kernel_ms"] = spread(k_ms)
        out["counted_tier"] = ctx.counted_stats()
        out["counted_tier_kernel_ms"] = spread(tier_ms)
        out["first_stage"] = ctx.last_witness_stats()
        out["kinds"] = {int(k): int((kind == k).sum()) for k in np.unique(kind)}
        out["valid"], out["invalid"], out["unknown"] = (int((res["verdict"] == v).sum()) for v in (1, 0, -1))
        # one wave's pace: every key alone, the one with the most steps reported
        best = None
        for k in range(len(off) - 1):
            sub = ops[off[k]:off[k + 1]]
            ctx.check(sub, np.array([0, len(sub)], dtype=np.int64), o_on, witness=True)
            st = ctx.last_counted_witness_stats()
            if st["n_found"] == 1 and (best is None or st["nodes"] > best[0]):
                best = (st["nodes"], st["kernel_ms"], st["cache_hits"], len(sub), k)
        if best:
            out["one_key"] = {"key": best[4], "records": best[3], "nodes": best[0], "cache_hits": best[2],
                              "kernel_ms": round(best[1], 4),
                              "nodes_per_ms": round(best[0] / max(best[1], 1e-9), 1)}
    return out


def off_leg(abi, batch, calls):
    if batch == "model":
        ops, off, _, _ = abi.synth(1000, 1000, concurrency=20, seed=7)
        ops = ops.copy()
        ops[:, 3] = -1
        init, flags = -1, SW
    else:
        import test_counted as t
        ops, off, init = t.packed("C")
        flags = CC | SW
    o = abi.default_opts(init_value=init, flags=flags)
    ms = []
    with abi.Context(1) as ctx:
        for i in range(calls + 1):
            dt, (_, res, _, kind) = timed(ctx, ops, off, o)
            if i:
                ms.append(dt)
        st = ctx.last_witness_stats()
    return {"leg": "off", "batch": batch, "lib": os.environ.get("LINCHECK_LIB", "tree"),
            "keys": len(off) - 1, "records": len(ops), "call": spread(ms), "first_stage": st,
            "kinds": {int(k): int((kind == k).sum()) for k in np.unique(kind)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="stage", choices=["stage", "off"])
    ap.add_argument("--batches", default="ABC")
    ap.add_argument("--batch", default="model", choices=["model", "counted_c"])
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from jepsen.etcd_amd import abi
    if a.leg == "off":
        print(json.dumps(off_leg(abi, a.batch, a.calls)), flush=True)
        return
    for name in a.batches:
        print(json.dumps(stage(abi, name, a.calls)), flush=True)


if __name__ == "__main__":
    main()
