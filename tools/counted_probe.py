"""Time one lc_check of a crash-heavy batch (tests/test_counted.py, batches
A-C) with the counted tier (LC_FLAG_COUNTED_CLASSES) or, with --baseline,
with LC_FLAG_WHOLE_GPU alone (the frontier exchange takes the window-overflow
keys one engine each): median of --calls calls after one warm-up, one JSON line.

    python tools/counted_probe.py [--batch A] [--baseline] [--calls 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="A", choices=["A", "B", "C"])
    ap.add_argument("--baseline", action="store_true")
    ap.add_argument("--calls", type=int, default=5)
    a = ap.parse_args()
    from jepsen.etcd_amd import abi
    import test_counted as t
    ops, off, init = t.packed(a.batch)
    flags = abi.LC_FLAG_WHOLE_GPU if a.baseline else abi.LC_FLAG_COUNTED_CLASSES
    o = abi.default_opts(init_value=init, flags=flags)
    ms, counted = [], None
    with abi.Context(1) as ctx:
        for i in range(a.calls + 1):
            t0 = time.perf_counter()
            _, r = ctx.check(ops, off, o)
            dt = (time.perf_counter() - t0) * 1e3
            if i:  # (the first call warms up: allocations, engines)
                ms.append(dt)
        if not a.baseline:
            counted = ctx.counted_stats()
        st = ctx.stats()
    print(json.dumps({
        "batch": a.batch, "mode": "whole-gpu" if a.baseline else "counted", "keys": len(r),
        "median_ms": round(statistics.median(ms), 3), "calls_ms": [round(x, 3) for x in ms],
        "valid": int((r["verdict"] == 1).sum()), "invalid": int((r["verdict"] == 0).sum()),
        "unknown": int((r["verdict"] == -1).sum()),
        "explored": int(r["configs_explored"].sum()), "counted_stats": counted,
        "kernel_ms": st["kernel_ms"], "hbm_kernel_ms": st["hbm_kernel_ms"],
    }))


if __name__ == "__main__":
    main()
